// wfs_evtable.h -- the event-offset table the event-local builds start from (include/wfsparse.h wfs_event_offsets):
//     off[e]              first row of event e, e = 0 .. B; off[B] = number of valid rows
//     off[B + 1 + blk]    1 if block blk saw a batch index outside [0, B) or smaller than its predecessor's
// One body for every kernel that writes it: wfs_event_offsets' own (evrulebook.hip) and the two batch hand-overs
// (optim.hip), which walk the batch column of the SOURCE rows inside their copy launch.
#pragma once
#include "wfs_common.h"

// Called by ALL 256 threads of each of the first `nblocks` blocks of a launch (it holds a block barrier); `col` is the
// batch column of the [nv, cols] rows.  Every word of the table is written by every launch (no clearing).
__device__ __forceinline__ void wfs_event_table_block(const int *__restrict__ rows, long long nv, int cols, int col, int B,
                                                      int *__restrict__ off, int nblocks) {
    int bad = 0;
    if (nv == 0)
        for (int e = blockIdx.x * 256 + threadIdx.x; e <= B; e += nblocks * 256) off[e] = 0;
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < nv; j += (long long)nblocks * 256) {
        const int b = rows[j * cols + col];
        const int bp = j > 0 ? rows[(j - 1) * cols + col] : -1;
        const bool ok = b >= 0 && b < B && b >= bp && bp >= -1 && bp < B;
        bad |= ok ? 0 : 1;
        if (ok) {
            for (int e = bp + 1; e <= b; ++e) off[e] = (int)j;
            if (j == nv - 1)
                for (int e = b + 1; e <= B; ++e) off[e] = (int)nv;
        }
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) off[B + 1 + blockIdx.x] = bad;
}
