// wfs_evoffsets.h -- the event-offset table of the evaluation kernels (evalstats.hip, segstats.hip): the first row of
// every event from a sorted event column.  Included into each file's anonymous namespace.
#pragma once
#include "wfs_common.h"

constexpr int WFS_EVOFF_THREADS = 256;


// one thread per row; off [E + 1].  An event without rows gets the offset of the next event that has some (a run of
// length 0).  flags bit 1: event column not sorted / outside [0, E); the offsets of such a batch are not meaningful (but
// every entry written lies in [0, valid rows]).
__global__ void __launch_bounds__(WFS_EVOFF_THREADS)
k_eval_offsets(const int *__restrict__ coords, long long n_cap, const long long *__restrict__ n_dev, int E,
               int *__restrict__ off, int *__restrict__ flags) {
    const long long nv = wfs_valid_rows_nonneg(n_cap, n_dev);
    const long long r = (long long)blockIdx.x * WFS_EVOFF_THREADS + threadIdx.x;
    if (nv == 0) {
        if (r == 0)
            for (int k = 0; k <= E; ++k) off[k] = 0;
        return;
    }
    if (r >= nv) return;
    const int e = coords[r * 3 + 2];
    const int ep = r > 0 ? coords[(r - 1) * 3 + 2] : -1;
    const bool ok = e >= 0 && e < E && ep >= -1 && ep <= e;
    if (!ok)
        atomicOr(flags, 1);                  // event column not sorted / out of range
    else
        for (int k = ep + 1; k <= e; ++k) off[k] = (int)r;
    if (r == nv - 1) {
        if (ok)
            for (int k = e + 1; k < E; ++k) off[k] = (int)nv;
        off[E] = (int)nv;
    }
}
