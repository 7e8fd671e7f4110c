// wfs_evoffsets.h -- the event-offset table of the evaluation kernels (evalstats.hip, segstats.hip, zreal.hip,
// segquant.hip, metricpairs.hip): the first row of every event from a sorted event column.  Included into each file's
// anonymous namespace.
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

// the launch over n_cap rows (one workgroup when there is none) with its check
inline int launch_eval_offsets(const int *coords, long long n_cap, const long long *n_dev, int E, int *off, int *flags,
                               hipStream_t s) {
    const unsigned rb = (unsigned)(n_cap > 0 ? wfs_cdiv(n_cap, WFS_EVOFF_THREADS) : 1);
    k_eval_offsets<<<rb, WFS_EVOFF_THREADS, 0, s>>>(coords, n_cap, n_dev, E, off, flags);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}

// the batch arguments of the entry points that launch it; `what` is the entry point's name and its word for the event
// count ("name: B").  wfs_zreal_row_stats names its class count in the same message and keeps its own statement.
#define WFS_REQUIRE_EVAL_BATCH(what, E, n_cap, nx, ny)                                                       \
    WFS_REQUIRE((E) >= 1 && (n_cap) >= 0 && (n_cap) < (1ll << 31) && (nx) >= 1 && (ny) >= 1, WFS_EINVAL,     \
                what " = %d, n_cap = %lld, grid %d x %d", E, (long long)(n_cap), nx, ny)
