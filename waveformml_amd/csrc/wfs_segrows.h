// wfs_segrows.h -- the head of a row in the per-segment evaluation kernels (segstats.hip, zreal.hip, segquant.hip,
// metricpairs.hip): coordinates, their two checks and the row run of the row's event; beside it the count of an event's
// single-ended rows and the PID column with its map (zreal.hip, segquant.hip).  Included into each file's anonymous
// namespace, after wfs_evoffsets.h.
#pragma once
#include "wfs_common.h"

// The row run [first, last) of event e from the offsets of k_eval_offsets, clamped to [0, valid rows] with
// last >= first.  On a batch that sets no flag the clamp changes nothing -- k_eval_offsets writes every entry within
// [0, valid rows] in non-decreasing order, so last - first is off[e + 1] - off[e] -- and on a flagged batch results()
// raises whatever the tables hold; the clamp only keeps the walks over a run inside the rows.
__device__ __forceinline__ void event_run(const int *off, int e, long long nv, long long *first, long long *last) {
    long long lo = off[e], hi = off[e + 1];
    lo = lo < 0 ? 0 : (lo > nv ? nv : lo);
    hi = hi < 0 ? 0 : (hi > nv ? nv : hi);
    *first = lo, *last = hi < lo ? lo : hi;   // hi < lo only with a flagged (unsorted) event column
}

struct SegRow {
    int x, y, e, cell;                        // cell = x * ny + y
    long long first, last;                    // event_run of e
    bool ok;                                  // false: a flag is set; cell and the run are 0
};
// row r < nv of coords [N, 3] = (x, y, event): the event first (flag 1), then the grid (flag 2)
__device__ __forceinline__ SegRow seg_row(const int *coords, long long r, long long nv, const int *off, int E, int nx,
                                          int ny, int *flags) {
    SegRow h;
    h.x = coords[r * 3], h.y = coords[r * 3 + 1], h.e = coords[r * 3 + 2];
    h.cell = 0, h.first = h.last = 0;
    h.ok = false;
    if (h.e < 0 || h.e >= E) {
        atomicOr(flags, 1);                   // k_eval_offsets has set it already
        return h;
    }
    if (h.x < 0 || h.x >= nx || h.y < 0 || h.y >= ny) {
        atomicOr(flags, 2);                   // a segment outside the detector
        return h;
    }
    h.cell = h.x * ny + h.y;
    event_run(off, h.e, nv, &h.first, &h.last);
    h.ok = true;
    return h;
}

// the single-ended rows among [first, last): the multiplicity coo[SE_inds] shows.  A row outside the grid is not
// counted; it raises flag 2 itself.
__device__ __forceinline__ int count_single_ended(const int *coords, long long first, long long last, const float *seg,
                                                  int nx, int ny) {
    int n = 0;
    for (long long q = first; q < last; ++q) {
        const int qx = coords[q * 3], qy = coords[q * 3 + 1];
        if (qx >= 0 && qx < nx && qy >= 0 && qy < ny && seg[qx * ny + qy] == 0.5f) ++n;
    }
    return n;
}

// the PID column, int32 or int64
__device__ __forceinline__ long long ld_pid(const void *pid, int is_int64, long long r) {
    return is_int64 ? static_cast<const long long *>(pid)[r] : (long long)static_cast<const int *>(pid)[r];
}
// class_PIDs in order (1 | 4 | 6, 258 | 256 | 512): the slot of a PID, -1 for one the map does not name, and the
// slot's class
__device__ __forceinline__ int pid_slot(long long pid) {
    return pid == 1 ? 0 : pid == 4 ? 1 : pid == 6 ? 2 : pid == 258 ? 3 : pid == 256 ? 4 : pid == 512 ? 5 : -1;
}
__device__ __forceinline__ int pid_slot_class(int slot) { return slot < 3 ? slot : slot - 1; }
// convert_PID(PID, PID_MAP): a PID the map does not name stays as it is
__device__ __forceinline__ long long pid_class(long long pid) {
    const int s = pid_slot(pid);
    return s >= 0 ? pid_slot_class(s) : pid;
}
