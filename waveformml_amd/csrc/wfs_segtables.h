// wfs_segtables.h -- what the evaluation kernels with fixed-point tables share (segstats.hip, zreal.hip, metricpairs.hip,
// classmetrics.hip):
// a plane of a dense [B, P, nx, ny] map, and the (count, fixed-point sum) cells of their int64 tables.  Included into
// each file's anonymous namespace, after wfs_evalbins.h (add64).
#pragma once
#include "wfs_common.h"

constexpr double FIX_ONE = 4294967296.0;     // 2^32, WFS_SEG_FIXED_ONE

struct Plane {                               // one [B, nx, ny] plane of a [B, P, nx, ny] tensor
    const void *base;
    long long batch_stride, offset;          // in elements; offset = plane * plane stride
    int dtype;
};
inline bool plane_ok(const void *base, int dtype, long long bs, long long ps, int plane) {
    return base && wfs_dtype_ok(dtype) && bs >= 0 && ps >= 0 && plane >= 0;
}

__device__ __forceinline__ float ld_plane(const Plane &m, long long e, int cell) {
    const long long i = e * m.batch_stride + m.offset + cell;
    if (m.dtype == WFS_F32) return wfs_ld((const float *)m.base + i);
    if (m.dtype == WFS_BF16) return wfs_ld((const wfs_bf16 *)m.base + i);
    return wfs_ld((const wfs_f16 *)m.base + i);
}

// the fixed-point image of a deviation, or false (flag 8): not finite, or 2^62 and above after scaling
__device__ __forceinline__ bool fixed_image(double dev, long long *out, int *flags) {
    const double s = __dmul_rn(dev, FIX_ONE);
    if (!(fabs(s) < 4611686018427387904.0)) {                 // 2^62; also catches NaN
        atomicOr(flags, 8);
        return false;
    }
    *out = __double2ll_rn(s);
    return true;
}
// the fixed-point image of a real-valued result (metricpairs.hip), or false (flag 8): not finite, or |r| >= 2^15 before
// scaling, so that the three limbs of v^2 hold
__device__ __forceinline__ bool real_image(float r, long long *v, int *flags) {
    if (!(fabsf(r) < 32768.f)) {              // also catches NaN
        atomicOr(flags, 8);
        return false;
    }
    *v = __double2ll_rn(__dmul_rn((double)r, FIX_ONE));
    return true;
}
// the same for a result held in fp64 (classmetrics.hip: a cross-entropy term), under the caller's flag bit
__device__ __forceinline__ bool real_image(double r, long long *v, int *flags, int bit) {
    if (!(fabs(r) < 32768.0)) {               // also catches NaN
        atomicOr(flags, bit);
        return false;
    }
    *v = __double2ll_rn(__dmul_rn(r, FIX_ONE));
    return true;
}
// a cell's sum; flag `bit` when it leaves int64 (the segment tables 8, the real-valued pair tables 16)
__device__ __forceinline__ void add_fixed(long long *p, long long v, int *flags, int bit) {
    const long long old = (long long)atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);
    const long long now = (long long)((unsigned long long)old + (unsigned long long)v);
    if (((old ^ now) & (v ^ now)) < 0) atomicOr(flags, bit);  // the cell's sum wrapped
}
// increment_metric_mult_SE's single / dual pair: tab = [count | sum] of one table of `cells` cells
__device__ __forceinline__ void add_cell(long long *tab, int cells, int cell, long long v, int *flags) {
    add64(tab + cell, 1);
    add_fixed(tab + cells + cell, v, flags, 8);
}
