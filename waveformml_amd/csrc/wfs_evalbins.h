// wfs_evalbins.h -- the bin walks and the int64 add of the evaluation tables (evalstats.hip, segstats.hip, metricpairs.hip,
// segquant.hip, zreal.hip).  Included into each file's anonymous namespace.  Edges follow the reference literally: the first j with
// j * width + low > value, a rounded product and a rounded sum (no fma).
#pragma once
#include "wfs_common.h"

// get_bin_index / metric_accumulate_2d: underflow in bin 0, >= high in bin nbins + 1
__device__ __forceinline__ int bin_metric(double v, double low, double high, int nb) {
    const double w = (high - low) / nb;
    if (v < low) return 0;
    if (v >= high) return nb + 1;
    for (int j = 1; j <= nb; ++j)
        if (__dadd_rn(__dmul_rn((double)j, w), low) > v) return j;
    return 0;
}
// confusion_accumulate_1d: no underflow bin, and although it names bin nbins for values > high, its increment sits
// inside `if find_bin:` -- values below low AND above high are dropped (-1); a value exactly at high finds no edge above
// it and lands in bin 0, as in the reference
__device__ __forceinline__ int bin_confusion(double v, double low, double high, int nb) {
    const double w = (high - low) / nb;
    if (v < low || v > high) return -1;
    for (int j = 1; j <= nb; ++j)
        if (__dadd_rn(__dmul_rn((double)j, w), low) > v) return j - 1;
    return 0;
}
// get_bin_index(v, low, high, w, nb) without the walk: the candidate floor((v - low) / w) + 1 corrected by the
// reference's own predicate at the candidate and its neighbours.  The width is the caller's (zreal.hip:
// z_deviation_with_E_full_correlation bins [0, 1176) by zrange / nz = 12, which is not (high - low) / nb)
__device__ __forceinline__ int bin_direct_w(double v, double low, double high, double w, int nb) {
    if (v < low) return 0;
    if (v >= high) return nb + 1;
    if (!(v == v)) return 0;                  // NaN: no edge compares above it
    double c = floor((v - low) / w) + 1.0;
    c = c < 1.0 ? 1.0 : (c > (double)nb ? (double)nb : c);
    int k = (int)c;
    // edges are non-decreasing in j, so "j * w + low > v" is false up to some j and true from there on
    while (k > 1 && __dadd_rn(__dmul_rn((double)(k - 1), w), low) > v) --k;
    while (k <= nb && !(__dadd_rn(__dmul_rn((double)k, w), low) > v)) ++k;
    return k <= nb ? k : 0;                   // no edge above v: the reference's bin_index stays 0
}
// get_bin_index(v, low, high, (high - low) / nb, nb) (metricpairs.hip, segquant.hip, zreal.hip)
__device__ __forceinline__ int bin_direct(double v, double low, double high, int nb) {
    return bin_direct_w(v, low, high, (high - low) / nb, nb);
}

__device__ __forceinline__ void add64(long long *p, long long v) {
    atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);
}
