// wfs_erroredges.h -- the histogram range the reference's ErrorAggregator.add_norm (src/utils/StatsUtils.py) fixes from
// the largest |error| of the first subset that reaches a class: low = -1.1 max, high = 1.1 max, and the FIRST and LAST
// entry of get_bins(low, high, nb) = np.arange(low, high + w / 2, w) with w = (high - low) / nb.  The last entry is not
// `high`: np.arange fills value[i] = low + i * delta with delta = (low + w) - low over L = ceil((high + w / 2 - low) / w)
// entries.  Every operation is one rounded fp64 operation (contraction is off in the function: no fma), on the host and on
// the device alike, so the two agree bit for bit with NumPy.
#pragma once

// false: max_abs is 0, negative or not finite (np.arange fails there too); nb >= 1
__host__ __device__ inline bool error_edge_range(double max_abs, int nb, double *first, double *last) {
#pragma clang fp contract(off)                // a fused multiply-add would round `low + (L - 1) * delta` once, NumPy twice
    if (!(max_abs > 0.0) || !(max_abs <= 1.7976931348623157e308) || nb < 1) return false;
    const double low = -1.1 * max_abs, high = 1.1 * max_abs;
    if (!(high <= 1.7976931348623157e308)) return false;
    const double w = (high - low) / (double)nb;
    if (!(w > 0.0)) return false;
    const double stop = high + w / 2.0;
    const double L = ceil((stop - low) / w);
    const double delta = (low + w) - low;
    const double span = (L - 1.0) * delta;
    *first = low;
    *last = low + span;
    return *last > *first;
}
