// physstats.hip -- the per-batch half of the reference's PhysEvaluator on the device.
//
// The reference's LitPSD hands every batch of a PulseDatasetDet run to PhysEvaluator.add (src/evaluation/PSDEvaluator.py:
// 319-397): seven extracted physics quantities per segment, averaged per event with the energy as weight
// (weighted_average_quantities, src/utils/SparseUtils.py:490-529), then binned.  Here the batch stays in HBM:
//
//   k_eval_offsets     (wfs_evoffsets.h) first row of every event from the sorted event column.
//   k_phys_events      ONE WAVEFRONT PER EVENT.  The reference's sums are sequential fp32 / fp64 sums in row order and that
//                      order is part of the result, so nothing is reduced across rows: lanes 0 .. 8 each own one
//                      accumulator (0 the fp64 energy, 1 .. 6 the fp32 weighted quantities, 7 and 8 the fp64 coordinate
//                      sums) and walk the event's rows front to back.  Every lane keeps its own copy of the running
//                      energy, so no lane waits for another; the loop body has no branch and its three loads do not
//                      depend on the sums, so the unrolled walk has the loads of four rows in flight together.  One lane per event would put 256 events on four waves and make
//                      every load a 28-byte-strided gather; one wave per event spreads them over the CUs and reads each
//                      row as one 28-byte piece.  The caller's rows are only read.
//   k_phys_accumulate  one thread per event into persistent int64 tables with integer atomics (exact, order-independent),
//                      and, where asked for, into the feature spectra.
//
// Every fp32 / fp64 product-then-sum of k_phys_events is two rounded operations as under numba (no fma).  What keeps it so
// is the pragma below and plain operators: hipcc's __fmul_rn / __fadd_rn and their fp64 kin are `x * y` and `x + y` in a
// header compiled with contraction allowed, so once inlined a product and the sum that takes it still fuse (seen in this
// file's device code); operators written under `contract(off)` carry no such permission.
#include "wfs_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int PB = 256;                      // 4 events per workgroup, one wave each
constexpr int PW = PB / WFS_WAVE;
constexpr int NQ = 7;                        // quantities per row
constexpr int NF = 8;                        // features per event: the seven averages and the multiplicity

#include "wfs_evoffsets.h"                   // k_eval_offsets
static_assert(PB == WFS_EVOFF_THREADS, "k_eval_offsets is launched with PB threads");
#include "wfs_evalbins.h"                   // bin_metric, bin_confusion, bin_direct, add64

// Stack entry j of PhysEvaluator.add:328-338 is (raw[col] - sub) * mul in fp32, as NumPy forms it; stack order (energy,
// psd, dt, PEL, PER, z, t0).  Where the code subtracts nothing or scales by nothing, sub = 0 and mul = 1 leave every bit.
struct Derived {
    int col;
    float sub, mul;
};
__device__ __forceinline__ Derived derived_of(int j) {
    switch (j) {
    case 1: return {5, 0.f, 1.f};
    case 2: return {1, 0.5f, 30.f};
    case 3: return {2, 0.f, 5000.f};
    case 4: return {3, 0.f, 5000.f};
    case 5: return {4, 0.5f, 1200.f};
    case 6: return {6, 0.f, 30.f};
    default: return {0, 0.f, 12.f};
    }
}

template <typename T>
__global__ void __launch_bounds__(PB)
k_phys_events(const int *__restrict__ coords, const T *__restrict__ rows, long long n_cap,
              const long long *__restrict__ n_dev, const int *__restrict__ off, int E, double *__restrict__ avg_coo,
              float *__restrict__ feat, int *__restrict__ mult) {
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * PW + (threadIdx.x >> 6);
    if (e >= E || lane > 8) return;
    const long long nv = wfs_valid_rows_nonneg(n_cap, n_dev);
    long long b = off[e], en = off[e + 1];
    b = b < 0 ? 0 : (b > nv ? nv : b);
    en = en < 0 ? 0 : (en > nv ? nv : en);
    if (en < b) en = b;                                        // only with a flagged (unsorted) event column
    // One loop body for all nine lanes, no branch in it: a quantity lane (1 .. 6) reads its column and x of the row, a
    // coordinate lane (7, 8) its coordinate and column 0; each adds to both of its accumulators and keeps the one it owns.
    const Derived d = derived_of(lane <= 6 ? lane : 0);
    const int cc = lane == 8 ? 1 : 0;
    double ene = 0.0, acc64 = 0.0;
    float acc32 = 0.f;
#pragma unroll 4
    for (long long r = b; r < en; ++r) {
        const float q0 = wfs_ld(rows + r * NQ) * 12.f;
        const float q = (wfs_ld(rows + r * NQ + d.col) - d.sub) * d.mul;
        const double xy = (double)coords[r * 3 + cc];
        ene = ene + (double)q0;
        const float w32 = q * q0;
        acc32 = acc32 + w32;
        // out_coords += coord[0:2] * ene_current: the RUNNING sum, not the row's energy (the reference's quirk)
        const double w64 = xy * ene;
        acc64 = acc64 + w64;
    }
    const bool pos = ene > 0.0;
    if (lane == 0) {
        feat[e] = pos ? (float)ene : 0.f;
        const int m = pos ? (int)(en - b) : 0;
        mult[e] = m;
        feat[(long long)NQ * E + e] = (float)m;
    } else if (lane <= 6) {
        // float32 /= float64 under numba: the quotient in fp64, stored to fp32
        feat[(long long)lane * E + e] = pos ? (float)((double)acc32 / ene) : acc32;
    } else {
        avg_coo[e * 2ll + (lane - 7)] = pos ? acc64 / ene : acc64;
    }
}

struct PhysBins {
    int n_bins, n_mult, n_conf, nx, ny, C;
    double emin, emax, pmin, pmax;
};
struct PhysSpectra {
    double lo[NF], hi[NF];
    int nb[NF];
    int per_class;                           // sum of nb + 2
};

__global__ void __launch_bounds__(PB)
k_phys_accumulate(int E, PhysBins B, const double *__restrict__ avg_coo, const float *__restrict__ feat,
                  const int *__restrict__ mult, const long long *__restrict__ pred, const long long *__restrict__ labels,
                  long long *__restrict__ tab, PhysSpectra S, long long *__restrict__ spectra, int *__restrict__ flags) {
    const int e = blockIdx.x * PB + threadIdx.x;
    if (e >= E) return;
    const int C = B.C;
    const long long p = pred[e], l = labels[e];
    if (p < 0 || p >= C || l < 0 || l >= C) {
        atomicOr(flags, 4);                                  // a class outside the evaluator's class_names
        return;
    }
    const long long hit = p == l ? 1 : 0;
    const long long nm = B.n_mult + 2, ne = B.n_bins + 2, px = B.nx + 2, py = B.ny + 2;
    const double en = (double)feat[e], psd = (double)feat[(long long)E + e], m = (double)mult[e];
    // table order: wfs_phys_table_ints
    long long *t = tab;
    const int km = bin_metric(m, 0.5, B.n_mult + 0.5, B.n_mult);
    add64(t + km, 1);
    add64(t + nm + km, hit);
    t += 2 * nm;
    const int bx = bin_metric(en, B.emin, B.emax, B.n_bins);
    const int by = bin_metric(psd, B.pmin, B.pmax, B.n_bins);
    add64(t + bx * ne + by, 1);
    add64(t + ne * ne + bx * ne + by, hit);
    t += 2 * ne * ne;
    const int qx = bin_metric(avg_coo[e * 2ll], 0.0, (double)B.nx, B.nx);
    const int qy = bin_metric(avg_coo[e * 2ll + 1], 0.0, (double)B.ny, B.ny);
    add64(t + qx * py + qy, 1);
    add64(t + px * py + qx * py + qy, hit);
    t += 2 * px * py;
    const int kc = bin_confusion(en, 0.0, B.emax, B.n_conf);
    if (kc >= 0) add64(t + ((long long)kc * C + l) * C + p, 1);
    t += (long long)(B.n_conf + 1) * C * C;
    // per TRUE class: ene_psd_prec, ene_prec, mult_prec
    t += l * 2 * ne * ne;
    add64(t + bx * ne + by, 1);
    add64(t + ne * ne + bx * ne + by, hit);
    t += (C - l) * 2 * ne * ne + l * 2 * ne;
    add64(t + bx, 1);
    add64(t + ne + bx, hit);
    t += (C - l) * 2 * ne + l * 2 * nm;
    add64(t + km, 1);
    add64(t + nm + km, hit);
    if (!spectra) return;
    // [by truth | by prediction][class][feature][nb + 2], hist_add_1d's bins
    long long *st = spectra + l * S.per_class, *sp = spectra + ((long long)C + p) * S.per_class;
    int at = 0;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        const double v = f == NF - 1 ? m : (double)feat[(long long)f * E + e];
        const int k = bin_direct(v, S.lo[f], S.hi[f], S.nb[f]);
        add64(st + at + k, 1);
        add64(sp + at + k, 1);
        at += S.nb[f] + 2;
    }
}

}  // namespace

extern "C" size_t wfs_phys_table_ints(int32_t n_bins, int32_t n_mult, int32_t n_confusion, int32_t nx, int32_t ny,
                                      int32_t n_classes) {
    const size_t C = (size_t)n_classes, ne = (size_t)n_bins + 2, nm = (size_t)n_mult + 2;
    return 2 * nm + 2 * ne * ne + 2 * ((size_t)nx + 2) * ((size_t)ny + 2) + ((size_t)n_confusion + 1) * C * C +
           C * (2 * ne * ne + 2 * ne + 2 * nm);
}

extern "C" size_t wfs_phys_spectra_ints(int32_t n_classes, const int32_t *spec_bins) {
    size_t per = 0;
    for (int f = 0; f < NF; ++f) per += (size_t)(spec_bins[f] > 0 ? spec_bins[f] : 0) + 2;
    return 2 * (size_t)n_classes * per;
}

extern "C" int wfs_phys_event_stats(const int32_t *coords, const void *rows, int64_t n_cap, int32_t dtype,
                                    const int64_t *n_dev, int32_t E, int32_t *offsets, double *avg_coo, float *features,
                                    int32_t *multiplicity, int32_t *flags, void *stream) {
    WFS_REQUIRE(wfs_dtype_ok(dtype), WFS_EINVAL, "wfs_phys_event_stats: unknown dtype %d", dtype);
    WFS_REQUIRE_EVAL_BATCH("wfs_phys_event_stats: E", E, n_cap, 1, 1);
    WFS_REQUIRE(coords && rows && offsets && avg_coo && features && multiplicity && flags, WFS_EINVAL,
                "wfs_phys_event_stats: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    const int rc = launch_eval_offsets(coords, n_cap, (const long long *)n_dev, E, offsets, flags, s);
    if (rc != WFS_OK) return rc;
    return wfs_with_dtype(dtype, [&](auto t) -> int {
        using TYPE = decltype(t);
        k_phys_events<TYPE><<<(unsigned)wfs_cdiv(E, PW), PB, 0, s>>>(coords, (const TYPE *)rows, n_cap,
                                                                      (const long long *)n_dev, offsets, E, avg_coo,
                                                                      features, multiplicity);
        WFS_LAUNCH_CHECK();
        return WFS_OK;
    });
}

extern "C" int wfs_phys_accumulate(int32_t E, int32_t n_classes, const double *avg_coo, const float *features,
                                   const int32_t *multiplicity, const int64_t *predictions, const int64_t *labels,
                                   int32_t n_bins, int32_t n_mult, int32_t n_confusion, int32_t nx, int32_t ny,
                                   double emin, double emax, double psd_min, double psd_max, int64_t *tables,
                                   const double *spec_ranges, const int32_t *spec_bins, int64_t *spectra, int32_t *flags,
                                   void *stream) {
    WFS_REQUIRE(E >= 1 && n_classes >= 1, WFS_EINVAL, "wfs_phys_accumulate: E = %d, classes = %d", E, n_classes);
    WFS_REQUIRE(n_bins >= 1 && n_mult >= 1 && n_confusion >= 1 && nx >= 1 && ny >= 1, WFS_EINVAL,
                "wfs_phys_accumulate: bad bin counts");
    WFS_REQUIRE(avg_coo && features && multiplicity && predictions && labels && tables && flags, WFS_EINVAL,
                "wfs_phys_accumulate: NULL argument");
    WFS_REQUIRE(!spectra || (spec_ranges && spec_bins), WFS_EINVAL, "wfs_phys_accumulate: spectra without their ranges");
    PhysBins B = {n_bins, n_mult, n_confusion, nx, ny, n_classes, emin, emax, psd_min, psd_max};
    PhysSpectra S = {};
    if (spectra)
        for (int f = 0; f < NF; ++f) {
            WFS_REQUIRE(spec_bins[f] >= 1 && spec_ranges[2 * f + 1] > spec_ranges[2 * f], WFS_EINVAL,
                        "wfs_phys_accumulate: spectrum %d has %d bins over [%g, %g]", f, spec_bins[f], spec_ranges[2 * f],
                        spec_ranges[2 * f + 1]);
            S.lo[f] = spec_ranges[2 * f], S.hi[f] = spec_ranges[2 * f + 1], S.nb[f] = spec_bins[f];
            S.per_class += spec_bins[f] + 2;
        }
    k_phys_accumulate<<<(unsigned)wfs_cdiv(E, PB), PB, 0, (hipStream_t)stream>>>(
        E, B, avg_coo, features, multiplicity, (const long long *)predictions, (const long long *)labels,
        (long long *)tables, S, (long long *)spectra, flags);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}
