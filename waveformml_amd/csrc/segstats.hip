// segstats.hip -- the per-batch half of the reference's per-segment evaluators on the device: ZEvaluatorWF.add and
// EnergyEvaluatorWF.add without a calibration group (src/evaluation/ZEvaluator.py:528-562, EnergyEvaluator.py:132-145),
// i.e. the row walks z_deviation / z_deviation_with_E / z_error / E_deviation of src/utils/SparseUtils.py:1190-1455.
//
//   k_eval_offsets   (wfs_evoffsets.h, shared with evalstats.hip) first row of every event; a row's multiplicity is the
//                    length of its event's run, which the reference finds by looking ahead.
//   k_seg_z          one thread per row: |p - t| into seg_mult_mae, z_mult_mae_single/dual (and E_mult_mae_* when an
//                    energy map is given), (p - t) * zrange into the sample segments' error histograms.
//   k_seg_energy     one thread per row: |p - t| / t into seg_mult_Emape and E_mult_single/dual.
//
// Bin arithmetic is fp64 on the fp32 value of the element, a rounded product then a rounded sum (no fma), the
// reference's literal edge walks (evalstats.hip has the same rule).  Counts are integer atomics on int64 cells.
// Deviation sums are integer atomics too, on the deviation's fixed-point image round(dev * 2^32) in an int64 cell:
// exact integer sums, hence independent of the order the rows arrive in and bit-identical from run to run, without a
// float atomic.  A deviation that has no image (not finite, |dev| >= 2^30) or a cell whose sum leaves int64 sets flag
// bit 8 and is left out.  The caller's tensors are only read; every index is checked before it is used.
#include "wfs_common.h"

namespace {

#include "wfs_evoffsets.h"
#include "wfs_segrows.h"
#include "wfs_evalbins.h"
#include "wfs_segtables.h"

constexpr int SB = WFS_EVOFF_THREADS;
// z_deviation's own walk: the first k with k * (zrange / nz) - zrange / 2 > true_z
__device__ __forceinline__ int bin_z(double z, double zrange, int nz) {
    const double half = zrange / 2., w = zrange / nz;
    if (z < -half) return 0;
    if (z >= half) return nz + 1;
    for (int k = 1; k <= nz; ++k)
        if (__dsub_rn(__dmul_rn((double)k, w), half) > z) return k;
    return 0;
}
// the multiplicity column of a row: the length of its event's run, beyond nmult (and a run of 0) in the last column
__device__ __forceinline__ int mult_col(const SegRow &h, int nmult) {
    const int mult = (int)(h.last - h.first);
    return 0 < mult && mult <= nmult ? mult - 1 : nmult;
}

struct ZBins {
    int nx, ny, nmult, nz, n_err, n_sample;
    double zrange, err_low, err_high, E_low, E_high, E_scale;
};

// z_deviation_with_E (z_deviation when has_E is false) and z_error of one row into one table set (wfs_seg_z_table_ints)
__device__ __forceinline__ void seg_z_row(const SegRow &h, double p, double t, bool has_E, double E, bool single,
                                          const int *__restrict__ sample_segs, const ZBins &Z, long long *tab, int *flags) {
    const int cell = h.cell, col = mult_col(h, Z.nmult), nm1 = Z.nmult + 1;
    const int seg_cells = Z.nx * Z.ny * nm1, bin_cells = (Z.nz + 2) * nm1;
    long long *t_seg = tab, *t_zs = t_seg + 2 * seg_cells, *t_zd = t_zs + 2 * bin_cells, *t_es = t_zd + 2 * bin_cells,
              *t_ed = t_es + 2 * bin_cells, *t_hist = t_ed + 2 * bin_cells;
    long long v;
    if (fixed_image(fabs(__dsub_rn(p, t)), &v, flags)) {
        const int zb = bin_z(__dmul_rn(__dsub_rn(t, 0.5), Z.zrange), Z.zrange, Z.nz);
        add_cell(t_seg, seg_cells, cell * nm1 + col, v, flags);
        add_cell(single ? t_zs : t_zd, bin_cells, zb * nm1 + col, v, flags);
        if (has_E) {
            const int eb = bin_metric(E, Z.E_low, Z.E_high, Z.nz);
            add_cell(single ? t_es : t_ed, bin_cells, eb * nm1 + col, v, flags);
        }
    }
    // z_error: only rows on a sample segment (the first that matches, as sample_index)
    for (int s = 0; s < Z.n_sample; ++s)
        if (sample_segs[2 * s] == h.x && sample_segs[2 * s + 1] == h.y) {
            const double err = __dmul_rn(__dsub_rn(p, t), Z.zrange);
            // NaN compares false everywhere: the reference's walk leaves it in bin 0, and so does this one
            const int b = bin_metric(err, Z.err_low, Z.err_high, Z.n_err);
            add64(t_hist + ((long long)s * nm1 + col) * (Z.n_err + 2) + b, 1);
            break;
        }
}

__global__ void __launch_bounds__(SB)
k_seg_z(const int *__restrict__ coords, long long n_cap, const long long *__restrict__ n_dev, int B, Plane pred,
        Plane targ, Plane ene, const float *__restrict__ seg, const int *__restrict__ sample_segs, ZBins Z,
        const int *__restrict__ off, long long *__restrict__ tab, int *__restrict__ flags) {
    const long long nv = wfs_valid_rows_nonneg(n_cap, n_dev);
    const long long r = (long long)blockIdx.x * SB + threadIdx.x;
    if (r >= nv) return;
    const SegRow h = seg_row(coords, r, nv, off, B, Z.nx, Z.ny, flags);
    if (!h.ok) return;
    const double p = (double)ld_plane(pred, h.e, h.cell), t = (double)ld_plane(targ, h.e, h.cell);
    // the reference scales the energy map on the host, float32 * E_scale in float32, before the walk sees it
    const double E = ene.base ? (double)__fmul_rn(ld_plane(ene, h.e, h.cell), (float)Z.E_scale) : 0.0;
    seg_z_row(h, p, t, ene.base != nullptr, E, seg[h.cell] > 0.f, sample_segs, Z, tab, flags);
}

// ZEvaluatorWF.add with a calibrator: the prediction into the first table set, the calibrated z into the second
// (z_from_cal), both through z_deviation_with_E on the same energy axis: the true energy map when there is one, else the
// calibrated E, unscaled.  A row whose reconstruction is not finite (wfs_calib_z_E, flag 16) is left out of both.
__global__ void __launch_bounds__(SB)
k_seg_z_cal(const int *__restrict__ coords, long long n_cap, const long long *__restrict__ n_dev, int B, Plane pred,
            Plane targ, Plane ene, const double *__restrict__ z_cal, const double *__restrict__ E_cal,
            const float *__restrict__ base, const float *__restrict__ seg, const int *__restrict__ sample_segs, ZBins Z,
            const int *__restrict__ off, long long *__restrict__ tab, long long set_ints, int *__restrict__ flags) {
    const long long nv = wfs_valid_rows_nonneg(n_cap, n_dev);
    const long long r = (long long)blockIdx.x * SB + threadIdx.x;
    if (r >= nv) return;
    const SegRow h = seg_row(coords, r, nv, off, B, Z.nx, Z.ny, flags);
    if (!h.ok) return;
    const double zc = z_cal[r], Ec = E_cal[r];
    if (!(fabs(zc) <= 1.7976931348623157e308) || !(fabs(Ec) <= 1.7976931348623157e308)) return;
    const double p = (double)ld_plane(pred, h.e, h.cell), t = (double)ld_plane(targ, h.e, h.cell);
    const double E = ene.base ? (double)__fmul_rn(ld_plane(ene, h.e, h.cell), (float)Z.E_scale) : Ec;
    const bool single = seg[h.cell] > 0.f;
    seg_z_row(h, p, t, true, E, single, sample_segs, Z, tab, flags);
    // target_is_cal: the baseline walk's float32 row in place of the calibrated z
    seg_z_row(h, base ? (double)base[r] : zc, t, true, E, single, sample_segs, Z, tab + set_ints, flags);
}

// the target plane as float32 rows, what wfs_zreal_baseline walks; 0 on rows that raise a flag and beyond the valid count
__global__ void __launch_bounds__(SB)
k_seg_target_rows(const int *__restrict__ coords, long long n_cap, const long long *__restrict__ n_dev, int B, Plane targ,
                  int nx, int ny, float *__restrict__ rows) {
    const long long nv = wfs_valid_rows_nonneg(n_cap, n_dev);
    const long long r = (long long)blockIdx.x * SB + threadIdx.x;
    if (r >= n_cap) return;
    float v = 0.f;
    if (r < nv) {
        const int x = coords[r * 3], y = coords[r * 3 + 1], e = coords[r * 3 + 2];
        if (e >= 0 && e < B && x >= 0 && x < nx && y >= 0 && y < ny) v = ld_plane(targ, e, x * ny + y);
    }
    rows[r] = v;
}

struct EBins {
    int nx, ny, nmult, nE;
    double E_low, E_high, E_scale;
};

__global__ void __launch_bounds__(SB)
k_seg_energy(const int *__restrict__ coords, long long n_cap, const long long *__restrict__ n_dev, int B, Plane pred,
             Plane targ, const float *__restrict__ seg, EBins Eb, const int *__restrict__ off,
             long long *__restrict__ tab, int *__restrict__ flags) {
    const long long nv = wfs_valid_rows_nonneg(n_cap, n_dev);
    const long long r = (long long)blockIdx.x * SB + threadIdx.x;
    if (r >= nv) return;
    const SegRow h = seg_row(coords, r, nv, off, B, Eb.nx, Eb.ny, flags);
    if (!h.ok) return;
    const int cell = h.cell, col = mult_col(h, Eb.nmult), nm1 = Eb.nmult + 1;
    const double p = (double)ld_plane(pred, h.e, cell), t = (double)ld_plane(targ, h.e, cell);
    if (t == 0.0) {
        atomicOr(flags, 4);                  // the reference divides by it (numba raises, plain Python gives inf)
        return;
    }
    long long v;
    if (!fixed_image(fabs(__dsub_rn(p, t)) / t, &v, flags)) return;
    const int eb = bin_metric(__dmul_rn(t, Eb.E_scale), Eb.E_low, Eb.E_high, Eb.nE);
    // table order: wfs_seg_energy_table_ints
    const int seg_cells = Eb.nx * Eb.ny * nm1, bin_cells = (Eb.nE + 2) * nm1;
    long long *t_seg = tab, *t_es = t_seg + 2 * seg_cells, *t_ed = t_es + 2 * bin_cells;
    add_cell(t_seg, seg_cells, cell * nm1 + col, v, flags);
    add_cell(seg[cell] > 0.f ? t_es : t_ed, bin_cells, eb * nm1 + col, v, flags);
}

// EnergyEvaluatorWF.add with a calibrator (calc_deviation_with_z): E_deviation_with_z of the prediction into the first
// table set and of the calibrated E into the second, both binned by the calibrated z.  The calibrated maps are float32
// there (WaveformEvaluator.z_E_from_cal), so both values are rounded to it first.
struct EzBins {
    int nx, ny, nmult, nE, nz;
    double E_low, E_high, E_scale, zrange;
};

__device__ __forceinline__ void seg_energy_z_row(const SegRow &h, double p, double t, int eb, int zb, bool single,
                                                 const EzBins &Eb, long long *tab, int *flags) {
    long long v;
    if (!fixed_image(fabs(__dsub_rn(p, t)) / t, &v, flags)) return;
    const int col = mult_col(h, Eb.nmult), nm1 = Eb.nmult + 1;
    const int seg_cells = Eb.nx * Eb.ny * nm1, bin_cells = (Eb.nE + 2) * nm1, ez_cells = (Eb.nE + 2) * (Eb.nz + 2);
    long long *t_seg = tab, *t_es = t_seg + 2 * seg_cells, *t_ed = t_es + 2 * bin_cells, *t_zs = t_ed + 2 * bin_cells,
              *t_zd = t_zs + 2 * ez_cells;
    add_cell(t_seg, seg_cells, h.cell * nm1 + col, v, flags);
    add_cell(single ? t_es : t_ed, bin_cells, eb * nm1 + col, v, flags);
    add_cell(single ? t_zs : t_zd, ez_cells, eb * (Eb.nz + 2) + zb, v, flags);
}

__global__ void __launch_bounds__(SB)
k_seg_energy_cal(const int *__restrict__ coords, long long n_cap, const long long *__restrict__ n_dev, int B, Plane pred,
                 Plane targ, const double *__restrict__ z_cal, const double *__restrict__ E_cal,
                 const float *__restrict__ seg, EzBins Eb, const int *__restrict__ off, long long *__restrict__ tab,
                 long long set_ints, int *__restrict__ flags) {
    const long long nv = wfs_valid_rows_nonneg(n_cap, n_dev);
    const long long r = (long long)blockIdx.x * SB + threadIdx.x;
    if (r >= nv) return;
    const SegRow h = seg_row(coords, r, nv, off, B, Eb.nx, Eb.ny, flags);
    if (!h.ok) return;
    const double zc = z_cal[r], Ec = E_cal[r];
    if (!(fabs(zc) <= 1.7976931348623157e308) || !(fabs(Ec) <= 1.7976931348623157e308)) return;
    const double p = (double)ld_plane(pred, h.e, h.cell), t = (double)ld_plane(targ, h.e, h.cell);
    if (t == 0.0) {
        atomicOr(flags, 4);
        return;
    }
    const int eb = bin_metric(__dmul_rn(t, Eb.E_scale), Eb.E_low, Eb.E_high, Eb.nE);
    const double half = Eb.zrange / 2.;
    const int zb = bin_direct_w(__dmul_rn(__dsub_rn((double)(float)zc, 0.5), Eb.zrange), -half, half, Eb.zrange / Eb.nE,
                                Eb.nE);
    const bool single = seg[h.cell] > 0.f;
    seg_energy_z_row(h, p, t, eb, zb, single, Eb, tab, flags);
    seg_energy_z_row(h, (double)(float)Ec, t, eb, zb, single, Eb, tab + set_ints, flags);
}

}  // namespace

extern "C" size_t wfs_seg_z_table_ints(int32_t nx, int32_t ny, int32_t nmult, int32_t nz, int32_t n_err,
                                       int32_t n_sample) {
    const size_t nm1 = (size_t)nmult + 1;
    return 2 * (size_t)nx * ny * nm1 + 8 * ((size_t)nz + 2) * nm1 + (size_t)n_sample * nm1 * ((size_t)n_err + 2);
}

extern "C" size_t wfs_seg_energy_table_ints(int32_t nx, int32_t ny, int32_t nmult, int32_t nE) {
    const size_t nm1 = (size_t)nmult + 1;
    return 2 * (size_t)nx * ny * nm1 + 4 * ((size_t)nE + 2) * nm1;
}

extern "C" int wfs_seg_z_accumulate(const int32_t *coords, int64_t n_cap, const int64_t *n_dev, int32_t B,
                                    const void *pred, int32_t pred_dtype, int64_t pred_bs, int64_t pred_ps,
                                    int32_t pred_plane, const void *targ, int32_t targ_dtype, int64_t targ_bs,
                                    int64_t targ_ps, int32_t targ_plane, const void *energy, int32_t e_dtype,
                                    int64_t e_bs, int64_t e_ps, int32_t e_plane, const float *seg_status, int32_t nx,
                                    int32_t ny, const int32_t *sample_segs, int32_t n_sample, int32_t nmult, int32_t nz,
                                    double zrange, int32_t n_err, double err_low, double err_high, double E_low,
                                    double E_high, double E_scale, int32_t *offsets, int64_t *tables, int32_t *flags,
                                    void *stream) {
    WFS_REQUIRE_EVAL_BATCH("wfs_seg_z_accumulate: B", B, n_cap, nx, ny);
    WFS_REQUIRE(nmult >= 1 && nz >= 1 && n_err >= 1 && n_sample >= 0 && err_high > err_low && zrange > 0, WFS_EINVAL,
                "wfs_seg_z_accumulate: bad bin parameters");
    WFS_REQUIRE(coords && seg_status && (sample_segs || n_sample == 0) && offsets && tables && flags, WFS_EINVAL,
                "wfs_seg_z_accumulate: NULL argument");
    WFS_REQUIRE(plane_ok(pred, pred_dtype, pred_bs, pred_ps, pred_plane) &&
                    plane_ok(targ, targ_dtype, targ_bs, targ_ps, targ_plane) &&
                    (!energy || (plane_ok(energy, e_dtype, e_bs, e_ps, e_plane) && E_high > E_low)),
                WFS_EINVAL, "wfs_seg_z_accumulate: bad map (NULL, unknown dtype or negative stride / plane)");
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = launch_eval_offsets(coords, n_cap, (const long long *)n_dev, B, offsets, flags, s)) return rc;
    if (n_cap == 0) return WFS_OK;
    const unsigned rb = (unsigned)wfs_cdiv(n_cap, SB);
    const Plane P = {pred, pred_bs, pred_ps * pred_plane, pred_dtype};
    const Plane T = {targ, targ_bs, targ_ps * targ_plane, targ_dtype};
    const Plane En = {energy, e_bs, energy ? e_ps * e_plane : 0, energy ? e_dtype : WFS_F32};
    const ZBins Z = {nx, ny, nmult, nz, n_err, n_sample, zrange, err_low, err_high, E_low, E_high, E_scale};
    k_seg_z<<<rb, SB, 0, s>>>(coords, n_cap, (const long long *)n_dev, B, P, T, En, seg_status, sample_segs, Z, offsets,
                              (long long *)tables, flags);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}

extern "C" int wfs_seg_energy_accumulate(const int32_t *coords, int64_t n_cap, const int64_t *n_dev, int32_t B,
                                         const void *pred, int32_t pred_dtype, int64_t pred_bs, int64_t pred_ps,
                                         int32_t pred_plane, const void *targ, int32_t targ_dtype, int64_t targ_bs,
                                         int64_t targ_ps, int32_t targ_plane, const float *seg_status, int32_t nx,
                                         int32_t ny, int32_t nmult, int32_t nE, double E_low, double E_high,
                                         double E_scale, int32_t *offsets, int64_t *tables, int32_t *flags,
                                         void *stream) {
    WFS_REQUIRE_EVAL_BATCH("wfs_seg_energy_accumulate: B", B, n_cap, nx, ny);
    WFS_REQUIRE(nmult >= 1 && nE >= 1 && E_high > E_low, WFS_EINVAL, "wfs_seg_energy_accumulate: bad bin parameters");
    WFS_REQUIRE(coords && seg_status && offsets && tables && flags, WFS_EINVAL,
                "wfs_seg_energy_accumulate: NULL argument");
    WFS_REQUIRE(plane_ok(pred, pred_dtype, pred_bs, pred_ps, pred_plane) &&
                    plane_ok(targ, targ_dtype, targ_bs, targ_ps, targ_plane),
                WFS_EINVAL, "wfs_seg_energy_accumulate: bad map (NULL, unknown dtype or negative stride / plane)");
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = launch_eval_offsets(coords, n_cap, (const long long *)n_dev, B, offsets, flags, s)) return rc;
    if (n_cap == 0) return WFS_OK;
    const unsigned rb = (unsigned)wfs_cdiv(n_cap, SB);
    const Plane P = {pred, pred_bs, pred_ps * pred_plane, pred_dtype};
    const Plane T = {targ, targ_bs, targ_ps * targ_plane, targ_dtype};
    const EBins Eb = {nx, ny, nmult, nE, E_low, E_high, E_scale};
    k_seg_energy<<<rb, SB, 0, s>>>(coords, n_cap, (const long long *)n_dev, B, P, T, seg_status, Eb, offsets,
                                   (long long *)tables, flags);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}

extern "C" int wfs_seg_z_accumulate_cal(const int32_t *coords, int64_t n_cap, const int64_t *n_dev, int32_t B,
                                        const void *pred, int32_t pred_dtype, int64_t pred_bs, int64_t pred_ps,
                                        int32_t pred_plane, const void *targ, int32_t targ_dtype, int64_t targ_bs,
                                        int64_t targ_ps, int32_t targ_plane, const void *energy, int32_t e_dtype,
                                        int64_t e_bs, int64_t e_ps, int32_t e_plane, const double *z_cal,
                                        const double *E_cal, int32_t target_is_cal, float *row_scratch,
                                        const float *seg_status, int32_t nx, int32_t ny, const int32_t *sample_segs,
                                        int32_t n_sample, int32_t nmult, int32_t nz, double zrange, int32_t n_err,
                                        double err_low, double err_high, double E_low, double E_high, double E_scale,
                                        int32_t *offsets, int64_t *tables, int32_t *flags, void *stream) {
    WFS_REQUIRE_EVAL_BATCH("wfs_seg_z_accumulate_cal: B", B, n_cap, nx, ny);
    WFS_REQUIRE(nmult >= 1 && nz >= 1 && n_err >= 1 && n_sample >= 0 && err_high > err_low && zrange > 0 && E_high > E_low,
                WFS_EINVAL, "wfs_seg_z_accumulate_cal: bad bin parameters");
    WFS_REQUIRE(coords && seg_status && (sample_segs || n_sample == 0) && offsets && tables && flags &&
                    (n_cap == 0 || (z_cal && E_cal && (row_scratch || !target_is_cal))),
                WFS_EINVAL, "wfs_seg_z_accumulate_cal: NULL argument");
    WFS_REQUIRE(plane_ok(pred, pred_dtype, pred_bs, pred_ps, pred_plane) &&
                    plane_ok(targ, targ_dtype, targ_bs, targ_ps, targ_plane) &&
                    (!energy || plane_ok(energy, e_dtype, e_bs, e_ps, e_plane)),
                WFS_EINVAL, "wfs_seg_z_accumulate_cal: bad map (NULL, unknown dtype or negative stride / plane)");
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = launch_eval_offsets(coords, n_cap, (const long long *)n_dev, B, offsets, flags, s)) return rc;
    if (n_cap == 0) return WFS_OK;
    const Plane P = {pred, pred_bs, pred_ps * pred_plane, pred_dtype};
    const Plane T = {targ, targ_bs, targ_ps * targ_plane, targ_dtype};
    const Plane En = {energy, e_bs, energy ? e_ps * e_plane : 0, energy ? e_dtype : WFS_F32};
    const ZBins Z = {nx, ny, nmult, nz, n_err, n_sample, zrange, err_low, err_high, E_low, E_high, E_scale};
    float *base = nullptr;
    if (target_is_cal) {
        // z_from_cal(target_is_cal=True): 0.5 on single-ended segments, the target elsewhere, then
        // z_basic_prediction_dense(truth_is_cal=True) -- the walk of wfs_zreal_baseline on the target's rows
        base = row_scratch + n_cap;
        k_seg_target_rows<<<(unsigned)wfs_cdiv(n_cap, SB), SB, 0, s>>>(coords, n_cap, (const long long *)n_dev, B, T, nx,
                                                                       ny, row_scratch);
        WFS_LAUNCH_CHECK();
        if (const int rc = wfs_zreal_baseline(coords, n_cap, n_dev, B, offsets, row_scratch, seg_status, nx, ny, base,
                                              stream))
            return rc;
    }
    k_seg_z_cal<<<(unsigned)wfs_cdiv(n_cap, SB), SB, 0, s>>>(
        coords, n_cap, (const long long *)n_dev, B, P, T, En, z_cal, E_cal, base, seg_status, sample_segs, Z, offsets,
        (long long *)tables, (long long)wfs_seg_z_table_ints(nx, ny, nmult, nz, n_err, n_sample), flags);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}

extern "C" size_t wfs_seg_energy_cal_table_ints(int32_t nx, int32_t ny, int32_t nmult, int32_t nE, int32_t nz) {
    return 2 * (wfs_seg_energy_table_ints(nx, ny, nmult, nE) + 4 * ((size_t)nE + 2) * ((size_t)nz + 2));
}

extern "C" int wfs_seg_energy_accumulate_cal(const int32_t *coords, int64_t n_cap, const int64_t *n_dev, int32_t B,
                                             const void *pred, int32_t pred_dtype, int64_t pred_bs, int64_t pred_ps,
                                             int32_t pred_plane, const void *targ, int32_t targ_dtype, int64_t targ_bs,
                                             int64_t targ_ps, int32_t targ_plane, const double *z_cal,
                                             const double *E_cal, const float *seg_status, int32_t nx, int32_t ny,
                                             int32_t nmult, int32_t nE, int32_t nz, double E_low, double E_high,
                                             double E_scale, double zrange, int32_t *offsets, int64_t *tables,
                                             int32_t *flags, void *stream) {
    WFS_REQUIRE_EVAL_BATCH("wfs_seg_energy_accumulate_cal: B", B, n_cap, nx, ny);
    WFS_REQUIRE(nmult >= 1 && nE >= 1 && nz >= nE && E_high > E_low && zrange > 0, WFS_EINVAL,
                "wfs_seg_energy_accumulate_cal: bad bin parameters (nz >= nE: the z bins are nE wide bins)");
    WFS_REQUIRE(coords && seg_status && offsets && tables && flags && (n_cap == 0 || (z_cal && E_cal)), WFS_EINVAL,
                "wfs_seg_energy_accumulate_cal: NULL argument");
    WFS_REQUIRE(plane_ok(pred, pred_dtype, pred_bs, pred_ps, pred_plane) &&
                    plane_ok(targ, targ_dtype, targ_bs, targ_ps, targ_plane),
                WFS_EINVAL, "wfs_seg_energy_accumulate_cal: bad map (NULL, unknown dtype or negative stride / plane)");
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = launch_eval_offsets(coords, n_cap, (const long long *)n_dev, B, offsets, flags, s)) return rc;
    if (n_cap == 0) return WFS_OK;
    const Plane P = {pred, pred_bs, pred_ps * pred_plane, pred_dtype};
    const Plane T = {targ, targ_bs, targ_ps * targ_plane, targ_dtype};
    const EzBins Eb = {nx, ny, nmult, nE, nz, E_low, E_high, E_scale, zrange};
    k_seg_energy_cal<<<(unsigned)wfs_cdiv(n_cap, SB), SB, 0, s>>>(
        coords, n_cap, (const long long *)n_dev, B, P, T, z_cal, E_cal, seg_status, Eb, offsets, (long long *)tables,
        (long long)(wfs_seg_energy_cal_table_ints(nx, ny, nmult, nE, nz) / 2), flags);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}
