// zreal.hip -- the reference's real-data z evaluator (src/evaluation/ZEvaluator.py ZEvaluatorRealWFNorm.add, with
// WaveformEvaluator.analyze_wf_z and RealDataEvaluator.add) on the device: the row walks align_wfs / find_peak /
// calc_crossing (src/utils/WaveformUtils.py), z_basic_prediction_dense and z_deviation_with_E_full_correlation
// (src/utils/SparseUtils.py).
//
//   k_align_pulses   one WAVEFRONT per row, both PMT sides in turn.  The side's L samples are staged once into LDS with
//                    unit-stride lanes (a row is 2 L contiguous elements), then per 64-sample chunk two ballots give the
//                    masks of rising and of non-flat steps.  A falling step at i closes a candidate exactly when the
//                    last non-flat step before it was a rise at j (find_peak's local_maxpos): one masked count of
//                    leading zeros finds j, the candidate is (j + i - 1) / 2.  find_peak's sequential "strictly above the
//                    running best" is the FIRST candidate that holds the largest candidate value, if that value lies above
//                    v[0], else index 0: a butterfly reduction over (value, index).  calc_crossing(-0.5) walks down from
//                    the peak to the first sample below half height: the LARGEST s in [1, peak] with v[s] < thresh, a
//                    max reduction; the interpolation and start = rint(peak + tx) - 1 are fp64 on the stored values,
//                    computed by every lane alike.  Samples before the row (start = -1) and beyond it are 0.
//   k_zreal_rows     one thread per row after the event offsets (wfs_evoffsets.h): the row's prediction, true z and
//                    energy out of the dense maps, |pred - z| (0 where the target is exactly 0), |z - z_pred| in mm, the
//                    mapped PID class, the single-ended flag, the z slice of analyze_wf_z, the categories of the class
//                    tables and of the sample tables, and the [4, N] parameters E / PSD / multiplicity / z, where the
//                    multiplicity is the number of SINGLE-ENDED rows of the event (RealDataEvaluator.add walks
//                    coo[SE_inds]).
//   k_zreal_baseline one lane per event walking its rows in order: z_basic_prediction_dense(truth_is_cal=True) on the
//                    map that is 0.5 on single-ended segments and the true z elsewhere.  The walk updates in place, so an
//                    averaged row feeds later rows of its event; the look-behind stops in front of row 0 of the batch.
//                    The average is an fp64 sum in the reference's order (ahead, then behind), stored once to fp32.
//   k_zreal_acc      one thread per row: z_deviation_with_E_full_correlation into seven (count, fixed-point sum) tables
//                    (wfs_segtables.h).  Integer atomics only.
#include "wfs_common.h"

namespace {

#include "wfs_evoffsets.h"
#include "wfs_segrows.h"
#include "wfs_evalbins.h"
#include "wfs_segtables.h"

constexpr int ZB = WFS_EVOFF_THREADS;
constexpr int AL_WAVES = 4, AL_THREADS = AL_WAVES * WFS_WAVE;
constexpr int AL_MAX_L = 512, AL_MAX_CHUNKS = AL_MAX_L / WFS_WAVE, AL_MAX_P = 16;
constexpr int ZR_SLICES = 12;                 // analyze_wf_z: NUM_Z_BINS + 2
constexpr double ZR_HALF_CELL = 588.;         // z_deviation_with_E_full_correlation's half_cell_length

template <typename T>
__global__ void __launch_bounds__(AL_THREADS)
k_align_pulses(const T *__restrict__ feats, long long n_cap, const long long *__restrict__ n_dev, int L, int P,
               float *__restrict__ out, int *__restrict__ start_out) {
    __shared__ float sv[AL_WAVES][AL_MAX_L];
    __shared__ unsigned long long s_nf[AL_WAVES][AL_MAX_CHUNKS], s_rise[AL_WAVES][AL_MAX_CHUNKS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long nv = wfs_valid_rows_nonneg(n_cap, n_dev);
    const long long r = (long long)blockIdx.x * AL_WAVES + wave;
    const bool in_cap = r < n_cap, live = r < nv;                       // wave-uniform
    const int chunks = (L + WFS_WAVE - 1) / WFS_WAVE;
    float *v = sv[wave];
    for (int side = 0; side < 2; ++side) {
        if (live) {
            const T *row = feats + r * 2 * L + (long long)side * L;
            for (int i = lane; i < L; i += WFS_WAVE) v[i] = wfs_ld(row + i);
        }
        __syncthreads();
        if (live)
            for (int c = 0; c < chunks; ++c) {
                const int i = c * WFS_WAVE + lane;
                const bool in = i >= 1 && i < L;
                const float a = in ? v[i - 1] : 0.f, b = in ? v[i] : 0.f;
                const unsigned long long rs = __ballot(in && b > a), nf = __ballot(in && (b > a || b < a));
                if (lane == 0) s_rise[wave][c] = rs, s_nf[wave][c] = nf;
            }
        __syncthreads();
        int maxloc = 0;
        double arrival = 0.0;
        if (live) {
            // candidates: this lane's falling steps whose last non-flat step before them was a rise
            float best = -INFINITY;
            int best_i = 0x7fffffff;
            for (int c = 0; c < chunks; ++c) {
                const int i = c * WFS_WAVE + lane;
                if (i < 1 || i >= L || !(v[i] < v[i - 1])) continue;
                int j = -1;
                unsigned long long m = s_nf[wave][c] & ((1ull << lane) - 1ull);
                int cc = c;
                while (!m && cc > 0) m = s_nf[wave][--cc];
                if (m) j = cc * WFS_WAVE + 63 - __clzll((long long)m);
                if (j < 0 || !((s_rise[wave][j >> 6] >> (j & 63)) & 1ull)) continue;
                const int lmax = (j + i - 1) >> 1;
                const float val = v[lmax];
                if (val > best) best = val, best_i = lmax;                // ascending i: the first of equal values stays
            }
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(best, o);
                const int oi = __shfl_xor(best_i, o);
                if (ov > best || (ov == best && oi < best_i)) best = ov, best_i = oi;
            }
            if (best_i != 0x7fffffff && best > v[0]) maxloc = best_i;
            // calc_crossing(data, -0.5, maxloc): the first sample below half height walking down from the peak; index 0
            // is never compared
            const double hmax = (double)v[maxloc], thresh = __dmul_rn(0.5, hmax);
            int s = 0;
            for (int c = 0; c < chunks; ++c) {
                const int i = c * WFS_WAVE + lane;
                if (i >= 1 && i <= maxloc && (double)v[i] < thresh) s = i;
            }
            for (int o = 32; o > 0; o >>= 1) {
                const int os = __shfl_xor(s, o);
                s = os > s ? os : s;
            }
            double tx;
            if (s == 0) {
                tx = -(double)maxloc;                                     // ran to the row's start: idx = maxloc
            } else {
                const double prev = (double)(s < maxloc ? v[s + 1] : v[maxloc]), cur = (double)v[s];
                const double q = __ddiv_rn(__dsub_rn(prev, thresh), __dsub_rn(prev, cur));
                tx = -__dadd_rn((double)(maxloc - s - 1), q);
            }
            arrival = __dadd_rn((double)maxloc, tx);
            if (!(0.0 <= arrival && arrival < (double)L)) arrival = (double)maxloc;      // tx = 0
        }
        if (in_cap) {
            const int start = live ? (int)rint(arrival) - 1 : 0;
            if (lane < P) {
                const int i = lane + start;
                out[((long long)side * P + lane) * n_cap + r] = live && i >= 0 && i < L ? v[i] : 0.f;
            }
            if (lane == 0) start_out[r * 2 + side] = start;
        }
        __syncthreads();
    }
}

// ---- rows ------------------------------------------------------------------------------------------------------------
struct ZrPlan {
    int nx, ny, has_pid, pid_int64, n_classes;
    double z_scale;
};

// analyze_wf_z's slices of z in mm (inc = 1200 / NUM_Z_BINS = 120): 0: z <= -600; i = 1 .. 9: -600 + (i - 1) inc < z <=
// -600 + i inc; 10: 480 < z < 600; 11: z >= 600; a NaN is in none (-1)
__device__ __forceinline__ int zr_slice(double z) {
    if (z <= -600.) return 0;
    if (z >= 600.) return ZR_SLICES - 1;
    if (z > 480.) return ZR_SLICES - 2;
    for (int i = 1; i <= 9; ++i)
        if (z > -600. + (i - 1) * 120. && z <= -600. + i * 120.) return i;
    return -1;
}

__global__ void __launch_bounds__(ZB)
k_zreal_rows(const int *__restrict__ coords, Plane pred, Plane tz, Plane te, Plane tp, const void *__restrict__ pid,
             long long n_cap, const long long *__restrict__ n_dev, int B, const float *__restrict__ seg, ZrPlan pp,
             const int *__restrict__ off, float *__restrict__ zp, float *__restrict__ zt, float *__restrict__ en,
             float *__restrict__ mae, float *__restrict__ dmm, float *__restrict__ params, int *__restrict__ cls_cat,
             int *__restrict__ smp_cat, int *__restrict__ se, int *__restrict__ flags) {
    const long long nv = wfs_valid_rows_nonneg(n_cap, n_dev);
    const long long r = (long long)blockIdx.x * ZB + threadIdx.x;
    if (r >= n_cap) return;
    // a row that is not scored (beyond the valid count or flagged) still gets defined outputs
    float o_zp = 0.f, o_zt = 0.f, o_en = 0.f, o_mae = 0.f, o_dmm = 0.f, o_par[4] = {0.f, 0.f, 0.f, 0.f};
    int o_cls = -1, o_smp = -1, o_se = 0;
    if (r < nv) {
        const SegRow h = seg_row(coords, r, nv, off, B, pp.nx, pp.ny, flags);
        if (h.ok) {
            const int e = h.e, cell = h.cell;
            const int n_se = count_single_ended(coords, h.first, h.last, seg, pp.nx, pp.ny);
            o_se = seg[cell] == 0.5f ? 1 : 0;
            o_zp = ld_plane(pred, e, cell), o_zt = ld_plane(tz, e, cell), o_en = ld_plane(te, e, cell);
            const double p = (double)o_zp, t = (double)o_zt;
            o_mae = t == 0.0 ? 0.f : (float)fabs(__dsub_rn(p, t));       // mean_absolute_error_dense
            const double z = __dmul_rn(__dsub_rn(t, 0.5), pp.z_scale), zq = __dmul_rn(__dsub_rn(p, 0.5), pp.z_scale);
            o_dmm = (float)fabs(__dsub_rn(z, zq));
            o_par[0] = o_en, o_par[1] = ld_plane(tp, e, cell), o_par[2] = (float)n_se, o_par[3] = o_zt;
            long long cls = 0;
            if (pp.has_pid) cls = pid_class(ld_pid(pid, pp.pid_int64, r));
            const bool in_classes = cls >= 0 && cls < pp.n_classes;
            if (pp.has_pid && o_se) {
                if (in_classes)
                    o_cls = (int)cls;
                else
                    atomicOr(flags, 4);       // a single-ended row whose class index the class tables do not have
            }
            const int sl = zr_slice(z);
            o_smp = sl >= 0 && in_classes ? sl * pp.n_classes + (int)cls : ZR_SLICES * pp.n_classes;
        }
    }
    zp[r] = o_zp, zt[r] = o_zt, en[r] = o_en, mae[r] = o_mae, dmm[r] = o_dmm;
    cls_cat[r] = o_cls, smp_cat[r] = o_smp, se[r] = o_se;
#pragma unroll
    for (int k = 0; k < 4; ++k) params[(long long)k * n_cap + r] = o_par[k];
}

__global__ void __launch_bounds__(ZB)
k_zreal_baseline(const int *__restrict__ coords, long long n_cap, const long long *__restrict__ n_dev, int B,
                 const int *__restrict__ off, const float *__restrict__ zt, const float *__restrict__ seg, int nx, int ny,
                 float *__restrict__ base) {
    const long long nv = wfs_valid_rows_nonneg(n_cap, n_dev);
    const int e = blockIdx.x * ZB + threadIdx.x;
    if (e >= B) return;
    long long b, last;
    event_run(off, e, nv, &b, &last);
    // the map ZEvaluatorRealWFNorm.add builds, and the look-ahead count of rows that can serve as a source
    int n = 0;
    for (long long r = b; r < last; ++r) {
        const int x = coords[r * 3], y = coords[r * 3 + 1];
        const bool ok = x >= 0 && x < nx && y >= 0 && y < ny;
        const float v = ok && seg[x * ny + y] != 0.5f ? zt[r] : 0.5f;
        base[r] = v;
        if (ok && v != 0.5f) ++n;
    }
    if (n == 0) return;
    for (long long r = b; r < last; ++r) {
        const int x = coords[r * 3], y = coords[r * 3 + 1];
        if (x < 0 || x >= nx || y < 0 || y >= ny || base[r] != 0.5f) continue;
        double sum = 0.0;
        int m = 0;
        for (long long q = r + 1; q < last; ++q) {                        // look ahead
            const float v = base[q];
            if (v != 0.5f && abs(x - coords[q * 3]) == 1 && abs(y - coords[q * 3 + 1]) == 1) sum += (double)v, ++m;
        }
        for (long long q = r - 1; q > 0 && q >= b; --q) {                 // look behind: `ind + a > 0`
            const float v = base[q];
            if (v != 0.5f && abs(x - coords[q * 3]) == 1 && abs(y - coords[q * 3 + 1]) == 1) sum += (double)v, ++m;
        }
        if (m > 0) base[r] = (float)(sum / (double)m);
    }
}

struct ZrBins {
    int nx, ny, nmult, nz, nE;
    double zrange, E_low, E_high;
};

__global__ void __launch_bounds__(ZB)
k_zreal_acc(const int *__restrict__ coords, long long n_cap, const long long *__restrict__ n_dev, int B,
            const int *__restrict__ off, const float *__restrict__ pred, const float *__restrict__ zt,
            const float *__restrict__ en, const float *__restrict__ seg, const int *__restrict__ blindl, ZrBins Z,
            long long *__restrict__ tab, int *__restrict__ flags) {
    const long long nv = wfs_valid_rows_nonneg(n_cap, n_dev);
    const long long r = (long long)blockIdx.x * ZB + threadIdx.x;
    if (r >= nv) return;
    const SegRow h = seg_row(coords, r, nv, off, B, Z.nx, Z.ny, flags);
    if (!h.ok) return;
    const int mult = (int)(h.last - h.first);
    if (mult < 1) return;                     // only with a flagged (unsorted) event column
    const int cell = h.cell, nm1 = Z.nmult + 1, nzb = Z.nz + 2, neb = Z.nE + 2;
    const double p = (double)pred[r], t = (double)zt[r];
    long long v;
    if (!fixed_image(fabs(__dsub_rn(p, t)), &v, flags)) return;          // a NaN row is left out of every table
    // table order: wfs_zreal_table_ints
    const int c_seg = Z.nx * Z.ny * nm1, c_zm = nzb * nm1, c_ze = nzb * neb, c_em = neb * nm1;
    long long *t_seg = tab, *t_zms = t_seg + 2 * c_seg, *t_zmd = t_zms + 2 * c_zm, *t_zes = t_zmd + 2 * c_zm,
              *t_zed = t_zes + 2 * c_ze, *t_ems = t_zed + 2 * c_ze, *t_emd = t_ems + 2 * c_em;
    const double true_z = __dmul_rn(__dsub_rn(t, 0.5), Z.zrange), zw = Z.zrange / Z.nz;
    const int eb = bin_direct((double)en[r], Z.E_low, Z.E_high, Z.nE);
    const int col = mult <= Z.nmult ? mult - 1 : Z.nmult;
    const float s = seg[cell];
    const bool single = s > 0.f;
    if (s == 0.5f || s == 0.f) {
        // a single-ended segment bins the distance from its live PMT; a double-ended one is entered at both distances
        const double first = s == 0.5f && blindl[cell] == 1 ? __dsub_rn(ZR_HALF_CELL, true_z)
                                                            : __dadd_rn(ZR_HALF_CELL, true_z);
        for (int k = 0; k < (s == 0.f ? 2 : 1); ++k) {
            const double dist = k == 0 ? first : __dsub_rn(ZR_HALF_CELL, true_z);
            const int zb = bin_direct_w(dist, 0., ZR_HALF_CELL * 2, zw, Z.nz);
            add_cell(t_seg, c_seg, cell * nm1 + col, v, flags);
            add_cell(single ? t_zms : t_zmd, c_zm, zb * nm1 + col, v, flags);
            add_cell(single ? t_zes : t_zed, c_ze, zb * neb + eb, v, flags);
        }
    }
    add_cell(single ? t_ems : t_emd, c_em, eb * nm1 + col, v, flags);
}

}  // namespace

extern "C" int wfs_align_pulses(const void *feats, int32_t dtype, int64_t n_cap, const int64_t *n_dev, int32_t L,
                                int32_t P, float *samples, int32_t *start, void *stream) {
    WFS_REQUIRE(wfs_dtype_ok(dtype), WFS_EINVAL, "wfs_align_pulses: unknown dtype %d", dtype);
    WFS_REQUIRE(n_cap >= 0 && n_cap < (1ll << 31) && L >= 1 && L <= AL_MAX_L && P >= 1 && P <= AL_MAX_P, WFS_EINVAL,
                "wfs_align_pulses: n_cap = %lld, L = %d (1 .. %d), P = %d (1 .. %d)", (long long)n_cap, L, AL_MAX_L, P,
                AL_MAX_P);
    WFS_REQUIRE(n_cap == 0 || (feats && samples && start), WFS_EINVAL, "wfs_align_pulses: NULL argument");
    if (n_cap == 0) return WFS_OK;
    return wfs_with_dtype(dtype, [&](auto t) -> int {
        using T = decltype(t);
        k_align_pulses<T><<<(unsigned)wfs_cdiv(n_cap, AL_WAVES), AL_THREADS, 0, (hipStream_t)stream>>>(
            (const T *)feats, n_cap, (const long long *)n_dev, L, P, samples, start);
        WFS_LAUNCH_CHECK();
        return WFS_OK;
    });
}

extern "C" int wfs_zreal_row_stats(const int32_t *coords, const void *pred, int32_t pred_dtype, int64_t pred_bs,
                                   int64_t pred_ps, int32_t pred_plane, const void *targ, int32_t targ_dtype,
                                   int64_t targ_bs, int64_t targ_ps, int32_t z_plane, int32_t e_plane, int32_t psd_plane,
                                   const void *pid, int32_t pid_int64, int64_t n_cap, const int64_t *n_dev, int32_t B,
                                   const float *seg_status, int32_t nx, int32_t ny, int32_t n_classes, double z_scale,
                                   int32_t *offsets, float *z_pred, float *z_true, float *energy, float *mae,
                                   float *dev_mm, float *params, int32_t *class_category, int32_t *sample_category,
                                   int32_t *se, int32_t *flags, void *stream) {
    WFS_REQUIRE(B >= 1 && n_cap >= 0 && n_cap < (1ll << 31) && nx >= 1 && ny >= 1 && n_classes >= 1, WFS_EINVAL,
                "wfs_zreal_row_stats: B = %d, n_cap = %lld, grid %d x %d, %d classes", B, (long long)n_cap, nx, ny,
                n_classes);
    WFS_REQUIRE(plane_ok(pred, pred_dtype, pred_bs, pred_ps, pred_plane) &&
                    plane_ok(targ, targ_dtype, targ_bs, targ_ps, z_plane) && e_plane >= 0 && psd_plane >= 0,
                WFS_EINVAL, "wfs_zreal_row_stats: bad map (NULL, unknown dtype or negative stride / plane)");
    WFS_REQUIRE(seg_status && offsets && flags && (pid_int64 == 0 || pid_int64 == 1) &&
                    (n_cap == 0 || (coords && z_pred && z_true && energy && mae && dev_mm && params && class_category &&
                                    sample_category && se)),
                WFS_EINVAL, "wfs_zreal_row_stats: NULL argument");
    if (n_cap == 0) return WFS_OK;
    hipStream_t s = (hipStream_t)stream;
    const unsigned rb = (unsigned)wfs_cdiv(n_cap, ZB);
    if (const int rc = launch_eval_offsets(coords, n_cap, (const long long *)n_dev, B, offsets, flags, s)) return rc;
    const Plane P = {pred, pred_bs, pred_ps * pred_plane, pred_dtype};
    const Plane Tz = {targ, targ_bs, targ_ps * z_plane, targ_dtype}, Te = {targ, targ_bs, targ_ps * e_plane, targ_dtype},
                Tp = {targ, targ_bs, targ_ps * psd_plane, targ_dtype};
    const ZrPlan pp = {nx, ny, pid ? 1 : 0, pid_int64, n_classes, z_scale};
    k_zreal_rows<<<rb, ZB, 0, s>>>(coords, P, Tz, Te, Tp, pid, n_cap, (const long long *)n_dev, B, seg_status, pp, offsets,
                                   z_pred, z_true, energy, mae, dev_mm, params, class_category, sample_category, se,
                                   flags);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}

extern "C" int wfs_zreal_baseline(const int32_t *coords, int64_t n_cap, const int64_t *n_dev, int32_t B,
                                  const int32_t *offsets, const float *z_true, const float *seg_status, int32_t nx,
                                  int32_t ny, float *baseline, void *stream) {
    WFS_REQUIRE_EVAL_BATCH("wfs_zreal_baseline: B", B, n_cap, nx, ny);
    WFS_REQUIRE(offsets && seg_status && (n_cap == 0 || (coords && z_true && baseline)), WFS_EINVAL,
                "wfs_zreal_baseline: NULL argument");
    if (n_cap == 0) return WFS_OK;
    k_zreal_baseline<<<(unsigned)wfs_cdiv(B, ZB), ZB, 0, (hipStream_t)stream>>>(
        coords, n_cap, (const long long *)n_dev, B, offsets, z_true, seg_status, nx, ny, baseline);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}

extern "C" size_t wfs_zreal_table_ints(int32_t nx, int32_t ny, int32_t n_mult, int32_t n_z, int32_t n_E) {
    const size_t nm1 = (size_t)n_mult + 1, nzb = (size_t)n_z + 2, neb = (size_t)n_E + 2;
    return 2 * (size_t)nx * ny * nm1 + 4 * nzb * nm1 + 4 * nzb * neb + 4 * neb * nm1;
}

extern "C" int wfs_zreal_accumulate(const int32_t *coords, int64_t n_cap, const int64_t *n_dev, int32_t B,
                                    const int32_t *offsets, const float *pred_rows, const float *z_true,
                                    const float *energy, const float *seg_status, const int32_t *blind_left, int32_t nx,
                                    int32_t ny, int32_t n_mult, int32_t n_z, double zrange, double E_low, double E_high,
                                    int32_t n_E, int64_t *tables, int32_t *flags, void *stream) {
    WFS_REQUIRE_EVAL_BATCH("wfs_zreal_accumulate: B", B, n_cap, nx, ny);
    WFS_REQUIRE(n_mult >= 1 && n_z >= 1 && n_E >= 1 && zrange > 0 && E_high > E_low, WFS_EINVAL,
                "wfs_zreal_accumulate: bad bin parameters");
    WFS_REQUIRE(offsets && seg_status && blind_left && tables && flags &&
                    (n_cap == 0 || (coords && pred_rows && z_true && energy)),
                WFS_EINVAL, "wfs_zreal_accumulate: NULL argument");
    if (n_cap == 0) return WFS_OK;
    const ZrBins Z = {nx, ny, n_mult, n_z, n_E, zrange, E_low, E_high};
    k_zreal_acc<<<(unsigned)wfs_cdiv(n_cap, ZB), ZB, 0, (hipStream_t)stream>>>(
        coords, n_cap, (const long long *)n_dev, B, offsets, pred_rows, z_true, energy, seg_status, blind_left, Z,
        (long long *)tables, flags);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}
