// evalstats.hip -- the per-batch half of the reference's PSDEvaluator on the device.
//
// The reference's LitPSD.test_step hands every batch to PSDEvaluator.add (src/evaluation/PSDEvaluator.py:101-198), which
// copies coordinates, waveforms and predictions to the host, walks them sample by sample in average_pulse
// (src/utils/SparseUtils.py:405-487) and bins the per-event results.  Here the batch stays in HBM:
//
//   k_eval_offsets   one thread per row: first row of every event from the sorted event column ([E + 1] ints).
//   k_event_stats    ONE WORKGROUP PER EVENT, one wave per row (rows of an event are contiguous).  Pass 1 stages a row in
//                    LDS and computes, per PMT half, charge, charge-weighted time, the half-peak arrival of calc_arrival
//                    and the PSD of calc_psd / integrate_lininterp_range; the wave adds the row into its own fp64 copy of
//                    the event's summed pulse and keeps the event's sums in registers.  Four numbers per row go to a
//                    scratch table for pass 2 (calc_spread needs the event's means first).  Then normalize_coords, the
//                    spreads, the summed pulse (fp32, as the reference stores it) and the two variances of moment().
//                    All sums are fp64 in a fixed order (row -> wave is fixed, waves are added 0..3): no atomics,
//                    bit-identical from run to run.  The caller's rows are only read.
//   k_eval_accumulate one launch, two kinds of block: the first ones take one event per thread and add it to the
//                    persistent int64 tables with integer atomics (exact, order-independent); the others own one
//                    (class slot, 64-sample chunk) of the summed-waveform tables and add the batch's events to it in
//                    event order (fp64, one writer per element).
//
// Bin indices follow the reference's edge arithmetic literally -- the first j with j * width + low > value, a rounded
// product and a rounded sum (no fma) -- with its two overflow conventions (confusion_accumulate_1d / get_bin_index).
#include "wfs_common.h"

#include <limits.h>

namespace {

constexpr int EB = 256;                      // 4 waves per event
constexpr int EW = EB / WFS_WAVE;
constexpr int NPART = 9;

#include "wfs_evoffsets.h"                   // k_eval_offsets (shared with segstats.hip)
static_assert(EB == WFS_EVOFF_THREADS, "k_eval_offsets is launched with EB threads");
#include "wfs_evalbins.h"                   // bin_metric, bin_confusion, add64 (shared with metricpairs.hip)

// butterfly sums: every lane ends with the same bits (a + b and b + a are the same number)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const double o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const int o = __shfl_xor(v, d);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ double block_sum(double v, double *red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0;
#pragma unroll
    for (int w = 0; w < EW; ++w) s += red[w];
    return s;
}
// a wave's LDS stores become visible to its other lanes
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// integrate_lininterp_range(v, r0, r1) over v[j] = raw[j] * g, j in [0, n); the whole wave takes part
__device__ __forceinline__ double integ(const float *raw, double g, int n, double r0, double r1, int lane) {
    const double c0 = ceil(r0), f1 = floor(r1);
    const int i0 = (int)c0, i1 = (int)f1;
    const double d0 = c0 - r0, d1 = r1 - f1;
    double s = 0;
    if (i0 <= i1) {
        const int lo = i0 > 0 ? i0 : 0, hi = i1 < n - 1 ? i1 : n - 1;
        for (int j = lo + lane; j <= hi; j += WFS_WAVE) s += (double)raw[j] * g;
        s = wave_sum(s);
    }
    if (0 <= i0 && i0 < n) s -= (1 - d0) * (1 - d0) / 2 * ((double)raw[i0] * g);
    if (1 <= i0 && i0 <= n) s += d0 * d0 / 2 * ((double)raw[i0 - 1] * g);
    if (0 <= i1 && i1 < n) s -= (1 - d1) * (1 - d1) / 2 * ((double)raw[i1] * g);
    if (-1 <= i1 && i1 < n - 1) s += d1 * d1 / 2 * ((double)raw[i1 + 1] * g);
    return s;
}

template <typename T>
__global__ void __launch_bounds__(EB)
k_event_stats(const int *__restrict__ coords, const T *__restrict__ rows, int Ts, long long n_cap,
              const long long *__restrict__ n_dev, const int *__restrict__ off, int E, const double *__restrict__ gains,
              const float *__restrict__ seg, int nx, int ny, int fix_last, double *__restrict__ rowstats,
              double *__restrict__ avg_coo, float *__restrict__ summed, float *__restrict__ stats, int *__restrict__ mult,
              int *__restrict__ nse, float *__restrict__ psdl, float *__restrict__ psdr, float *__restrict__ energy,
              float *__restrict__ feat, int *__restrict__ flags) {
    extern __shared__ double smem[];
    __shared__ double part[EW][NPART];
    __shared__ double red[EW];
    const int W = 2 * Ts;
    double *acc = smem;                                        // [EW][W] the waves' copies of the summed pulse
    float *raw = reinterpret_cast<float *>(smem + EW * W);      // [EW][W] the row a wave is working on
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int e = blockIdx.x;
    const long long nv = wfs_valid_rows_nonneg(n_cap, n_dev);
    long long b = off[e], en = off[e + 1];
    b = b < 0 ? 0 : (b > nv ? nv : b);
    en = en < 0 ? 0 : (en > nv ? nv : en);
    if (en < b) en = b;                                        // only with a flagged (unsorted) event column
    double *wacc = acc + wid * W;
    float *wraw = raw + wid * W;
    for (int j = lane; j < W; j += WFS_WAVE) wacc[j] = 0;
    double p_totl = 0, p_totr = 0, p_psdl = 0, p_psdr = 0, p_dt = 0, p_E = 0, p_cx = 0, p_cy = 0, p_se = 0;
    for (long long r = b + wid; r < en; r += EW) {
        const int x = coords[r * 3], y = coords[r * 3 + 1];
        double g[2] = {1.0, 1.0};
        float st = 0.f;
        if (x >= 0 && x < nx && y >= 0 && y < ny) {
            g[0] = gains[(x * ny + y) * 2];
            g[1] = gains[(x * ny + y) * 2 + 1];
            st = seg[x * ny + y];
        } else if (lane == 0) {
            atomicOr(flags, 2);                               // a segment outside the detector
        }
        const T *row = rows + r * W;
        wave_sync();                                           // the previous row's reads are done
        for (int j = lane; j < W; j += WFS_WAVE) wraw[j] = wfs_ld(row + j);
        wave_sync();
        double tot[2], tm[2], psd[2], tot32[2], ts32[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float *v = wraw + h * Ts;
            const double gh = g[h];
            double s = 0, ts = 0, pk = 0, s32 = 0, t32 = 0;
            for (int j = lane; j < Ts; j += WFS_WAVE) {
                const double d = (double)v[j] * gh;
                s += d;
                ts += d * (j + 0.5);
                pk = d > pk ? d : pk;
                const double df = (double)(float)d;           // what the reference stores back into its fp32 rows
                s32 += df;
                t32 += df * (j + 0.5);
                wacc[h * Ts + j] += df;
            }
            s = wave_sum(s);
            ts = wave_sum(ts);
            pk = wave_max(pk);
            tot32[h] = wave_sum(s32);
            ts32[h] = wave_sum(t32);
            // calc_arrival: the first sample above half the peak, interpolated
            const double thresh = 0.5 * pk;
            int first = INT_MAX;
            for (int j = lane; j < Ts; j += WFS_WAVE)
                if ((double)v[j] * gh > thresh) {
                    first = j;
                    break;
                }
            first = wave_min(first);
            double arr = 0;
            if (first != INT_MAX) {
                const double d = (double)v[first] * gh;
                if (first == 0) {
                    arr = thresh / d;
                } else {
                    const double dp = (double)v[first - 1] * gh;
                    arr = first + (thresh - dp) / (d - dp);
                }
            }
            // calc_psd with the reference's windows (-3, 11, 50) and a zero baseline residual
            const double fast = integ(v, gh, Ts, arr - 3, arr + 11, lane);
            const double slow = integ(v, gh, Ts, arr + 11, arr + 50, lane);
            psd[h] = (slow + fast) == 0 ? 0 : slow / (slow + fast);
            tot[h] = s;
            tm[h] = s != 0.0 ? ts / s : 0;                     // calc_time
        }
        const double t = tot[0] + tot[1];
        p_totl += tot[0];
        p_totr += tot[1];
        p_psdl += psd[0] * tot[0];
        p_psdr += psd[1] * tot[1];
        p_dt += (tm[1] - tm[0]) * t;
        p_E += t;
        p_cx += x * t;
        p_cy += y * t;
        p_se += st == 0.5f ? 1 : 0;
        if (lane == 0) {
            double *rs = rowstats + r * 4;
            rs[0] = tot32[0];
            rs[1] = tot32[1];
            rs[2] = ts32[0];
            rs[3] = ts32[1];
        }
    }
    if (lane == 0) {
        double *p = part[wid];
        p[0] = p_totl, p[1] = p_totr, p[2] = p_psdl, p[3] = p_psdr, p[4] = p_dt, p[5] = p_E, p[6] = p_cx, p[7] = p_cy,
        p[8] = p_se;
    }
    __syncthreads();
    double q[NPART];
#pragma unroll
    for (int k = 0; k < NPART; ++k) {
        q[k] = 0;
#pragma unroll
        for (int w = 0; w < EW; ++w) q[k] += part[w][k];
    }
    const long long n = en - b;
    const double totL = q[0], totR = q[1];
    const double E_cur = n > 0 ? q[5] / (double)n : 0;
    double dt = q[4], cx = q[6], cy = q[7], pl = q[2], pr = q[3];
    if (totL > 0 || totR > 0) {                                // normalize_coords
        dt /= (totL + totR);
        cx /= (totL + totR);
        cy /= (totL + totR);
    }
    if (totL > 0) pl /= totL;
    if (totR > 0) pr /= totR;
    // calc_spread: a second walk over the event's rows, now that the means are known
    double dx = 0, dy = 0, ddt = 0, dE = 0, stot = 0;
    if (n >= 2) {
        for (long long r = b + tid; r < en; r += EB) {
            const double *rs = rowstats + r * 4;
            const double tl = rs[0], tr = rs[1], timel = rs[2], timer = rs[3];
            const double t = tl + tr;
            stot += t;
            if (tl > 0 && tr > 0) {
                ddt += fabs((timer / tr - timel / tl) - dt) * t;
                dE += fabs(E_cur - t);
            } else if (tl > 0) {
                ddt += fabs(-1.0 * timel / tl - dt) * tl;
                dE += fabs(E_cur - tl);
            } else if (tr > 0) {
                ddt += fabs(timer / tr - dt) * tr;
                dE += fabs(E_cur - tr);
            }
            dx += fabs(coords[r * 3] - cx) * t;
            dy += fabs(coords[r * 3 + 1] - cy) * t;
        }
        dx = block_sum(dx, red);
        dy = block_sum(dy, red);
        ddt = block_sum(ddt, red);
        dE = block_sum(dE, red);
        stot = block_sum(stot, red);
        if (stot > 0) {
            dx /= stot, dy /= stot, ddt /= stot, dE /= (double)n;
        } else {
            dx = dy = ddt = dE = 0;
        }
    }
    // the summed pulse, stored in fp32 as the reference's out_pulses
    float *fs = raw;                                           // [W]; every wave is past its last row (barrier above)
    double esum = 0;
    for (int j = tid; j < W; j += EB) {
        double s = 0;
#pragma unroll
        for (int w = 0; w < EW; ++w) s += acc[w * W + j];
        const float f = (float)s;
        summed[(long long)e * W + j] = f;
        fs[j] = f;
        esum += (double)f;
    }
    esum = block_sum(esum, red);                               // also orders the fs stores before the reads below
    const float ene = (float)(esum * 0.5);
    // moment(times, T, weights = pulse)[0] and moment(pulse, T)[0] over the folded pulse, times[j] = j + 0.5
    double tvar = 0, nvar = 0;
    if (Ts > 1) {
        double sw = 0, ws = 0, su = 0;
        for (int j = tid; j < Ts; j += EB) {
            const double p = (double)(fs[j] + fs[Ts + j]);
            if (p > 0) {
                sw += (j + 0.5) * p;
                ws += p;
            }
            su += p;
        }
        sw = block_sum(sw, red);
        ws = block_sum(ws, red);
        su = block_sum(su, red);
        const double ave_w = ws > 0.0 ? sw / ws : sw / Ts, ave_u = su / Ts;
        double tv = 0, nvs = 0;
        for (int j = tid; j < Ts; j += EB) {
            const double p = (double)(fs[j] + fs[Ts + j]);
            const double a = (j + 0.5) - ave_w;
            tv += ws > 0.0 ? a * a * p : a * a;
            if (p != 0.0) nvs += (p - ave_u) * (p - ave_u);
        }
        tv = block_sum(tv, red);
        nvs = block_sum(nvs, red);
        tvar = ws > 0.0 ? (ws > 1.0 ? tv / (ws - 1) : 0) : tv / (Ts - 1);
        nvar = nvs / (Ts - 1);
    }
    if (tid == 0) {
        avg_coo[e * 2] = cx;
        avg_coo[e * 2 + 1] = cy;
        const float o[6] = {(float)dx, (float)dy, (float)ddt, (float)dE, (float)tvar, (float)nvar};
        for (int k = 0; k < 6; ++k) stats[(long long)k * E + e] = o[k];
        mult[e] = (int)n;
        // the reference's loop never writes n_SE of a batch's last event (it stays 0) unless the caller asks for it
        const int se = (e == E - 1 && !fix_last) ? 0 : (int)q[8];
        nse[e] = se;
        psdl[e] = (float)pl;
        psdr[e] = (float)pr;
        energy[e] = ene;
        // metric_names order: energy, psd, multiplicity, x_dev, y_dev, dt_dev, E_dev, t_variance, n_variance
        feat[e] = ene;
        feat[(long long)E + e] = (float)pl;
        feat[2ll * E + e] = (float)n;
        for (int k = 0; k < 6; ++k) feat[(long long)(3 + k) * E + e] = o[k];
    }
}

struct EvalBins {
    int n_bins, n_mult, n_conf, n_se_max, nx, ny, C;
    double emin, emax, pmin, pmax;
};

__global__ void __launch_bounds__(EB)
k_eval_accumulate(int E, int Ts, EvalBins B, int event_blocks, const double *__restrict__ avg_coo,
                  const float *__restrict__ summed, const int *__restrict__ mult, const int *__restrict__ nse,
                  const float *__restrict__ psdl, const float *__restrict__ psdr, const float *__restrict__ energy,
                  const long long *__restrict__ pred, const long long *__restrict__ labels, long long *__restrict__ tab,
                  double *__restrict__ sum_wf, double *__restrict__ sum_lab, int *__restrict__ flags) {
    const int C = B.C, W = 2 * Ts;
    if ((int)blockIdx.x < event_blocks) {
        const int e = blockIdx.x * EB + threadIdx.x;
        if (e >= E) return;
        const long long p = pred[e], l = labels[e];
        if (p < 0 || p >= C || l < 0 || l >= C) {
            atomicOr(flags, 4);                              // a class outside the evaluator's class_names
            return;
        }
        const long long hit = p == l ? 1 : 0;
        // table order: wfs_eval_table_ints
        long long *t = tab;
        const int nm = B.n_mult + 2, ne = B.n_bins + 2, px = B.nx + 2, py = B.ny + 2;
        const int m = mult[e];
        const double en = (double)energy[e];
        int k = bin_metric((double)m, 0.5, B.n_mult + 0.5, B.n_mult);
        add64(t + k, 1);
        add64(t + nm + k, hit);
        t += 2 * nm;
        const int bx = bin_metric(en, B.emin, B.emax, B.n_bins);
        const int byl = bin_metric((double)psdl[e], B.pmin, B.pmax, B.n_bins);
        const int byr = bin_metric((double)psdr[e], B.pmin, B.pmax, B.n_bins);
        add64(t + bx * ne + byl, 1);
        add64(t + bx * ne + byr, 1);
        add64(t + ne * ne + bx * ne + byl, hit);
        add64(t + ne * ne + bx * ne + byr, hit);
        t += 2 * ne * ne;
        const int qx = bin_metric(avg_coo[e * 2], 0.0, (double)B.nx, B.nx);
        const int qy = bin_metric(avg_coo[e * 2 + 1], 0.0, (double)B.ny, B.ny);
        add64(t + qx * py + qy, 1);
        add64(t + px * py + qx * py + qy, hit);
        t += 2 * px * py;
        k = bin_confusion(en, 0.0, B.emax, B.n_conf);
        if (k >= 0) add64(t + ((long long)k * C + l) * C + p, 1);
        t += (B.n_conf + 1) * C * C;
        k = bin_confusion((double)nse[e], -0.5, B.n_se_max + 0.5, B.n_se_max + 1);
        if (k >= 0) add64(t + ((long long)k * C + l) * C + p, 1);
        t += (B.n_se_max + 2) * C * C;
        add64(t, m);                                         // n_wfs [C + 1]
        add64(t + 1 + l, m);
        add64(t + C + 1 + p, m);                             // n_labelled_wfs [C]
        return;
    }
    // summed waveforms: slot 0 all events, 1 .. C by label, C + 1 .. 2C by prediction; 64 samples x 4 event quarters
    __shared__ double quarter[EW][WFS_WAVE];
    const int chunks = (W + WFS_WAVE - 1) / WFS_WAVE;
    const int id = blockIdx.x - event_blocks;
    const int slot = id / chunks, j = (id - slot * chunks) * WFS_WAVE + (threadIdx.x & 63), g = threadIdx.x >> 6;
    const int per = (E + EW - 1) / EW;
    const int e0 = g * per, e1 = e0 + per < E ? e0 + per : E;
    const long long *key = slot == 0 ? nullptr : (slot <= C ? labels : pred);
    const long long want = slot <= C ? slot - 1 : slot - C - 1;
    double s = 0;
    if (j < W)
        for (int e = e0; e < e1; ++e)
            if (!key || key[e] == want) s += (double)summed[(long long)e * W + j];
    quarter[g][threadIdx.x & 63] = s;
    __syncthreads();
    if (g == 0 && j < W) {
        double tot = 0;
#pragma unroll
        for (int w = 0; w < EW; ++w) tot += quarter[w][threadIdx.x];
        double *dst = slot <= C ? sum_wf + (long long)slot * W : sum_lab + (long long)(slot - C - 1) * W;
        dst[j] += tot;
    }
}

size_t stats_lds_bytes(int T) { return (size_t)EW * 2 * T * (sizeof(double) + sizeof(float)); }

}  // namespace

extern "C" size_t wfs_eval_table_ints(int32_t n_bins, int32_t n_mult, int32_t n_confusion, int32_t n_se_max, int32_t nx,
                                      int32_t ny, int32_t n_classes) {
    const size_t C = (size_t)n_classes, ne = (size_t)n_bins + 2;
    return 2 * ((size_t)n_mult + 2) + 2 * ne * ne + 2 * ((size_t)nx + 2) * ((size_t)ny + 2) +
           ((size_t)n_confusion + 1) * C * C + ((size_t)n_se_max + 2) * C * C + (C + 1) + C;
}

extern "C" int wfs_event_pulse_stats(const int32_t *coords, const void *rows, int64_t n_cap, int32_t T, int32_t dtype,
                                     const int64_t *n_dev, int32_t E, const double *gains, const float *seg_status,
                                     int32_t nx, int32_t ny, int32_t fix_last_n_se, int32_t *offsets, double *rowstats,
                                     double *avg_coo, float *summed, float *stats, int32_t *multiplicity, int32_t *n_se,
                                     float *psdl, float *psdr, float *energy, float *features, int32_t *flags,
                                     void *stream) {
    WFS_REQUIRE(wfs_dtype_ok(dtype), WFS_EINVAL, "wfs_event_pulse_stats: unknown dtype %d", dtype);
    WFS_REQUIRE(T >= 1 && T <= WFS_EVAL_MAX_SAMPLES, WFS_EINVAL, "wfs_event_pulse_stats: T = %d outside [1, %d]", T,
                WFS_EVAL_MAX_SAMPLES);
    WFS_REQUIRE(E >= 1 && n_cap >= 0 && n_cap < (1ll << 31) && nx >= 1 && ny >= 1, WFS_EINVAL,
                "wfs_event_pulse_stats: E = %d, n_cap = %lld, grid %d x %d", E, (long long)n_cap, nx, ny);
    WFS_REQUIRE(coords && rows && gains && seg_status && offsets && rowstats && avg_coo && summed && stats &&
                    multiplicity && n_se && psdl && psdr && energy && features && flags,
                WFS_EINVAL, "wfs_event_pulse_stats: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    const unsigned rb = (unsigned)(n_cap > 0 ? wfs_cdiv(n_cap, EB) : 1);
    k_eval_offsets<<<rb, EB, 0, s>>>(coords, n_cap, (const long long *)n_dev, E, offsets, flags);
    WFS_LAUNCH_CHECK();
    const size_t lds = stats_lds_bytes(T);
    return wfs_with_dtype(dtype, [&](auto t) -> int {
        using TYPE = decltype(t);
        k_event_stats<TYPE><<<E, EB, lds, s>>>(coords, (const TYPE *)rows, T, n_cap, (const long long *)n_dev, offsets, E,
                                               gains, seg_status, nx, ny, fix_last_n_se, rowstats, avg_coo, summed, stats,
                                               multiplicity, n_se, psdl, psdr, energy, features, flags);
        WFS_LAUNCH_CHECK();
        return WFS_OK;
    });
}

extern "C" int wfs_eval_accumulate(int32_t E, int32_t T, int32_t n_classes, const double *avg_coo, const float *summed,
                                   const int32_t *multiplicity, const int32_t *n_se, const float *psdl,
                                   const float *psdr, const float *energy, const int64_t *predictions,
                                   const int64_t *labels, int32_t n_bins, int32_t n_mult, int32_t n_confusion,
                                   int32_t n_se_max, int32_t nx, int32_t ny, double emin, double emax, double psd_min,
                                   double psd_max, int64_t *tables, double *sum_wf, double *sum_labelled, int32_t *flags,
                                   void *stream) {
    WFS_REQUIRE(E >= 1 && T >= 1 && T <= WFS_EVAL_MAX_SAMPLES && n_classes >= 1, WFS_EINVAL,
                "wfs_eval_accumulate: E = %d, T = %d, classes = %d", E, T, n_classes);
    WFS_REQUIRE(n_bins >= 1 && n_mult >= 1 && n_confusion >= 1 && n_se_max >= 0 && nx >= 1 && ny >= 1, WFS_EINVAL,
                "wfs_eval_accumulate: bad bin counts");
    WFS_REQUIRE(avg_coo && summed && multiplicity && n_se && psdl && psdr && energy && predictions && labels && tables &&
                    sum_wf && sum_labelled && flags,
                WFS_EINVAL, "wfs_eval_accumulate: NULL argument");
    EvalBins B = {n_bins, n_mult, n_confusion, n_se_max, nx, ny, n_classes, emin, emax, psd_min, psd_max};
    const int event_blocks = (int)wfs_cdiv(E, EB);
    const int chunks = (int)wfs_cdiv(2 * T, WFS_WAVE);
    const unsigned grid = (unsigned)(event_blocks + (2 * n_classes + 1) * chunks);
    k_eval_accumulate<<<grid, EB, 0, (hipStream_t)stream>>>(
        E, T, B, event_blocks, avg_coo, summed, multiplicity, n_se, psdl, psdr, energy, (const long long *)predictions,
        (const long long *)labels, (long long *)tables, sum_wf, sum_labelled, flags);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}
