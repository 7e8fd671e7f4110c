// calibz.hip -- the reference's classical calibrated reconstruction on the device: calc_calib_z_E of
// src/utils/SparseUtils.py:938-1026 with everything under it (find_peaks, cull_peaks, remove_end_zeros, match_peaks,
// peak_to_z, peak_to_dt, z_dt_to_z, z_from_total_light, calc_arrival_from_peak, calc_size, sum1d, lin_interp; :532-935),
// z and E of a segment from its two waveforms and the calibration curves.
//
//   k_calib_z_E   one WAVEFRONT per row (the shape of k_align_pulses, zreal.hip).  Both sides' L samples are staged once
//                 into LDS by unit-stride lanes.  Per side and 64-sample chunk two ballots give the masks of rising and of
//                 non-flat steps; a falling step at i closes a local maximum exactly when the last non-flat step before it
//                 was a rise at j (find_peaks' local_maxpos), the maximum is the plateau centre (j + i - 1) / 2.  A ballot
//                 per chunk ranks the maxima in the order they occur, the first 50 are kept as find_peaks keeps them.
//                 The reference's stable descending sort by value is a rank sort, one maximum per lane: a maximum's place
//                 is the number of maxima above it plus the number of equal ones in front of it.  What follows is short
//                 and serial in the reference; every lane computes it alike on wave-uniform values (no divergence, lane 0
//                 stores): the greedy choice of at most 5 maxima more than 2 * minsep apart, the cull, the pairing.  The
//                 two searches with width are done across the lanes: calc_arrival_from_peak's walk down the rising edge
//                 is the LARGEST s < peak with v[s] < half height (a max reduction), and lin_interp's first curve point
//                 beyond x is one ballot over the <= 64 points of a curve.  calc_size and sum1d add in the reference's
//                 order, ascending, so the sums are the reference's to the last bit.
//
// Arithmetic is fp64 on the stored values with contraction off, as in physstats.hip.  Quirks kept: a side on which all five
// slots survive the cull counts as having NO peaks (remove_end_zeros(.., -1) finds no -1); both sides' peak lists are
// sorted DESCENDING before they are paired; cull_peaks' second clause compares the normalised sample with 15; for unequal
// counts the energy-weighted mean of the dt (in ns) goes into z_dt_to_z where a z belongs; a NaN z clamps to 650.
// Departures: the reference's sort of more than 41 maxima takes a merge path that does not sort, the device sorts any
// count; where numba raises (a zero divisor) or a value has no image (not finite) the device sets flag 16 and stores the
// value as it is, the callers leave the row out.  No atomics but the flag word's.
#include "wfs_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int CZ_WAVES = 4, CZ_THREADS = CZ_WAVES * WFS_WAVE;
constexpr int CZ_MAX_L = WFS_CALIB_MAX_L, CZ_MAX_CHUNKS = CZ_MAX_L / WFS_WAVE;
constexpr int CZ_MAX_CAND = 50;               // find_peaks' local_maxima
constexpr int CZ_KEEP = WFS_CALIB_PEAKS;      // calc_calib_z_E's local_maxima0 / 1
constexpr int CZ_MINSEP = 10;
constexpr double CZ_MAX_RANGE = 16383.;       // src/datasets/HDF5Dataset.py MAX_RANGE = 2^14 - 1
constexpr int CZ_NT = WFS_CALIB_T_POINTS, CZ_NTP = WFS_CALIB_TIME_POINTS, CZ_NLP = WFS_CALIB_LIGHT_POINTS,
              CZ_NLS = WFS_CALIB_SUM_POINTS;
static_assert(CZ_NT <= WFS_WAVE && CZ_NTP <= WFS_WAVE && CZ_NLP <= WFS_WAVE && CZ_NLS <= WFS_WAVE && CZ_NT > 10,
              "lin_interp finds its point with one ballot");

struct Curves {
    const double *gain, *eres, *rel, *st, *tint, *tpos, *lpos, *lsum;
};

// lin_interp(xy, x): the first point whose abscissa lies beyond x; wave-uniform x, every lane active
__device__ __forceinline__ double lin_interp(const double *__restrict__ xy, int n, double x, int lane) {
    const unsigned long long m = __ballot(lane < n && xy[2 * lane] > x);
    if (!m) return xy[2 * (n - 1) + 1];
    const int i = __ffsll((long long)m) - 1;
    if (i == 0) return xy[1];
    const double x0 = xy[2 * i - 2], y0 = xy[2 * i - 1], x1 = xy[2 * i], y1 = xy[2 * i + 1];
    return y0 + (x - x0) * ((y1 - y0) / (x1 - x0));
}

// calc_arrival_from_peak(fdat, peak_ind)
__device__ __forceinline__ double arrival_from_peak(const float *v, int chunks, int pk, int lane) {
    if (pk == 0) return 0.5;
    const double thresh = 0.5 * (double)v[pk];
    int s = -1;
    for (int c = 0; c < chunks; ++c) {
        const int i = c * WFS_WAVE + lane;
        if (i < pk && (double)v[i] < thresh) s = i;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const int os = __shfl_xor(s, o);
        s = os > s ? os : s;
    }
    if (s < 0) return thresh / (double)v[0];
    const double cur = (double)v[s];
    return (double)(s + 1) + (thresh - cur) / ((double)v[s + 1] - cur);
}

// sum_range(data, start, stop), ascending; calc_size's residual term is n * 0
__device__ __forceinline__ double sum_range(const float *v, int L, int r0, int r1) {
    r0 = r0 >= 0 ? r0 : 0;
    if (!(r0 < L)) return 0.0;
    r1 = r1 < L ? r1 : L - 1;
    double s = 0.0;
    for (int i = r0; i <= r1; ++i) s += (double)v[i];
    return s;
}
__device__ __forceinline__ double calc_size(const float *v, int L, int pk) { return sum_range(v, L, pk - 3, pk + 25); }

// Python's max([a, 1.0]): a NaN in front stays
__device__ __forceinline__ double max_with_one(double a) { return 1.0 > a ? 1.0 : a; }
__device__ __forceinline__ double clamp650(double z) { return fabs(z) < 650. ? z : (z < -650. ? -650. : 650.); }

// the two arrival times of peak_to_z / peak_to_dt, in ns, through the t_interp curve where the PMT has one
__device__ __forceinline__ void arrival_times(const float *v0, const float *v1, int chunks, int m0, int m1, int cell,
                                              const Curves &C, double sw, int lane, double *t) {
    t[0] = arrival_from_peak(v0, chunks, m0, lane) * sw;
    t[1] = arrival_from_peak(v1, chunks, m1, lane) * sw;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const double *curve = C.tint + (long long)(cell * 2 + i) * CZ_NT * 2;
        if (curve[10 * 2] == 0.0) continue;
        const double st = C.st[cell * 2 + i];
        const double t0 = st * floor(t[i] / st);
        t[i] = t0 + lin_interp(curve, CZ_NT, t[i] - t0, lane);
    }
}

// the light half shared by peak_to_z and z_from_total_light: R, its validity, dRpos
struct Light {
    double PE0, PE1, R, dRpos;
    bool valid;
};
__device__ __forceinline__ Light light_ratio(double L0, double L1, int cell, const Curves &C, int lane) {
    Light q;
    q.PE0 = L0 * C.eres[cell * 2], q.PE1 = L1 * C.eres[cell * 2 + 1];
    q.R = log(L1 / L0);
    q.valid = q.R == q.R;
    const double dR = sqrt(1.0 / max_with_one(q.PE0) + 1.0 / max_with_one(q.PE1));
    const double *lp = C.lpos + (long long)cell * CZ_NLP * 2;
    q.dRpos = q.valid ? fabs(lin_interp(lp, CZ_NLP, q.R + 0.5 * dR, lane) - lin_interp(lp, CZ_NLP, q.R - 0.5 * dR, lane))
                      : 0.0;
    return q;
}

__device__ __forceinline__ void peak_to_z(const float *v0, const float *v1, int L, int chunks, int m0, int m1, int cell,
                                          const Curves &C, double sw, int lane, double *z_out, double *E_out) {
    double t[2];
    arrival_times(v0, v1, chunks, m0, m1, cell, C, sw, lane, t);
    const double dt = t[1] - t[0] - C.rel[cell];
    const double tpos = lin_interp(C.tpos + (long long)cell * CZ_NTP * 2, CZ_NTP, dt, lane);
    const double L0 = calc_size(v0, L, m0) * C.gain[cell * 2], L1 = calc_size(v1, L, m1) * C.gain[cell * 2 + 1];
    const double *ls = C.lsum + (long long)cell * CZ_NLS * 2;
    if (L0 == 0.0 || L1 == 0.0) {
        *z_out = 0.0, *E_out = (L0 + L1) / lin_interp(ls, CZ_NLS, 0.0, lane);
        return;
    }
    const Light q = light_ratio(L0, L1, cell, C, lane);
    const double Rpos = q.valid ? lin_interp(C.lpos + (long long)cell * CZ_NLP * 2, CZ_NLP, q.R, lane) : 0.0;
    const double Rweight = q.dRpos > 0.0 ? 1.0 / (q.dRpos * q.dRpos) : 0.0;
    const double tweight = 1.0 / (60 * 60);
    const double z = clamp650((Rweight * Rpos + tweight * tpos) / (Rweight + tweight));
    *z_out = z, *E_out = (q.PE0 + q.PE1) / lin_interp(ls, CZ_NLS, z, lane);
}

__device__ __forceinline__ void peak_to_dt(const float *v0, const float *v1, int L, int chunks, int m0, int m1, int cell,
                                           const Curves &C, double sw, int lane, double *dt, double *area) {
    double t[2];
    arrival_times(v0, v1, chunks, m0, m1, cell, C, sw, lane, t);
    const double L0 = calc_size(v0, L, m0) * C.gain[cell * 2], L1 = calc_size(v1, L, m1) * C.gain[cell * 2 + 1];
    *dt = t[1] - t[0] - C.rel[cell], *area = L0 + L1;
}

// z_dt_to_z over z_from_total_light
__device__ __forceinline__ void z_dt_to_z(const float *v0, const float *v1, int L, double z_dt, int cell, const Curves &C,
                                          int lane, double *z_out, double *E_out) {
    const double L0 = sum_range(v0, L, 0, L - 1) * C.gain[cell * 2], L1 = sum_range(v1, L, 0, L - 1) * C.gain[cell * 2 + 1];
    const double *ls = C.lsum + (long long)cell * CZ_NLS * 2;
    const double w_dt = 1.0 / (60. * 60.);
    double z, w, E;
    if (L0 == 0.0 || L1 == 0.0) {
        z = 0.0, w = 1.0 / 100000., E = (L0 + L1) / lin_interp(ls, CZ_NLS, 0.0, lane);
    } else {
        const Light q = light_ratio(L0, L1, cell, C, lane);
        z = clamp650(q.valid ? lin_interp(C.lpos + (long long)cell * CZ_NLP * 2, CZ_NLP, q.R, lane) : 0.0);
        w = q.dRpos > 0.0 ? 1.0 / (q.dRpos * q.dRpos) : 0.0;
        E = (q.PE0 + q.PE1) / lin_interp(ls, CZ_NLS, z, lane);
    }
    *z_out = (w_dt * z_dt + z * w) / (w + w_dt), *E_out = E;
}

template <typename T>
__global__ void __launch_bounds__(CZ_THREADS)
k_calib_z_E(const T *__restrict__ feats, const int *__restrict__ coords, long long n_cap,
            const long long *__restrict__ n_dev, int L, int nx, int ny, Curves C, double sw, double z_scale,
            double *__restrict__ z_out, double *__restrict__ E_out, int *__restrict__ state_out,
            int *__restrict__ peaks_out, int *__restrict__ flags) {
    __shared__ float sv[CZ_WAVES][2][CZ_MAX_L];
    __shared__ unsigned long long s_nf[CZ_WAVES][CZ_MAX_CHUNKS], s_rise[CZ_WAVES][CZ_MAX_CHUNKS];
    __shared__ float s_val[CZ_WAVES][CZ_MAX_CAND];
    __shared__ int s_loc[CZ_WAVES][CZ_MAX_CAND], s_sorted[CZ_WAVES][CZ_MAX_CAND];
    __shared__ int s_pk[CZ_WAVES][2][CZ_KEEP];          // the culled peaks of a side, -1 behind them
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long nv = wfs_valid_rows_nonneg(n_cap, n_dev);
    const long long r = (long long)blockIdx.x * CZ_WAVES + wave;
    const bool in_cap = r < n_cap;                                       // wave-uniform, as everything below
    bool live = r < nv;
    const int chunks = (L + WFS_WAVE - 1) / WFS_WAVE;
    const unsigned long long below = (1ull << lane) - 1ull;
    int cell = 0;
    if (live) {
        const int x = coords[r * 3], y = coords[r * 3 + 1];
        if (x < 0 || x >= nx || y < 0 || y >= ny) {
            if (lane == 0) atomicOr(flags, 2);
            live = false;
        } else {
            cell = x * ny + y;
        }
    }
    bool finite = true;
    if (live) {
        const T *row = feats + r * 2 * L;
        bool bad = false;
        for (int i = lane; i < 2 * L; i += WFS_WAVE) {
            const float f = wfs_ld(row + i);
            sv[wave][i >= L ? 1 : 0][i >= L ? i - L : i] = f;
            bad = bad || !(fabsf(f) <= 3.402823466e38f);
        }
        finite = !__ballot(bad);
    }
    int n_pk[2] = {0, 0};
    for (int side = 0; side < 2; ++side) {
        const float *v = sv[wave][side];
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
        int n = 0;
        if (live)
            for (int c = 0; c < chunks; ++c) {
                const int i = c * WFS_WAVE + lane;
                bool cand = false;
                int lmax = 0;
                if (i >= 1 && i < L && v[i] < v[i - 1]) {
                    int j = -1;
                    unsigned long long m = s_nf[wave][c] & below;
                    int cc = c;
                    while (!m && cc > 0) m = s_nf[wave][--cc];
                    if (m) j = cc * WFS_WAVE + 63 - __clzll((long long)m);
                    if (j >= 0 && ((s_rise[wave][j >> 6] >> (j & 63)) & 1ull)) cand = true, lmax = (j + i - 1) >> 1;
                }
                const unsigned long long cm = __ballot(cand);
                const int at = n + __popcll(cm & below);
                if (cand && at < CZ_MAX_CAND) s_loc[wave][at] = lmax, s_val[wave][at] = v[lmax];
                n += __popcll(cm);
            }
        n = n < CZ_MAX_CAND ? n : CZ_MAX_CAND;
        __syncthreads();
        // merge_sort_two for up to 41 entries: a stable descending insertion sort by value
        if (live && lane < n) {
            const float mine = s_val[wave][lane];
            int place = 0;
            for (int j = 0; j < n; ++j) {
                const float o = s_val[wave][j];
                place += (o > mine || (o == mine && j < lane)) ? 1 : 0;
            }
            s_sorted[wave][place] = s_loc[wave][lane];
        }
        __syncthreads();
        int kept[CZ_KEEP], gmax = 0, cnt = 0;
#pragma unroll
        for (int k = 0; k < CZ_KEEP; ++k) kept[k] = -1;
        if (live && finite && n == 1) {
            kept[0] = s_loc[wave][0], cnt = 1;
            gmax = v[kept[0]] > v[0] ? kept[0] : 0;
        } else if (live && finite && n > 1) {
            gmax = kept[0] = s_sorted[wave][0], cnt = 1;
            for (int i = 1; i < n && cnt < CZ_KEEP; ++i) {
                const int c = s_sorted[wave][i];
                bool apart = true;
#pragma unroll
                for (int k = 0; k < CZ_KEEP; ++k) apart = apart && !(k < cnt && abs(c - kept[k]) <= 2 * CZ_MINSEP);
                if (apart) {
#pragma unroll
                    for (int k = 0; k < CZ_KEEP; ++k)
                        if (k == cnt) kept[k] = c;
                    ++cnt;
                }
            }
        }
        // cull_peaks; every lane stores the same values
        int nc = 0;
#pragma unroll
        for (int k = 0; k < CZ_KEEP; ++k) s_pk[wave][side][k] = -1;
#pragma unroll
        for (int k = 0; k < CZ_KEEP; ++k)
            if (k < cnt) {
                const double w = (double)v[kept[k]];
                if (w * CZ_MAX_RANGE > 30. || (w > 15. && kept[k] == gmax)) s_pk[wave][side][nc++] = kept[k];
            }
        n_pk[side] = nc;
        if (in_cap && lane < CZ_KEEP) peaks_out[(r * 2 + side) * CZ_KEEP + lane] = s_pk[wave][side][lane];
    }
    // remove_end_zeros(.., -1): no peak, or all five slots taken, is None
    const int n0 = n_pk[0] == CZ_KEEP ? 0 : n_pk[0], n1 = n_pk[1] == CZ_KEEP ? 0 : n_pk[1];
    double z = 0.0, E = 0.0;
    int state = 0;
    if (live && !finite) {
        z = E = __longlong_as_double(0x7ff8000000000000ll);
    } else if (live && (n0 > 0 || n1 > 0)) {
        const float *v0 = sv[wave][0], *v1 = sv[wave][1];
        const double *ls = C.lsum + (long long)cell * CZ_NLS * 2;
        if (n0 == 0 || n1 == 0) {
            const int side = n0 == 0 ? 1 : 0;
            state = 1;
            const double Ls = sum_range(side ? v1 : v0, L, 0, L - 1) * C.gain[cell * 2 + side];
            z = 0.5, E = Ls * C.eres[cell * 2 + side] / lin_interp(ls, CZ_NLS, 0.0, lane);
        } else {
            // merge_sort_main_numba: both lists descending (at most 4 entries, insertion sort)
            for (int side = 0; side < 2; ++side) {
                int *p = s_pk[wave][side];
                const int np = side ? n1 : n0;
                for (int i = 1; i < np; ++i) {
                    const int key = p[i];
                    int j = i - 1;
                    while (j >= 0 && p[j] < key) p[j + 1] = p[j], --j;
                    p[j + 1] = key;
                }
            }
            const int *p0 = s_pk[wave][0], *p1 = s_pk[wave][1];
            if (n0 == n1) {
                state = 2;
                double zw = 0.0, area = 0.0;
                for (int k = 0; k < n0; ++k) {
                    double pz, pE;
                    peak_to_z(v0, v1, L, chunks, p0[k], p1[k], cell, C, sw, lane, &pz, &pE);
                    zw += pz * pE, area += pE;
                }
                z = zw / area / z_scale + 0.5, E = area;
            } else {
                state = 3;
                const bool small0 = n0 < n1;
                const int *small = small0 ? p0 : p1, *large = small0 ? p1 : p0;
                const int ns = small0 ? n0 : n1, nl = small0 ? n1 : n0;
                double zw = 0.0, tot = 0.0;
                for (int i = 0; i < ns; ++i) {
                    int ld = 100000, ind = 0;                             // match_peaks
                    for (int j = 0; j < nl; ++j) {
                        const int d = abs(small[i] - large[j]);
                        if (d < ld) ld = d, ind = j;
                    }
                    double dt, area;
                    peak_to_dt(v0, v1, L, chunks, small0 ? small[i] : large[ind], small0 ? large[ind] : small[i], cell, C,
                               sw, lane, &dt, &area);
                    zw += dt * area, tot += area;
                }
                double zz;
                z_dt_to_z(v0, v1, L, zw / tot, cell, C, lane, &zz, &E);
                z = zz / z_scale + 0.5;
            }
        }
        if (!(fabs(z) <= 1.7976931348623157e308) || !(fabs(E) <= 1.7976931348623157e308)) finite = false;
    }
    if (live && !finite && lane == 0) atomicOr(flags, 16);
    if (in_cap && lane == 0) z_out[r] = z, E_out[r] = E, state_out[r] = state;
}

}  // namespace

extern "C" int wfs_calib_z_E(const void *feats, int32_t dtype, const int32_t *coords, int64_t n_cap, const int64_t *n_dev,
                             int32_t L, int32_t nx, int32_t ny, const double *gain_factor, const double *eres,
                             const double *rel_times, const double *sampletime, const double *t_interp_curves,
                             const double *time_pos_curves, const double *light_pos_curves, const double *light_sum_curves,
                             int32_t sample_width, double z_scale, double *z_cal, double *E_cal, int32_t *state,
                             int32_t *peaks, int32_t *flags, void *stream) {
    WFS_REQUIRE(wfs_dtype_ok(dtype), WFS_EINVAL, "wfs_calib_z_E: unknown dtype %d", dtype);
    WFS_REQUIRE(n_cap >= 0 && n_cap < (1ll << 31) && L >= 2 && L <= CZ_MAX_L && nx >= 1 && ny >= 1 && sample_width >= 1 &&
                    z_scale != 0,
                WFS_EINVAL, "wfs_calib_z_E: n_cap = %lld, L = %d (2 .. %d), grid %d x %d, sample_width = %d",
                (long long)n_cap, L, CZ_MAX_L, nx, ny, sample_width);
    WFS_REQUIRE(gain_factor && eres && rel_times && sampletime && t_interp_curves && time_pos_curves && light_pos_curves &&
                    light_sum_curves && flags && (n_cap == 0 || (feats && coords && z_cal && E_cal && state && peaks)),
                WFS_EINVAL, "wfs_calib_z_E: NULL argument");
    if (n_cap == 0) return WFS_OK;
    const Curves C = {gain_factor, eres, rel_times, sampletime, t_interp_curves, time_pos_curves, light_pos_curves,
                      light_sum_curves};
    return wfs_with_dtype(dtype, [&](auto t) -> int {
        using T = decltype(t);
        k_calib_z_E<T><<<(unsigned)wfs_cdiv(n_cap, CZ_WAVES), CZ_THREADS, 0, (hipStream_t)stream>>>(
            (const T *)feats, coords, n_cap, (const long long *)n_dev, L, nx, ny, C, (double)(float)sample_width, z_scale,
            z_cal, E_cal, state, peaks, flags);
        WFS_LAUNCH_CHECK();
        return WFS_OK;
    });
}
