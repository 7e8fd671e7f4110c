// metricpairs.hip -- the reference's MetricPairAggregator and the per-row half of its PIDEvaluator on the device; in the
// second half of the file the same for a real-valued result, with the per-row half of its TensorEvaluator.
//
// MetricPairAggregator.add / add_normalized (src/evaluation/MetricAggregator.py:339-366) bins a 0/1 result of every
// element by each of P parameters (metric_accumulate_1d) and by every pair i < j (metric_accumulate_2d), per class.  Both
// reference callers feed it a 0/1 result (find_matches, calculate_class_accuracy), so every table here is an int64 count
// -- a count table and a match-sum table -- exact, independent of the order the elements arrive in and bit-identical from
// run to run; the running mean / M2 of metric_accumulate_1d follow from the two counts on the host.
//
//   k_metric_pairs   one thread per element, grid-stride over slices of MP_SLICE elements per workgroup.  The 1-D tables
//                    (few cells, every element hits P of them: the contended ones) go through an int32 image of them in
//                    LDS that the workgroup flushes sparsely with int64 atomics; the pair tables (many cells, P(P-1)/2
//                    hits spread over them) take int64 global atomics directly.  A miss adds nothing to a match-sum.
//   k_pid_rows       one thread per row of a LitSegClassifier batch: accuracy, multiplicity (the length of the row's event
//                    run from the offsets of wfs_evoffsets.h), single-ended flag, single-ended rows of its event, the
//                    [4, N] parameter matrix and the category of PIDEvaluator.add (src/evaluation/PIDEvaluator.py:93-135);
//                    the three confusion tables are folded in the same launch.
//
// Bins: get_bin_index in fp64 on the fp32 value of the element, without walking the bins: the candidate
// floor((v - low) / width) + 1 is corrected by the reference's own predicate j * width + low > v (a rounded product and
// a rounded sum, no fma) at the candidate and its neighbours, so every value lands where the walk would put it --
// including the value just below `high` for which no edge is above it (bin 0) and NaN (bin 0).
#include "wfs_common.h"

namespace {

#include "wfs_evoffsets.h"
#include "wfs_segrows.h"
#include "wfs_evalbins.h"
#include "wfs_segtables.h"

constexpr int MB = WFS_EVOFF_THREADS;
constexpr int MP_MAX = 16;                    // WFS_METRIC_PAIRS_MAX
constexpr int MP_SLICE = 4 * MB;              // elements per workgroup pass
constexpr int MP_LDS_CELLS = 4096;            // cells of the 1-D image (2 x 16 KB of int32); above it the 1-D tables go direct
constexpr int PID_CLASSES = 5;                // WFS_PID_CLASSES

#ifndef MP_LDS_1D
#define MP_LDS_1D 1                           // 0: timing variant, every table by direct global atomics
#endif

struct PairPlan {
    int P, C, cells1;                         // cells1: sum over i of C * (nb[i] + 2)
    int nb[MP_MAX];
    double lo[MP_MAX], hi[MP_MAX];
    long long off1[MP_MAX];                   // metric i: count table, then the match-sum table C * (nb[i] + 2) further
                                              // (k_metric_pairs_real: count, S and the three limbs of Q)
    long long off2[MP_MAX];                   // first pair of row i (i_i+1); the pairs i_j follow in j
    int img[MP_MAX];                          // metric i's offset in the LDS image
};

template <bool LDS1D>
__global__ void __launch_bounds__(MB)
k_metric_pairs(const float *__restrict__ params, const int *__restrict__ result, const int *__restrict__ category,
               long long M, const long long *__restrict__ n_dev, PairPlan pl, long long *__restrict__ tab,
               int *__restrict__ flags) {
    extern __shared__ int image[];            // [2][cells1]: counts, then match sums
    const long long nv = wfs_valid_rows_nonneg(M, n_dev);
    const int P = pl.P, C = pl.C;
    for (long long base = (long long)blockIdx.x * MP_SLICE; base < nv; base += (long long)gridDim.x * MP_SLICE) {
        if (LDS1D) {
            for (int k = threadIdx.x; k < 2 * pl.cells1; k += MB) image[k] = 0;
            __syncthreads();
        }
        for (int s = 0; s < MP_SLICE / MB; ++s) {
            const long long m = base + s * MB + threadIdx.x;
            if (m >= nv) break;
            const int cat = category[m];
            if (cat == -1) continue;
            const int res = result[m];
            if (cat < -1 || cat >= C) {
                atomicOr(flags, 4);           // a class outside class_names
                continue;
            }
            if (res != 0 && res != 1) {
                atomicOr(flags, 8);           // not a 0/1 result
                continue;
            }
            int b[MP_MAX];
#pragma unroll
            for (int i = 0; i < MP_MAX; ++i)
                b[i] = i < P ? bin_direct((double)params[(long long)i * M + m], pl.lo[i], pl.hi[i], pl.nb[i]) : 0;
            for (int i = 0; i < P; ++i) {
                const int ni = pl.nb[i] + 2;
                if (LDS1D) {
                    const int cell = pl.img[i] + cat * ni + b[i];
                    atomicAdd(image + cell, 1);
                    if (res) atomicAdd(image + pl.cells1 + cell, 1);
                } else {
                    long long *t = tab + pl.off1[i] + (long long)cat * ni + b[i];
                    add64(t, 1);
                    if (res) add64(t + (long long)C * ni, 1);
                }
                long long *t2 = tab + pl.off2[i];
                for (int j = i + 1; j < P; ++j) {
                    const int nj = pl.nb[j] + 2;
                    const long long cells = (long long)C * ni * nj;
                    long long *t = t2 + ((long long)cat * ni + b[i]) * nj + b[j];
                    add64(t, 1);
                    if (res) add64(t + cells, 1);
                    t2 += 2 * cells;
                }
            }
        }
        if (LDS1D) {
            __syncthreads();
            // the image's cells in table order: metric i's count cells, then its match-sum cells
            for (int k = threadIdx.x; k < 2 * pl.cells1; k += MB) {
                const int v = image[k];
                if (v == 0) continue;
                const int half = k >= pl.cells1 ? 1 : 0, cell = k - half * pl.cells1;
                int i = 0;
                while (i + 1 < P && pl.img[i + 1] <= cell) ++i;
                const long long sz = (long long)C * (pl.nb[i] + 2);
                add64(tab + pl.off1[i] + half * sz + (cell - pl.img[i]), v);
            }
            __syncthreads();
        }
    }
}

// result = (prediction == label), category = label, for a caller that holds int64 class indices
__global__ void __launch_bounds__(MB)
k_match_categories(const long long *__restrict__ pred, const long long *__restrict__ labels, long long M,
                   int *__restrict__ result, int *__restrict__ category) {
    const long long m = (long long)blockIdx.x * MB + threadIdx.x;
    if (m >= M) return;
    const long long l = labels[m];
    result[m] = pred[m] == l ? 1 : 0;
    category[m] = l >= 0 && l < (1ll << 30) ? (int)l : -2;       // outside any class count: flagged by the accumulate
}

struct PidPlan {
    int nx, ny, n_phys, e_index, psd_index, z_index, n_conf, n_se_max;
    double e_high;                            // n_confusion / E_scale
};

template <typename T>
__global__ void __launch_bounds__(MB)
k_pid_rows(const int *__restrict__ coords, const long long *__restrict__ pred, const long long *__restrict__ targ,
           const T *__restrict__ phys, long long n_cap, const long long *__restrict__ n_dev, int E,
           const float *__restrict__ seg, PidPlan pp, const int *__restrict__ off, int *__restrict__ accuracy,
           int *__restrict__ mult, int *__restrict__ se, int *__restrict__ n_se, float *__restrict__ params,
           int *__restrict__ category, long long *__restrict__ tab, int *__restrict__ flags) {
    const long long nv = wfs_valid_rows_nonneg(n_cap, n_dev);
    const long long r = (long long)blockIdx.x * MB + threadIdx.x;
    if (r >= n_cap) return;
    // a row that is not scored (beyond the valid count or flagged) still gets defined outputs; category -1 keeps it out
    // of the pair tables
    int o_acc = 0, o_mult = 0, o_se = 0, o_nse = 0, o_cat = -1;
    float o_par[4] = {0.f, 0.f, 0.f, 0.f};
    if (r < nv) {
        const SegRow h = seg_row(coords, r, nv, off, E, pp.nx, pp.ny, flags);
        const long long p = pred[r], t = targ[r];
        const bool classes_ok = p >= 0 && p < PID_CLASSES && t >= 0 && t < PID_CLASSES;
        if (h.ok && !classes_ok) {
            atomicOr(flags, 4);               // a class outside PID_MAPPED_NAMES
        } else if (h.ok) {
            o_mult = (int)(h.last - h.first);
            o_nse = count_single_ended(coords, h.first, h.last, seg, pp.nx, pp.ny);
            o_acc = p == t ? 1 : 0;
            o_se = seg[h.cell] == 0.5f ? 1 : 0;
            const T *row = phys + r * pp.n_phys;
            o_par[0] = wfs_ld(row + pp.e_index);
            o_par[1] = wfs_ld(row + pp.psd_index);
            o_par[2] = (float)o_mult;
            o_par[3] = wfs_ld(row + pp.z_index);
            o_cat = o_se ? (int)t : -1;
            // table order: wfs_pid_table_ints
            constexpr int CC = PID_CLASSES * PID_CLASSES;
            const long long cell = t * PID_CLASSES + p;
            long long *t_se = tab, *t_nse = t_se + CC, *t_ene = t_nse + (long long)(pp.n_se_max + 2) * CC;
            if (o_se) add64(t_se + cell, 1);
            int k = bin_confusion((double)o_nse, -0.5, pp.n_se_max + 0.5, pp.n_se_max + 1);
            if (k >= 0) add64(t_nse + (long long)k * CC + cell, 1);
            k = bin_confusion((double)o_par[0], 0.0, pp.e_high, pp.n_conf);
            if (k >= 0) add64(t_ene + (long long)k * CC + cell, 1);
        }
    }
    accuracy[r] = o_acc;
    mult[r] = o_mult;
    se[r] = o_se;
    n_se[r] = o_nse;
    category[r] = o_cat;
#pragma unroll
    for (int k = 0; k < 4; ++k) params[(long long)k * n_cap + r] = o_par[k];
}

// k1: int64 tables per metric (2: count + match sum; the real-valued accumulate keeps MPR_TABS)
bool make_plan(int P, const int32_t *nbins, const double *lo, const double *hi, int C, PairPlan *pl, size_t *total,
               int k1 = 2) {
    if (P < 1 || P > MP_MAX || C < 1 || !nbins) return false;
    pl->P = P, pl->C = C;
    size_t at = 0;
    int img = 0;
    for (int i = 0; i < P; ++i) {
        if (nbins[i] < 1 || nbins[i] > (1 << 20)) return false;
        if (lo && hi && !(hi[i] > lo[i])) return false;
        pl->nb[i] = nbins[i];
        pl->lo[i] = lo ? lo[i] : 0.0;
        pl->hi[i] = hi ? hi[i] : 1.0;
        pl->off1[i] = (long long)at;
        pl->img[i] = img;
        at += (size_t)k1 * (size_t)C * ((size_t)nbins[i] + 2);
        if ((size_t)img + (size_t)C * ((size_t)nbins[i] + 2) > (size_t)1 << 30) return false;
        img += C * (nbins[i] + 2);
    }
    pl->cells1 = img;
    for (int i = 0; i < P; ++i) {
        pl->off2[i] = (long long)at;
        for (int j = i + 1; j < P; ++j) at += 2 * (size_t)C * ((size_t)nbins[i] + 2) * ((size_t)nbins[j] + 2);
    }
    for (int i = P; i < MP_MAX; ++i) pl->nb[i] = 1, pl->lo[i] = 0, pl->hi[i] = 1, pl->off1[i] = pl->off2[i] = 0, pl->img[i] = 0;
    *total = at;
    return true;
}

}  // namespace

extern "C" size_t wfs_metric_pairs_table_ints(int32_t P, const int32_t *nbins, int32_t n_classes) {
    PairPlan pl;
    size_t total = 0;
    return make_plan(P, nbins, nullptr, nullptr, n_classes, &pl, &total) ? total : 0;
}

extern "C" int wfs_metric_pairs_accumulate(const float *params, const int32_t *result, const int32_t *category,
                                           int64_t M, const int64_t *n_dev, int32_t P, const double *lo,
                                           const double *hi, const int32_t *nbins, int32_t n_classes, int64_t *tables,
                                           int32_t *flags, void *stream) {
    PairPlan pl;
    size_t total = 0;
    WFS_REQUIRE(lo && hi && make_plan(P, nbins, lo, hi, n_classes, &pl, &total), WFS_EINVAL,
                "wfs_metric_pairs_accumulate: P = %d (1 .. %d), classes = %d, or a bad bin count / range (high > low)", P,
                MP_MAX, n_classes);
    WFS_REQUIRE(M >= 0 && M < (1ll << 31), WFS_EINVAL, "wfs_metric_pairs_accumulate: M = %lld", (long long)M);
    WFS_REQUIRE(tables && flags && (M == 0 || (params && result && category)), WFS_EINVAL,
                "wfs_metric_pairs_accumulate: NULL argument");
    if (M == 0) return WFS_OK;
    long long blocks = wfs_cdiv(M, MP_SLICE);
    if (blocks > 1024) blocks = 1024;
    hipStream_t s = (hipStream_t)stream;
    if (MP_LDS_1D && pl.cells1 <= MP_LDS_CELLS)
        k_metric_pairs<true><<<(unsigned)blocks, MB, 2 * (size_t)pl.cells1 * sizeof(int), s>>>(
            params, result, category, M, (const long long *)n_dev, pl, (long long *)tables, flags);
    else
        k_metric_pairs<false><<<(unsigned)blocks, MB, 0, s>>>(params, result, category, M, (const long long *)n_dev, pl,
                                                              (long long *)tables, flags);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}

extern "C" int wfs_match_categories(const int64_t *predictions, const int64_t *labels, int64_t M, int32_t *result,
                                    int32_t *category, void *stream) {
    WFS_REQUIRE(M >= 0 && M < (1ll << 31), WFS_EINVAL, "wfs_match_categories: M = %lld", (long long)M);
    WFS_REQUIRE(M == 0 || (predictions && labels && result && category), WFS_EINVAL, "wfs_match_categories: NULL argument");
    if (M == 0) return WFS_OK;
    k_match_categories<<<(unsigned)wfs_cdiv(M, MB), MB, 0, (hipStream_t)stream>>>(
        (const long long *)predictions, (const long long *)labels, M, result, category);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}

extern "C" size_t wfs_pid_table_ints(int32_t n_confusion, int32_t n_se_max) {
    return (size_t)PID_CLASSES * PID_CLASSES * (1 + ((size_t)n_se_max + 2) + ((size_t)n_confusion + 1));
}

extern "C" int wfs_pid_row_stats(const int32_t *coords, const int64_t *predictions, const int64_t *targets,
                                 const void *phys, int32_t n_phys, int32_t dtype, int64_t n_cap, const int64_t *n_dev,
                                 int32_t E, const float *seg_status, int32_t nx, int32_t ny, int32_t e_index,
                                 int32_t psd_index, int32_t z_index, int32_t n_confusion, int32_t n_se_max,
                                 double e_high, int32_t *offsets, int32_t *accuracy, int32_t *multiplicity, int32_t *se,
                                 int32_t *n_se, float *params, int32_t *category, int64_t *tables, int32_t *flags,
                                 void *stream) {
    WFS_REQUIRE(wfs_dtype_ok(dtype), WFS_EINVAL, "wfs_pid_row_stats: unknown dtype %d", dtype);
    WFS_REQUIRE_EVAL_BATCH("wfs_pid_row_stats: E", E, n_cap, nx, ny);
    WFS_REQUIRE(n_phys >= 1 && e_index >= 0 && e_index < n_phys && psd_index >= 0 && psd_index < n_phys && z_index >= 0 &&
                    z_index < n_phys,
                WFS_EINVAL, "wfs_pid_row_stats: column indices %d, %d, %d outside [0, %d)", e_index, psd_index, z_index,
                n_phys);
    WFS_REQUIRE(n_confusion >= 1 && n_se_max >= 0 && e_high > 0, WFS_EINVAL, "wfs_pid_row_stats: bad bin parameters");
    WFS_REQUIRE(seg_status && offsets && tables && flags &&
                    (n_cap == 0 || (coords && predictions && targets && phys && accuracy && multiplicity && se && n_se &&
                                    params && category)),
                WFS_EINVAL, "wfs_pid_row_stats: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    if (n_cap == 0) return WFS_OK;
    const unsigned rb = (unsigned)wfs_cdiv(n_cap, MB);
    if (const int rc = launch_eval_offsets(coords, n_cap, (const long long *)n_dev, E, offsets, flags, s)) return rc;
    const PidPlan pp = {nx, ny, n_phys, e_index, psd_index, z_index, n_confusion, n_se_max, e_high};
    return wfs_with_dtype(dtype, [&](auto t) -> int {
        using TYPE = decltype(t);
        k_pid_rows<TYPE><<<rb, MB, 0, s>>>(coords, (const long long *)predictions, (const long long *)targets,
                                           (const TYPE *)phys, n_cap, (const long long *)n_dev, E, seg_status, pp, offsets,
                                           accuracy, multiplicity, se, n_se, params, category, (long long *)tables, flags);
        WFS_LAUNCH_CHECK();
        return WFS_OK;
    });
}

// ---- real-valued results: the reference's TensorEvaluator (src/evaluation/TensorEvaluator.py:70-91) -------------------
//
// A result that is a loss value, not 0/1: the mean and M2 of metric_accumulate_1d no longer follow from two counts.  Per
// 1-D cell the tables keep n, S = sum v and Q = sum v^2 of the fixed-point image v = round(r * 2^32) of the result, Q as
// three int64 limbs holding the 32-bit pieces of v^2 (|r| < 2^15, so v^2 < 2^94 and every limb sum fits an int64 for up
// to 2^31 elements per cell); per pair cell n and S.  Integer atomics only, so the tables do not depend on the order of
// the rows or on the launch shape; the host forms mean = S / (n 2^32) and M2 = (n Q - S^2) / (n 2^64) from integers.
//
//   k_tensor_rows          one thread per row of a LitWaveform batch: the [P, N] parameter matrix (the transposed target,
//                          or the single target), the category (0, or -1 beyond the valid rows) and the per-PMT count /
//                          loss-sum tables of TensorEvaluator.add's loop over (x, y, side).
//   k_metric_pairs_real    k_metric_pairs's shape and bin_direct; the 1-D cells through an int64 image in LDS where they
//                          fit (MPR_LDS_CELLS), by direct global atomics above that; the pair cells direct.
namespace {

constexpr int MPR_TABS = 5;                   // per 1-D cell: n, S, and the limbs Q0, Q1, Q2
constexpr int MPR_LDS_CELLS = 1024;           // cells of the 1-D image (5 x 8 KB of int64)
#ifndef MPR_SLICE_ROWS
#define MPR_SLICE_ROWS 1                      // elements per thread and workgroup pass
#endif
#ifndef MPR_BINS_LDS
#define MPR_BINS_LDS 1                        // 0: timing variant, the element's bin indices in a private array
#endif
constexpr int MPR_SLICE = MPR_SLICE_ROWS * MB;
constexpr int TENSOR_DET_ROW = 14;            // det == 2 * (14 * j + i) + k
constexpr int MPR_WRAP = 16;                  // flag: a cell's S left int64 (add_fixed, wfs_segtables.h)

template <bool LDS1D>
__global__ void __launch_bounds__(MB)
k_metric_pairs_real(const float *__restrict__ params, const float *__restrict__ result,
                    const int *__restrict__ category, long long M, const long long *__restrict__ n_dev, PairPlan pl,
                    long long *__restrict__ tab, int *__restrict__ flags) {
    extern __shared__ long long image64[];    // [MPR_TABS][cells1]
#if MPR_BINS_LDS
    // the element's bin indices: the loops over metrics are not unrolled, and a private array indexed by them would live
    // in scratch memory
    __shared__ int bins[MP_MAX][MB];
#endif
    const long long nv = wfs_valid_rows_nonneg(M, n_dev);
    const int P = pl.P, C = pl.C, cells1 = pl.cells1;
    for (long long base = (long long)blockIdx.x * MPR_SLICE; base < nv; base += (long long)gridDim.x * MPR_SLICE) {
        if (LDS1D) {
            for (int k = threadIdx.x; k < MPR_TABS * cells1; k += MB) image64[k] = 0;
            __syncthreads();
        }
        for (int s = 0; s < MPR_SLICE / MB; ++s) {
            const long long m = base + s * MB + threadIdx.x;
            if (m >= nv) break;
            const int cat = category[m];
            if (cat == -1) continue;
            if (cat < -1 || cat >= C) {
                atomicOr(flags, 4);           // a class outside class_names
                continue;
            }
            long long v;
            if (!real_image(result[m], &v, flags)) continue;
            // v^2 < 2^94 in 32-bit pieces
            const unsigned long long a = (unsigned long long)(v < 0 ? -v : v);
            const unsigned long long lo = a * a;
            const long long q[3] = {(long long)(lo & 0xffffffffull), (long long)(lo >> 32), (long long)__umul64hi(a, a)};
#if MPR_BINS_LDS
            for (int i = 0; i < P; ++i)
                bins[i][threadIdx.x] = bin_direct((double)params[(long long)i * M + m], pl.lo[i], pl.hi[i], pl.nb[i]);
#define MPR_BIN(i) bins[i][threadIdx.x]
#else
            int b[MP_MAX];
#pragma unroll
            for (int i = 0; i < MP_MAX; ++i)
                b[i] = i < P ? bin_direct((double)params[(long long)i * M + m], pl.lo[i], pl.hi[i], pl.nb[i]) : 0;
#define MPR_BIN(i) b[i]
#endif
            for (int i = 0; i < P; ++i) {
                const int ni = pl.nb[i] + 2, bi = MPR_BIN(i);
                if (LDS1D) {
                    unsigned long long *c = reinterpret_cast<unsigned long long *>(image64) + pl.img[i] + cat * ni + bi;
                    atomicAdd(c, 1ull);
                    if (v != 0) {             // a slice's S stays below 2^10 * 2^47
                        atomicAdd(c + cells1, (unsigned long long)v);
#pragma unroll
                        for (int k = 0; k < 3; ++k)
                            if (q[k] != 0) atomicAdd(c + (2 + k) * cells1, (unsigned long long)q[k]);
                    }
                } else {
                    const long long sz = (long long)C * ni;
                    long long *t = tab + pl.off1[i] + (long long)cat * ni + bi;
                    add64(t, 1);
                    if (v != 0) {
                        add_fixed(t + sz, v, flags, MPR_WRAP);
#pragma unroll
                        for (int k = 0; k < 3; ++k)
                            if (q[k] != 0) add64(t + (2 + k) * sz, q[k]);
                    }
                }
                long long *t2 = tab + pl.off2[i];
                for (int j = i + 1; j < P; ++j) {
                    const int nj = pl.nb[j] + 2;
                    const long long cells = (long long)C * ni * nj;
                    long long *t = t2 + ((long long)cat * ni + bi) * nj + MPR_BIN(j);
                    add64(t, 1);
                    if (v != 0) add_fixed(t + cells, v, flags, MPR_WRAP);
                    t2 += 2 * cells;
                }
            }
#undef MPR_BIN
        }
        if (LDS1D) {
            __syncthreads();
            // the image's cells in table order: metric i's n cells, then its S cells, then the limbs
            for (int k = threadIdx.x; k < MPR_TABS * cells1; k += MB) {
                const long long v = image64[k];
                if (v == 0) continue;
                const int which = k / cells1, cell = k - which * cells1;
                int i = 0;
                while (i + 1 < P && pl.img[i + 1] <= cell) ++i;
                const long long sz = (long long)C * (pl.nb[i] + 2);
                long long *t = tab + pl.off1[i] + which * sz + (cell - pl.img[i]);
                if (which == 1)
                    add_fixed(t, v, flags, MPR_WRAP);
                else
                    add64(t, v);
            }
            __syncthreads();
        }
    }
}

template <typename T>
__device__ __forceinline__ float target_f32(const T *p) {
    return wfs_ld(p);
}
template <>
__device__ __forceinline__ float target_f32<long long>(const long long *p) {
    return (float)*p;                         // a class index
}

// CT: int or long long coordinates; T: the target's element type
template <typename CT, typename T>
__global__ void __launch_bounds__(MB)
k_tensor_rows(const CT *__restrict__ c, int c_cols, const T *__restrict__ target, int P,
              const float *__restrict__ results, long long N, const long long *__restrict__ n_dev, int nx, int ny,
              float *__restrict__ params, int *__restrict__ category, long long *__restrict__ det,
              int *__restrict__ flags) {
    const long long nv = wfs_valid_rows_nonneg(N, n_dev);
    const long long r = (long long)blockIdx.x * MB + threadIdx.x;
    if (r >= N) return;
    if (r >= nv) {                            // beyond the valid count: defined outputs, category -1, nothing read
        category[r] = -1;
        for (int k = 0; k < P; ++k) params[(long long)k * N + r] = 0.f;
        return;
    }
    for (int k = 0; k < P; ++k) params[(long long)k * N + r] = target_f32(target + r * P + k);
    category[r] = 0;
    long long x, y, side;
    if (c_cols == 1) {
        const long long d = (long long)c[r];
        if (d < 0) return;                    // no (i, j, k) gives a negative number
        side = d & 1;
        x = (d >> 1) % TENSOR_DET_ROW;
        y = (d >> 1) / TENSOR_DET_ROW;
    } else {
        x = (long long)c[r * 3], y = (long long)c[r * 3 + 1], side = (long long)c[r * 3 + 2];
    }
    // a PMT outside the grid: the reference's loop over (i, j, k) never selects the row
    if (x < 0 || x >= nx || y < 0 || y >= ny || side < 0 || side > 1) return;
    long long v;
    if (!real_image(results[r], &v, flags)) return;
    const long long cells = (long long)nx * ny * 2, cell = (x * ny + y) * 2 + side;
    add64(det + cell, 1);
    if (v != 0) add_fixed(det + cells + cell, v, flags, MPR_WRAP);
}

}  // namespace

extern "C" size_t wfs_metric_pairs_real_table_ints(int32_t P, const int32_t *nbins, int32_t n_classes) {
    PairPlan pl;
    size_t total = 0;
    return make_plan(P, nbins, nullptr, nullptr, n_classes, &pl, &total, MPR_TABS) ? total : 0;
}

extern "C" int wfs_metric_pairs_accumulate_real(const float *params, const float *result, const int32_t *category,
                                                int64_t M, const int64_t *n_dev, int32_t P, const double *lo,
                                                const double *hi, const int32_t *nbins, int32_t n_classes,
                                                int64_t *tables, int32_t *flags, void *stream) {
    PairPlan pl;
    size_t total = 0;
    WFS_REQUIRE(lo && hi && make_plan(P, nbins, lo, hi, n_classes, &pl, &total, MPR_TABS), WFS_EINVAL,
                "wfs_metric_pairs_accumulate_real: P = %d (1 .. %d), classes = %d, or a bad bin count / range (high > low)",
                P, MP_MAX, n_classes);
    WFS_REQUIRE(M >= 0 && M < (1ll << 31), WFS_EINVAL, "wfs_metric_pairs_accumulate_real: M = %lld", (long long)M);
    WFS_REQUIRE(tables && flags && (M == 0 || (params && result && category)), WFS_EINVAL,
                "wfs_metric_pairs_accumulate_real: NULL argument");
    if (M == 0) return WFS_OK;
    long long blocks = wfs_cdiv(M, MPR_SLICE);
    if (blocks > 1024) blocks = 1024;
    hipStream_t s = (hipStream_t)stream;
    if (MP_LDS_1D && pl.cells1 <= MPR_LDS_CELLS)
        k_metric_pairs_real<true><<<(unsigned)blocks, MB, (size_t)MPR_TABS * pl.cells1 * sizeof(long long), s>>>(
            params, result, category, M, (const long long *)n_dev, pl, (long long *)tables, flags);
    else
        k_metric_pairs_real<false><<<(unsigned)blocks, MB, 0, s>>>(params, result, category, M, (const long long *)n_dev,
                                                                   pl, (long long *)tables, flags);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}

extern "C" int wfs_tensor_rows(const void *c, int32_t c_int64, int32_t c_cols, const void *target,
                               int32_t target_dtype, int32_t P, const float *results, int64_t N, const int64_t *n_dev,
                               int32_t nx, int32_t ny, float *params, int32_t *category, int64_t *det_tables,
                               int32_t *flags, void *stream) {
    WFS_REQUIRE(wfs_dtype_ok(target_dtype) || target_dtype == WFS_TENSOR_TARGET_I64, WFS_EINVAL,
                "wfs_tensor_rows: unknown target dtype %d", target_dtype);
    WFS_REQUIRE((c_cols == 1 || c_cols == 3) && (c_int64 == 0 || c_int64 == 1), WFS_EINVAL,
                "wfs_tensor_rows: c must be detector numbers [N] or (x, y, side) rows [N, 3] of int32 / int64");
    WFS_REQUIRE(P >= 1 && P <= MP_MAX && N >= 0 && N < (1ll << 31) && nx >= 1 && nx <= TENSOR_DET_ROW && ny >= 1 &&
                    ny <= (1 << 15),
                WFS_EINVAL, "wfs_tensor_rows: P = %d (1 .. %d), N = %lld, grid %d x %d", P, MP_MAX, (long long)N, nx, ny);
    WFS_REQUIRE(det_tables && flags && (N == 0 || (c && target && results && params && category)), WFS_EINVAL,
                "wfs_tensor_rows: NULL argument");
    if (N == 0) return WFS_OK;
    const unsigned rb = (unsigned)wfs_cdiv(N, MB);
    hipStream_t s = (hipStream_t)stream;
    const auto rows = [&](auto t) -> int {
        using TYPE = decltype(t);
        if (c_int64)
            k_tensor_rows<long long, TYPE><<<rb, MB, 0, s>>>((const long long *)c, c_cols, (const TYPE *)target, P, results, N,
                                                             (const long long *)n_dev, nx, ny, params, category,
                                                             (long long *)det_tables, flags);
        else
            k_tensor_rows<int, TYPE><<<rb, MB, 0, s>>>((const int *)c, c_cols, (const TYPE *)target, P, results, N,
                                                       (const long long *)n_dev, nx, ny, params, category,
                                                       (long long *)det_tables, flags);
        WFS_LAUNCH_CHECK();
        return WFS_OK;
    };
    if (wfs_dtype_ok(target_dtype)) return wfs_with_dtype(target_dtype, rows);
    return rows((long long)0);                   // WFS_TENSOR_TARGET_I64: class indices
}
