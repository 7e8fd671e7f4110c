// segquant.hip -- the per-segment regression module (the reference's LitSegQuantifier) on the device: its masked loss for
// the training step, and the per-row half of its evaluator (src/evaluation/SegEvaluator.py with StatsUtils.ErrorAggregator).
//
// Masked regression loss: the mean of |d| (L1) or d^2 (MSE), d = pred - target[:, col], over the rows below the valid
// count that lie on a single-ended segment (when a mask is given), with the mean of d^2 over the same rows beside it.
//
//   k_mrl_forward    ONE launch.  The rows are cut into chunks of MRL_CHUNK by row index, whatever the grid: a workgroup
//                    sums a chunk in a fixed shape (every thread its MRL_CHUNK / MRL_THREADS rows in row order, then a
//                    fixed tree over the threads) and stores the chunk's (count, sum, sum of squares).  The workgroup that
//                    draws the last ticket folds the chunk sums -- every thread its chunks in chunk order, then the same
//                    tree -- and writes count, loss and mse.  d and every sum are fp64; there is no floating-point atomic,
//                    so the result repeats bit for bit and does not depend on the grid (nor on the rows' capacity: a chunk
//                    beyond the valid rows adds an exact 0).  The hand-off is one agent-scope release in each workgroup
//                    (after its chunk stores have drained) in front of a relaxed ticket add, and one agent-scope acquire in
//                    the last one; the last one puts the ticket back to 0.
//   k_mrl_backward   ONE launch, one thread per row: dpred = g * s / count in pred's type, s = sign(d) (sign(0) = 0) or 2 d.
//
// A row that is not counted is SELECTED out: none of its values is loaded into the arithmetic (beyond the valid count not
// even its coordinates), so a NaN, an Inf or the captured step's padding value there cannot reach the loss, and its
// gradient is a stored 0.  With no row counted the loss is NaN (0 / 0, torch's mean over nothing) and dpred is all zeros.
//
// Evaluator (SegEvaluator.add): after the event offsets of wfs_evoffsets.h,
//   k_segq_rows      one thread per row: error = results - target[:, ti] in fp64, mae = |error|, multiplicity (the length of
//                    the row's event run), the single-ended flag, the [4, N] parameters (E, PSD, multiplicity, z), the PID
//                    slot (class_PIDs in order: 1 | 4 | 6, 258 | 256 | 512) and the category (the slot's class on a valid
//                    single-ended row whose PID is in the map, else -1; without PID: class 0 for every valid row, no mask).
//                    The same launch is the ErrorAggregator's first pass: per slot the row count and max |error|, folded in
//                    LDS and flushed with an integer atomicMax on the bits of the non-negative value (a NaN's bits lie
//                    above every finite value's, so a NaN error surfaces as a max that is not finite).
//   k_segq_edges     one workgroup: a class whose edges are not yet set takes the first slot with rows -- the reference's
//                    first add_norm call that reaches the class -- and stores (edges[0], edges[-1]) of get_bins(-1.1 max,
//                    1.1 max, nb) (wfs_erroredges.h); a max that is 0 or not finite sets the class's bit in the error
//                    flags and leaves the edges unset.  It clears the slot scratch for the next add.
//   k_segq_bins      one thread per row: error_hist by the class's edges, error_2d by (actual, predicted) over [0, 1], both
//                    through bin_direct (wfs_evalbins.h) as int64 counts.
#include "wfs_common.h"
#include "wfs_erroredges.h"
#include "wfs_rows.h"                         // ldt / stt: rows of a runtime dtype

namespace {

#include "wfs_evoffsets.h"
#include "wfs_segrows.h"
#include "wfs_evalbins.h"

constexpr int MB = WFS_EVOFF_THREADS;
constexpr int MRL_THREADS = 256;
constexpr int MRL_ROWS = 4;                   // rows per thread and chunk
constexpr int MRL_CHUNK = MRL_THREADS * MRL_ROWS;
constexpr int MRL_MAX_BLOCKS = 256;
constexpr int MRL_HEAD = 16;                  // workspace: the ticket (and padding), then 3 x 8 bytes per chunk
constexpr int SEGQ_SLOTS = 6, SEGQ_CLASSES = 5;

struct MrlIn {
    const void *pred, *target;
    const int *coords;
    const float *mask;                        // [nx, ny] or NULL
    const long long *n_dev;
    long long n_cap;
    int pred_dtype, target_dtype, n_cols, col, nx, ny, kind;
};

// row r (below the valid count) is counted: on a single-ended segment when there is a mask
__device__ __forceinline__ bool mrl_counted(const MrlIn &in, long long r) {
    if (!in.mask) return true;
    const int x = in.coords[r * 3], y = in.coords[r * 3 + 1];
    return x >= 0 && x < in.nx && y >= 0 && y < in.ny && in.mask[x * in.ny + y] == 1.0f;
}

// fixed tree over the workgroup's threads; the result is in thread 0
__device__ __forceinline__ void mrl_tree(double *sa, double *sb, long long *sc, double &a, double &b, long long &c) {
    const int t = threadIdx.x;
    sa[t] = a, sb[t] = b, sc[t] = c;
    __syncthreads();
    for (int s = MRL_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) sa[t] += sa[t + s], sb[t] += sb[t + s], sc[t] += sc[t + s];
        __syncthreads();
    }
    a = sa[0], b = sb[0], c = sc[0];
    __syncthreads();
}

__global__ void __launch_bounds__(MRL_THREADS)
k_mrl_forward(MrlIn in, long long n_chunks, unsigned *__restrict__ ticket, double *__restrict__ part,
              float *__restrict__ out, long long *__restrict__ count) {
    __shared__ double sa[MRL_THREADS], sb[MRL_THREADS];
    __shared__ long long sc[MRL_THREADS];
    const long long nv = wfs_valid_rows_nonneg(in.n_cap, in.n_dev);
    const int t = threadIdx.x;
    for (long long ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
        double a = 0.0, b = 0.0;
        long long c = 0;
#pragma unroll
        for (int j = 0; j < MRL_ROWS; ++j) {
            const long long r = ch * MRL_CHUNK + (long long)j * MRL_THREADS + t;
            if (r < nv && mrl_counted(in, r)) {
                const double d = (double)ldt(in.pred, r, in.pred_dtype) -
                                 (double)ldt(in.target, r * in.n_cols + in.col, in.target_dtype);
                const double q = d * d;
                a += in.kind == WFS_LOSS_L1 ? fabs(d) : q;
                b += q;
                ++c;
            }
        }
        mrl_tree(sa, sb, sc, a, b, c);
        if (t == 0) {
            part[ch * 3] = a, part[ch * 3 + 1] = b;
            reinterpret_cast<long long *>(part)[ch * 3 + 2] = c;
        }
    }
    // hand-off: the chunk stores drain, one agent-scope release, then the ticket
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned drawn = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sc[0] = drawn == gridDim.x - 1 ? 1 : 0;
        if (sc[0]) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    const bool last = sc[0] != 0;
    __syncthreads();
    if (!last) return;
    double a = 0.0, b = 0.0;
    long long c = 0;
    for (long long ch = t; ch < n_chunks; ch += MRL_THREADS) {
        a += part[ch * 3], b += part[ch * 3 + 1];
        c += reinterpret_cast<const long long *>(part)[ch * 3 + 2];
    }
    mrl_tree(sa, sb, sc, a, b, c);
    if (t == 0) {
        out[0] = (float)(a / (double)c);      // no row counted: 0 / 0 = NaN
        out[1] = (float)(b / (double)c);
        *count = c;
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ void __launch_bounds__(MRL_THREADS)
k_mrl_backward(MrlIn in, const long long *__restrict__ count, const float *__restrict__ grad, void *__restrict__ dpred) {
    const long long r = (long long)blockIdx.x * MRL_THREADS + threadIdx.x;
    if (r >= in.n_cap) return;
    const long long nv = wfs_valid_rows_nonneg(in.n_cap, in.n_dev), cnt = *count;
    float v = 0.f;
    if (cnt > 0 && r < nv && mrl_counted(in, r)) {
        const double d = (double)ldt(in.pred, r, in.pred_dtype) -
                         (double)ldt(in.target, r * in.n_cols + in.col, in.target_dtype);
        const double s = in.kind == WFS_LOSS_L1 ? (d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : (d == d ? 0.0 : d))) : 2.0 * d;
        v = (float)((double)*grad * s / (double)cnt);
    }
    stt(dpred, r, in.pred_dtype, v);
}

bool mrl_args(const void *pred, int32_t pred_dtype, const void *target, int32_t target_dtype, int32_t n_cols, int32_t col,
              const int32_t *coords, const float *se_mask, int32_t nx, int32_t ny, int64_t n_cap, const int64_t *n_dev,
              int32_t kind, MrlIn *in) {
    if (!wfs_dtype_ok(pred_dtype) || !wfs_dtype_ok(target_dtype) || n_cols < 1 || col < 0 || col >= n_cols) return false;
    if (n_cap < 0 || n_cap >= (1ll << 31) || (kind != WFS_LOSS_L1 && kind != WFS_LOSS_MSE)) return false;
    if (n_cap > 0 && (!pred || !target)) return false;
    if (se_mask && (!coords || nx < 1 || ny < 1)) return false;
    *in = MrlIn{pred, target, coords, se_mask, (const long long *)n_dev, n_cap, pred_dtype, target_dtype, n_cols, col, nx, ny,
                kind};
    return true;
}

// ---- evaluator -------------------------------------------------------------------------------------------------------
struct SegqPlan {
    int nx, ny, n_phys, e_index, psd_index, z_index, t_index, has_pid, pid_int64;
};

__global__ void __launch_bounds__(MB)
k_segq_rows(const int *__restrict__ coords, const void *__restrict__ results, int r_dtype, const void *__restrict__ target,
            int t_dtype, const void *__restrict__ pid, long long n_cap, const long long *__restrict__ n_dev, int E,
            const float *__restrict__ seg, SegqPlan pp, const int *__restrict__ off, float *__restrict__ mae,
            double *__restrict__ error, int *__restrict__ mult, int *__restrict__ se, float *__restrict__ params,
            int *__restrict__ category, int *__restrict__ slot, unsigned long long *__restrict__ slot_max,
            long long *__restrict__ slot_rows, int *__restrict__ flags) {
    __shared__ unsigned long long smax[SEGQ_SLOTS];
    __shared__ int srows[SEGQ_SLOTS];
    if (threadIdx.x < SEGQ_SLOTS) smax[threadIdx.x] = 0ull, srows[threadIdx.x] = 0;
    __syncthreads();
    const long long nv = wfs_valid_rows_nonneg(n_cap, n_dev);
    const long long r = (long long)blockIdx.x * MB + threadIdx.x;
    if (r < n_cap) {
        // a row that is not scored (beyond the valid count or flagged) still gets defined outputs
        int o_mult = 0, o_se = 0, o_cat = -1, o_slot = -1;
        float o_par[4] = {0.f, 0.f, 0.f, 0.f}, o_mae = 0.f;
        double o_err = 0.0;
        if (r < nv) {
            const SegRow h = seg_row(coords, r, nv, off, E, pp.nx, pp.ny, flags);
            if (h.ok) {
                o_mult = (int)(h.last - h.first);
                o_se = seg[h.cell] == 0.5f ? 1 : 0;
                const long long row = r * pp.n_phys;
                o_err = (double)ldt(results, r, r_dtype) - (double)ldt(target, row + pp.t_index, t_dtype);
                o_mae = (float)fabs(o_err);
                o_par[0] = ldt(target, row + pp.e_index, t_dtype);
                o_par[1] = ldt(target, row + pp.psd_index, t_dtype);
                o_par[2] = (float)o_mult;
                o_par[3] = ldt(target, row + pp.z_index, t_dtype);
                if (pp.has_pid) {
                    const int s = pid_slot(ld_pid(pid, pp.pid_int64, r));
                    if (s >= 0 && o_se) o_slot = s, o_cat = pid_slot_class(s);
                } else {
                    o_slot = 0, o_cat = 0;    // the single class "all": every valid row, no single-ended mask
                }
                if (o_slot >= 0) {
                    atomicAdd(&srows[o_slot], 1);
                    atomicMax(&smax[o_slot], (unsigned long long)__double_as_longlong(fabs(o_err)));
                }
            }
        }
        mae[r] = o_mae;
        error[r] = o_err;
        mult[r] = o_mult;
        se[r] = o_se;
        category[r] = o_cat;
        slot[r] = o_slot;
#pragma unroll
        for (int k = 0; k < 4; ++k) params[(long long)k * n_cap + r] = o_par[k];
    }
    __syncthreads();
    if (threadIdx.x < SEGQ_SLOTS && srows[threadIdx.x] > 0) {
        add64(slot_rows + threadIdx.x, srows[threadIdx.x]);
        atomicMax(slot_max + threadIdx.x, smax[threadIdx.x]);
    }
}

// edges double [C, 2]; edges_set int32 [C]; eflags int32 [1]: bit c = class c met a first subset whose max |error| was 0 or
// not finite
__global__ void __launch_bounds__(64)
k_segq_edges(int C, int has_pid, int nb, unsigned long long *__restrict__ slot_max, long long *__restrict__ slot_rows,
             double *__restrict__ edges, int *__restrict__ edges_set, int *__restrict__ eflags) {
    const int c = threadIdx.x;
    if (c < C && !edges_set[c]) {
        for (int s = 0; s < SEGQ_SLOTS; ++s) {
            if ((has_pid ? pid_slot_class(s) : 0) != c || slot_rows[s] <= 0) continue;   // without PID: slot 0, class 0 only
            double first, last;
            if (error_edge_range(__longlong_as_double((long long)slot_max[s]), nb, &first, &last)) {
                edges[2 * c] = first, edges[2 * c + 1] = last;
                edges_set[c] = 1;
            } else {
                atomicOr(eflags, 1 << c);
            }
            break;                            // the first subset that reaches the class decides
        }
    }
    __syncthreads();
    if (threadIdx.x < SEGQ_SLOTS) slot_max[threadIdx.x] = 0ull, slot_rows[threadIdx.x] = 0;
}

__global__ void __launch_bounds__(MB)
k_segq_bins(const void *__restrict__ results, int r_dtype, const void *__restrict__ target, int t_dtype, int n_phys,
            int t_index, const double *__restrict__ error, const int *__restrict__ category, long long n_cap,
            const long long *__restrict__ n_dev, int C, int nb, const double *__restrict__ edges,
            const int *__restrict__ edges_set, long long *__restrict__ hist, long long *__restrict__ hist2d) {
    const long long nv = wfs_valid_rows_nonneg(n_cap, n_dev);
    const long long r = (long long)blockIdx.x * MB + threadIdx.x;
    if (r >= nv) return;
    const int c = category[r];
    if (c < 0 || c >= C || !edges_set[c]) return;
    const int n2 = nb + 2;
    add64(hist + (long long)c * n2 + bin_direct(error[r], edges[2 * c], edges[2 * c + 1], nb), 1);
    const int bx = bin_direct((double)ldt(target, r * n_phys + t_index, t_dtype), 0.0, 1.0, nb);
    const int by = bin_direct((double)ldt(results, r, r_dtype), 0.0, 1.0, nb);
    add64(hist2d + ((long long)c * n2 + bx) * n2 + by, 1);
}

}  // namespace

extern "C" size_t wfs_masked_regression_loss_workspace_bytes(int64_t n_cap) {
    if (n_cap < 0) return 0;
    return (size_t)MRL_HEAD + (size_t)(n_cap > 0 ? wfs_cdiv(n_cap, MRL_CHUNK) : 1) * 3 * sizeof(double);
}

extern "C" int wfs_masked_regression_loss(const void *pred, int32_t pred_dtype, const void *target, int32_t target_dtype,
                                          int32_t n_cols, int32_t col, const int32_t *coords, const float *se_mask,
                                          int32_t nx, int32_t ny, int64_t n_cap, const int64_t *n_dev, int32_t kind,
                                          int32_t max_blocks, void *workspace, size_t workspace_bytes, float *out,
                                          int64_t *count, void *stream) {
    MrlIn in;
    WFS_REQUIRE(mrl_args(pred, pred_dtype, target, target_dtype, n_cols, col, coords, se_mask, nx, ny, n_cap, n_dev, kind,
                         &in),
                WFS_EINVAL, "wfs_masked_regression_loss: dtypes %d / %d, column %d of %d, n_cap = %lld, kind %d, mask %d x %d",
                pred_dtype, target_dtype, col, n_cols, (long long)n_cap, kind, nx, ny);
    WFS_REQUIRE(workspace && out && count && max_blocks >= 0, WFS_EINVAL, "wfs_masked_regression_loss: NULL argument");
    WFS_REQUIRE(workspace_bytes >= wfs_masked_regression_loss_workspace_bytes(n_cap), WFS_EWORKSPACE,
                "wfs_masked_regression_loss: workspace of %zu bytes, %zu needed", workspace_bytes,
                wfs_masked_regression_loss_workspace_bytes(n_cap));
    const long long n_chunks = wfs_cdiv(n_cap, MRL_CHUNK);       // 0 rows: no chunk, the fold writes NaN and count 0
    long long blocks = n_chunks < 1 ? 1 : n_chunks;
    const long long cap = max_blocks > 0 ? max_blocks : MRL_MAX_BLOCKS;
    if (blocks > cap) blocks = cap;
    k_mrl_forward<<<(unsigned)blocks, MRL_THREADS, 0, (hipStream_t)stream>>>(
        in, n_chunks, (unsigned *)workspace, (double *)((char *)workspace + MRL_HEAD), out, (long long *)count);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}

extern "C" int wfs_masked_regression_loss_backward(const void *pred, int32_t pred_dtype, const void *target,
                                                   int32_t target_dtype, int32_t n_cols, int32_t col,
                                                   const int32_t *coords, const float *se_mask, int32_t nx, int32_t ny,
                                                   int64_t n_cap, const int64_t *n_dev, int32_t kind,
                                                   const int64_t *count, const float *grad, void *dpred, void *stream) {
    MrlIn in;
    WFS_REQUIRE(mrl_args(pred, pred_dtype, target, target_dtype, n_cols, col, coords, se_mask, nx, ny, n_cap, n_dev, kind,
                         &in),
                WFS_EINVAL,
                "wfs_masked_regression_loss_backward: dtypes %d / %d, column %d of %d, n_cap = %lld, kind %d, mask %d x %d",
                pred_dtype, target_dtype, col, n_cols, (long long)n_cap, kind, nx, ny);
    WFS_REQUIRE(count && grad && (n_cap == 0 || dpred), WFS_EINVAL, "wfs_masked_regression_loss_backward: NULL argument");
    if (n_cap == 0) return WFS_OK;
    k_mrl_backward<<<(unsigned)wfs_cdiv(n_cap, MRL_THREADS), MRL_THREADS, 0, (hipStream_t)stream>>>(
        in, (const long long *)count, grad, dpred);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}

extern "C" int wfs_error_edges(double max_abs, int32_t n_bins, double *first_last) {
    WFS_REQUIRE(first_last && n_bins >= 1, WFS_EINVAL, "wfs_error_edges: NULL argument or n_bins = %d", n_bins);
    WFS_REQUIRE(error_edge_range(max_abs, n_bins, first_last, first_last + 1), WFS_EINVAL,
                "wfs_error_edges: a largest |error| of %g gives no bins", max_abs);
    return WFS_OK;
}

extern "C" int wfs_segq_row_stats(const int32_t *coords, const void *results, int32_t results_dtype, const void *target,
                                  int32_t target_dtype, int32_t n_phys, const void *pid, int32_t pid_int64, int64_t n_cap,
                                  const int64_t *n_dev, int32_t E, const float *seg_status, int32_t nx, int32_t ny,
                                  int32_t e_index, int32_t psd_index, int32_t z_index, int32_t target_index,
                                  int32_t *offsets, float *mae, double *error, int32_t *multiplicity, int32_t *se,
                                  float *params, int32_t *category, int32_t *slot, int64_t *slot_scratch, int32_t *flags,
                                  void *stream) {
    WFS_REQUIRE(wfs_dtype_ok(results_dtype) && wfs_dtype_ok(target_dtype), WFS_EINVAL,
                "wfs_segq_row_stats: unknown dtype %d / %d", results_dtype, target_dtype);
    WFS_REQUIRE_EVAL_BATCH("wfs_segq_row_stats: E", E, n_cap, nx, ny);
    WFS_REQUIRE(n_phys >= 1 && e_index >= 0 && e_index < n_phys && psd_index >= 0 && psd_index < n_phys && z_index >= 0 &&
                    z_index < n_phys && target_index >= 0 && target_index < n_phys,
                WFS_EINVAL, "wfs_segq_row_stats: column indices %d, %d, %d, %d outside [0, %d)", e_index, psd_index,
                z_index, target_index, n_phys);
    WFS_REQUIRE(seg_status && offsets && slot_scratch && flags && (pid_int64 == 0 || pid_int64 == 1) &&
                    (n_cap == 0 || (coords && results && target && mae && error && multiplicity && se && params &&
                                    category && slot)),
                WFS_EINVAL, "wfs_segq_row_stats: NULL argument");
    if (n_cap == 0) return WFS_OK;
    hipStream_t s = (hipStream_t)stream;
    const unsigned rb = (unsigned)wfs_cdiv(n_cap, MB);
    if (const int rc = launch_eval_offsets(coords, n_cap, (const long long *)n_dev, E, offsets, flags, s)) return rc;
    const SegqPlan pp = {nx, ny, n_phys, e_index, psd_index, z_index, target_index, pid ? 1 : 0, pid_int64};
    k_segq_rows<<<rb, MB, 0, s>>>(coords, results, results_dtype, target, target_dtype, pid, n_cap,
                                  (const long long *)n_dev, E, seg_status, pp, offsets, mae, error, multiplicity, se, params,
                                  category, slot, (unsigned long long *)slot_scratch,
                                  (long long *)slot_scratch + SEGQ_SLOTS, flags);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}

extern "C" int wfs_segq_error_accumulate(const void *results, int32_t results_dtype, const void *target,
                                         int32_t target_dtype, int32_t n_phys, int32_t target_index, const double *error,
                                         const int32_t *category, int64_t n_cap, const int64_t *n_dev, int32_t n_classes,
                                         int32_t has_pid, int32_t n_bins, int64_t *slot_scratch, double *edges,
                                         int32_t *edges_set, int32_t *error_flags, int64_t *error_hist, int64_t *error_2d,
                                         void *stream) {
    WFS_REQUIRE(wfs_dtype_ok(results_dtype) && wfs_dtype_ok(target_dtype), WFS_EINVAL,
                "wfs_segq_error_accumulate: unknown dtype %d / %d", results_dtype, target_dtype);
    WFS_REQUIRE(n_cap >= 0 && n_cap < (1ll << 31) && n_bins >= 1 && n_bins <= (1 << 20) && n_phys >= 1 &&
                    target_index >= 0 && target_index < n_phys &&
                    n_classes == (has_pid ? SEGQ_CLASSES : 1),
                WFS_EINVAL, "wfs_segq_error_accumulate: n_cap = %lld, %d bins, %d classes, column %d of %d",
                (long long)n_cap, n_bins, n_classes, target_index, n_phys);
    WFS_REQUIRE(slot_scratch && edges && edges_set && error_flags && error_hist && error_2d &&
                    (n_cap == 0 || (results && target && error && category)),
                WFS_EINVAL, "wfs_segq_error_accumulate: NULL argument");
    if (n_cap == 0) return WFS_OK;
    hipStream_t s = (hipStream_t)stream;
    k_segq_edges<<<1, 64, 0, s>>>(n_classes, has_pid ? 1 : 0, n_bins, (unsigned long long *)slot_scratch,
                                  (long long *)slot_scratch + SEGQ_SLOTS, edges, edges_set, error_flags);
    WFS_LAUNCH_CHECK();
    k_segq_bins<<<(unsigned)wfs_cdiv(n_cap, MB), MB, 0, s>>>(results, results_dtype, target, target_dtype, n_phys,
                                                             target_index, error, category, n_cap,
                                                             (const long long *)n_dev, n_classes, n_bins, edges, edges_set,
                                                             (long long *)error_hist, (long long *)error_2d);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}
