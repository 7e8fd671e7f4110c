// segquant.hip -- the per-row half of the evaluator of the per-segment regression module (the reference's
// LitSegQuantifier: src/evaluation/SegEvaluator.py with StatsUtils.ErrorAggregator) on the device.  The module's masked
// loss for the training step is in segloss.hip.
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
#include "wfs_rows.h"                         // ldt: rows of a runtime dtype

namespace {

#include "wfs_evoffsets.h"
#include "wfs_segrows.h"
#include "wfs_evalbins.h"

constexpr int MB = WFS_EVOFF_THREADS;
constexpr int SEGQ_SLOTS = 6, SEGQ_CLASSES = 5;

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
