// classmetrics.hip -- the classification metrics of the reference's LitPSD / LitSegClassifier validation and test steps on
// the device: torchmetrics' Accuracy and ConfusionMatrix(num_classes = n_type) summed over the batches, the cross-entropy
// mean, and the 100 binary confusion matrices of its ROCCurve (src/evaluation/ROCCurve.py) for EVERY class, all from one
// read of each logit row.
//
//   k_class_metrics  ONE launch, one lane per row, grid-stride over passes of CM_THREADS rows per workgroup.  Per counted
//                    row (below the valid count, label not ignore_index):
//                      pred  = first index of the largest logit (strict >, so a tie goes to the lower index);
//                      p_k   = exp(x_k - m) / sum_j exp(x_j - m) in fp64 from the stored logits, rounded once to fp32;
//                      b_k   = #{i : p_k >= thr[i]} by bisection in the ascending threshold table (LDS);
//                      nll   = m + log(sum_j exp(x_j - m)) - x_label in fp64, into the tables as round(nll * 2^32).
//                    Every workgroup keeps an int32 image of the head counters, the confusion cells and the ROC cells in
//                    LDS (integer LDS atomics; the loss sum a 64-bit one) and flushes its non-zero cells once, with
//                    64-bit integer global atomics.  No floating-point atomic and nothing that depends on the order of
//                    the rows: the tables repeat bit for bit and do not depend on the grid.
//
// C <= CM_REG classes stay in registers (the row is read once: CR = 2, 4 or 8 slots, unrolled, the slots past C guarded
// out); above that the row is read three times (maximum, sum, probabilities) out of L1 / L2 -- a private array of up to
// 32 values indexed by a run-time count would live in scratch memory.
//
// Loads are element loads: the base needs only element alignment and the row stride may exceed C, so a view that starts
// at an odd 16-bit element is read as it lies.  With one lane per row and C * 2 .. C * 4 bytes per row, neighbouring lanes
// read neighbouring rows; a 16-byte lane would need C a multiple of 4 (fp32) or 8 (16-bit), which neither caller has
// (C = 2, C = 5).
//
// A row that is not counted is SELECTED out: beyond the valid count nothing of it is loaded, so a NaN or the captured
// step's padding there cannot reach a table.  A flagged row (flags below) is left out of every table.
#include "wfs_common.h"

namespace {

#include "wfs_evalbins.h"                     // add64
#include "wfs_segtables.h"                    // real_image (fp64), add_fixed

constexpr int CM_THREADS = 256;               // rows per workgroup pass
#ifndef CM_PASSES
#define CM_PASSES 1                           // passes per workgroup that the launch's own block count aims at; 2: timing variant
#endif
constexpr int CM_BLOCKS = 256;                // the launch's own block count at most (one per CU)
constexpr int CM_REG = 8;                     // classes held in registers at most
constexpr int CM_CLASSES = 32;                // WFS_CLASS_METRICS_MAX_CLASSES
constexpr int CM_THRESH = 1024;               // WFS_CLASS_METRICS_MAX_THRESH
constexpr int CM_HEAD = 5;                    // table head: rows counted, rows correct, loss rows, loss sum, rows ignored
constexpr int CM_LDS_HEAD = 6;                // image head: counted, correct, loss rows, ignored, then the 64-bit loss sum
constexpr int CM_LDS_WORDS = 16384;           // 64 KB: head + cells + thresholds must fit (WFS_CLASS_METRICS_LDS_BYTES)
constexpr int CM_NONFINITE = 1, CM_LABEL = 2, CM_LOSS = 4;

struct CmIn {
    const void *logits;
    const long long *labels, *n_dev;
    const unsigned char *mask;                // NULL: every counted row enters the loss
    const float *thr;
    long long stride, N, ignore;
    int C, T;
};

static inline long long cm_cells(int C, int T) { return (long long)C * C + 2ll * C * (T + 1); }
static inline bool cm_fits(int C, int T) {
    return C >= 2 && C <= CM_CLASSES && T >= 1 && T <= CM_THRESH && CM_LDS_HEAD + cm_cells(C, T) + T <= CM_LDS_WORDS;
}

// CR > 0: the row's C <= CR logits in registers; CR == 0: the row is read again for every pass
template <typename T, int CR>
__global__ void __launch_bounds__(CM_THREADS)
k_class_metrics(CmIn in, long long *__restrict__ tab, int *__restrict__ flags) {
    extern __shared__ __attribute__((aligned(16))) int image[];   // [CM_LDS_HEAD | C * C | C * 2 * (T + 1) | float thr[T]]
    const int C = in.C, nT = in.T, cells = C * C + 2 * C * (nT + 1);
    int *conf = image + CM_LDS_HEAD, *roc = conf + C * C;
    float *thr = reinterpret_cast<float *>(roc + 2 * C * (nT + 1));
    for (int k = threadIdx.x; k < CM_LDS_HEAD + cells; k += CM_THREADS) image[k] = 0;
    for (int k = threadIdx.x; k < nT; k += CM_THREADS) thr[k] = in.thr[k];
    __syncthreads();
    const long long nv = wfs_valid_rows_nonneg(in.N, in.n_dev);
    for (long long base = (long long)blockIdx.x * CM_THREADS; base < nv; base += (long long)gridDim.x * CM_THREADS) {
        const long long r = base + threadIdx.x;
        if (r >= nv) break;
        const long long lab = in.labels[r];
        if (lab == in.ignore) {
            atomicAdd(image + 3, 1);
            continue;
        }
        if (lab < 0 || lab >= C) {
            atomicOr(flags, CM_LABEL);
            continue;
        }
        const T *row = (const T *)in.logits + r * in.stride;
        float x[CR > 0 ? CR : 1];
        if constexpr (CR > 0) {
#pragma unroll
            for (int k = 0; k < CR; ++k) x[k] = k < C ? wfs_ld(row + k) : 0.f;
        }
#define CM_X(k) (CR > 0 ? x[CR > 0 ? (k) : 0] : wfs_ld(row + (k)))
        // maximum, its first index, the label's logit; the loops of the register arm are unrolled, so x[] stays in registers
        float m = 0.f, xl = 0.f;
        int pred = 0;
        bool finite = true;
#define CM_LOOP(k, ...)                                       \
    if constexpr (CR > 0) {                                   \
        _Pragma("unroll") for (int k = 0; k < CR; ++k) {      \
            if (k < C) __VA_ARGS__                            \
        }                                                     \
    } else {                                                  \
        for (int k = 0; k < C; ++k) __VA_ARGS__               \
    }
        CM_LOOP(k, {
            const float v = CM_X(k);
            finite = finite && fabsf(v) <= 3.402823466e+38f;  // false for NaN and +-Inf
            if (k == 0 || v > m) m = v, pred = k;
            if (k == lab) xl = v;
        })
        if (!finite) {
            atomicOr(flags, CM_NONFINITE);
            continue;
        }
        double e[CR > 0 ? CR : 1], s = 0.0;
        CM_LOOP(k, {
            const double ek = exp((double)CM_X(k) - (double)m);
            if constexpr (CR > 0) e[k] = ek;
            s += ek;
        })
        const bool in_loss = !in.mask || in.mask[r] != 0;
        long long v = 0;
        if (in_loss) {
            const double nll = ((double)m + log(s)) - (double)xl;
            if (!real_image(nll, &v, flags, CM_LOSS)) continue;
        }
        atomicAdd(image + 0, 1);
        if (pred == lab) atomicAdd(image + 1, 1);
        if (in_loss) {
            atomicAdd(image + 2, 1);
            if (v != 0) atomicAdd(reinterpret_cast<unsigned long long *>(image + 4), (unsigned long long)v);
        }
        atomicAdd(conf + (int)lab * C + pred, 1);
        CM_LOOP(k, {
            double ek;
            if constexpr (CR > 0) ek = e[k]; else ek = exp((double)CM_X(k) - (double)m);
            const float p = (float)(ek / s);
            int lo = 0, hi = nT;              // #{i : thr[i] <= p} of the ascending table
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (thr[mid] <= p) lo = mid + 1; else hi = mid;
            }
            atomicAdd(roc + (k * 2 + (k == lab ? 1 : 0)) * (nT + 1) + lo, 1);
        })
#undef CM_LOOP
#undef CM_X
    }
    __syncthreads();
    // the image's cells lie in table order behind the head
    for (int k = threadIdx.x; k < cells; k += CM_THREADS) {
        const int c = conf[k];
        if (c != 0) add64(tab + CM_HEAD + k, c);
    }
    if (threadIdx.x == 0) {
        if (image[0]) add64(tab + 0, image[0]);
        if (image[1]) add64(tab + 1, image[1]);
        if (image[2]) add64(tab + 2, image[2]);
        const long long sum = *reinterpret_cast<const long long *>(image + 4);
        if (sum != 0) add_fixed(tab + 3, sum, flags, CM_LOSS);
        if (image[3]) add64(tab + 4, image[3]);
    }
}

}  // namespace

extern "C" size_t wfs_class_metrics_table_ints(int32_t C, int32_t T) {
    return cm_fits(C, T) ? (size_t)(CM_HEAD + cm_cells(C, T)) : 0;
}

extern "C" int wfs_class_metrics_accumulate(const void *logits, int32_t dtype, int64_t row_stride, const int64_t *labels,
                                            int64_t ignore_index, const uint8_t *loss_mask, int64_t N,
                                            const int64_t *n_dev, int32_t C, const float *thresholds, int32_t T,
                                            int64_t *tables, int32_t *flags, int32_t max_blocks, void *stream) {
    WFS_REQUIRE(wfs_dtype_ok(dtype), WFS_EINVAL, "wfs_class_metrics_accumulate: unknown dtype %d", dtype);
    WFS_REQUIRE(cm_fits(C, T), WFS_EINVAL,
                "wfs_class_metrics_accumulate: %d classes (2 .. %d), %d thresholds (1 .. %d), and head + C * C + "
                "2 * C * (T + 1) + T = %lld words of LDS (at most %d)",
                C, CM_CLASSES, T, CM_THRESH, (long long)CM_LDS_HEAD + cm_cells(C, T) + T, CM_LDS_WORDS);
    WFS_REQUIRE(N >= 0 && N < (1ll << 31) && row_stride >= C && row_stride < (1ll << 31) && max_blocks >= 0, WFS_EINVAL,
                "wfs_class_metrics_accumulate: N = %lld, row stride %lld (at least C = %d), max_blocks = %d", (long long)N,
                (long long)row_stride, C, max_blocks);
    WFS_REQUIRE(thresholds && tables && flags && (N == 0 || (logits && labels)), WFS_EINVAL,
                "wfs_class_metrics_accumulate: NULL argument");
    if (N == 0) return WFS_OK;
    long long blocks = wfs_cdiv(N, (long long)CM_THREADS * CM_PASSES);
    const long long cap = max_blocks > 0 ? max_blocks : CM_BLOCKS;
    if (blocks > cap) blocks = cap;
    const CmIn in = {logits, (const long long *)labels, (const long long *)n_dev, loss_mask, thresholds, row_stride, N,
                     ignore_index, C, T};
    const size_t lds = (size_t)(CM_LDS_HEAD + cm_cells(C, T) + T) * sizeof(int);
    const int slots = C <= 2 ? 2 : C <= 4 ? 4 : C <= CM_REG ? CM_REG : 0;
    return wfs_with_dtype(dtype, [&](auto t) -> int {
        using TYPE = decltype(t);
        return wfs_with_int<2, 4, CM_REG, 0>(slots, [&](auto cr) -> int {
            k_class_metrics<TYPE, decltype(cr)::value><<<(unsigned)blocks, CM_THREADS, lds, (hipStream_t)stream>>>(
                in, (long long *)tables, flags);
            WFS_LAUNCH_CHECK();
            return WFS_OK;
        });
    });
}
