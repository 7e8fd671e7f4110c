// optim.hip -- the optimizer update of the PSD training step on ONE flat parameter buffer, in one launch.
//
// The reference builds its optimizer from the config (src/engineering/LitPSD.py:60-76; the examples use
// torch.optim.SGD with momentum 0.98 and nesterov, config/examples/GEP.json:51-69).  torch's single-tensor SGD is four
// elementwise launches (and its "fused" multi-tensor kernel runs a single flat tensor on a handful of blocks); at the
// PSD batch sizes every launch costs ~5 us, so the update is one kernel here.  Same arithmetic, in torch's order
// (torch/optim/sgd.py _single_tensor_sgd):
//     g = grad + weight_decay * p
//     buf = g                                   (first step)      buf = momentum * buf + (1 - dampening) * g
//     g = nesterov ? g + momentum * buf : buf
//     p -= lr * g
#include <string.h>

#include "wfs_common.h"
#include "wfs_evtable.h"
#include "wfs_filterimg.h"

namespace {

__global__ void __launch_bounds__(256) k_sgd_step(float *__restrict__ P, const float *__restrict__ G,
                                                  float *__restrict__ M, long long n, const float *__restrict__ lr_dev,
                                                  float momentum, float dampening, float weight_decay, int nesterov,
                                                  int first_step) {
    const float lr = *lr_dev;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        float p = P[i];
        float g = G[i];
        if (weight_decay != 0.f) g = fmaf(weight_decay, p, g);
        if (M) {
            float b = first_step ? g : fmaf(1.f - dampening, g, M[i] * momentum);
            M[i] = b;
            g = nesterov ? fmaf(momentum, b, g) : b;
        }
        P[i] = fmaf(-lr, g, p);
    }
}

}  // namespace

extern "C" int wfs_sgd_step(float *param, const float *grad, float *momentum_buf, int64_t n, const float *lr_dev,
                            float momentum, float dampening, float weight_decay, int32_t nesterov, int32_t first_step,
                            void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n == 0) return WFS_OK;
    WFS_REQUIRE(param && grad && lr_dev, WFS_EINVAL, "NULL device pointer");
    WFS_REQUIRE(momentum_buf || momentum == 0.f, WFS_EINVAL, "momentum needs a buffer");
    long long blocks = wfs_cdiv(n, 256);
    if (blocks > 2048) blocks = 2048;
    k_sgd_step<<<dim3((unsigned)blocks), dim3(256), 0, stream>>>(param, grad, momentum != 0.f ? momentum_buf : nullptr, n,
                                                                 lr_dev, momentum, dampening, weight_decay, nesterov,
                                                                 first_step);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Adam / AdamW on the same flat buffer.  The config's optimizer_class may name torch.optim.Adam or
// AdamW (LitPSD.configure_optimizers); torch's non-capturable step refuses a graph capture, its capturable one bakes the
// Python-float lr into the graph and costs ~10 elementwise launches.  Arithmetic and order of torch/optim/adam.py
// _single_tensor_adam (capturable=False), element by element in fp32 with the scalars rounded as torch rounds them:
//     g = maximize ? -grad : grad
//     weight_decay != 0:  decoupled ? p *= (float)(1 - lr * wd)  :  g = g + (float)wd * p
//     m = lerp(m, g, (float)(1 - beta1))                       (torch's two-branch lerp)
//     v = v * (float)beta2;  v = v + (float)(1 - beta2) * g * g
//     t = step + 1;  bc1 = 1 - beta1^t;  bc2s = sqrt(1 - beta2^t)          (double, as torch does on the host)
//     vmax = amsgrad ? (vm = maximum(vm, v)) : v
//     p = p + (float)(-lr / bc1) * (m / (sqrt(vmax) / (float)bc2s + (float)eps))
// lr, betas, eps and weight_decay are read from a device block of doubles, so that a scheduler (ExponentialLR,
// OneCycleLR's cycled momentum) reaches a replayed graph.  The step count is a device float, torch's state["step"].
// Two launches: a one-thread prologue reads the step, stores step + 1 and turns t and the doubles into the fp32
// coefficients above (the double pow() runs once, not per block), then the update reads those coefficients beside its
// first rows.  The alternative, one launch whose blocks all read the step and whose LAST block out (an atomic ticket)
// stores step + 1, measured slower (tools/microbench_optim.py, profiles/optim_adam_variants_ab.txt and
// optim_microbench_update.jsonl): C2 (220 k elements) 6.7 us against 5.4, GEP (1.05 M) 17.3 against 7.9.  The
// ticket's cost grows with the blocks that finish together (GEP: 10.5 us at 256 blocks, 17.3 at 1022).
namespace {

struct AdamCoef {
    float decay, wd, w1, omw1, b2, omb2, bc2s, eps, neg_step;
    int has_wd;
};
static_assert(sizeof(AdamCoef) <= WFS_ADAM_COEF_FLOATS * sizeof(float), "coefficient workspace");

__global__ void __launch_bounds__(64) k_adam_prologue(const double *__restrict__ hp, float *__restrict__ step,
                                                      AdamCoef *__restrict__ coef) {
    if (threadIdx.x != 0) return;
    const float t = *step + 1.f;
    *step = t;
    const double lr = hp[0], beta1 = hp[1], beta2 = hp[2], eps = hp[3], wd = hp[4];
    AdamCoef c;
    c.has_wd = wd != 0.0;
    c.decay = (float)(1.0 - lr * wd);
    c.wd = (float)wd;
    c.w1 = (float)(1.0 - beta1);
    c.omw1 = 1.f - c.w1;
    c.b2 = (float)beta2;
    c.omb2 = (float)(1.0 - beta2);
    const double bc1 = 1.0 - pow(beta1, (double)t), bc2 = 1.0 - pow(beta2, (double)t);
    c.bc2s = (float)sqrt(bc2);
    c.eps = (float)eps;
    c.neg_step = (float)(-(lr / bc1));
    *coef = c;
}

template <bool AMS>
__device__ __forceinline__ void adam1(float &p, float g, float &m, float &v, float &vm, const AdamCoef &c, int maximize,
                                      int decoupled) {
    if (maximize) g = -g;
    if (c.has_wd) {
        if (decoupled)
            p = p * c.decay;
        else
            g = g + c.wd * p;
    }
    const float d = g - m;
    m = c.w1 < 0.5f ? m + c.w1 * d : g - d * c.omw1;
    v = v * c.b2;
    v = v + c.omb2 * g * g;
    float den = v;
    if (AMS) {
        vm = (vm > v || vm != vm) ? vm : v;        // torch.maximum: NaN propagates
        den = vm;
    }
    p = p + c.neg_step * (m / (sqrtf(den) / c.bc2s + c.eps));
}

template <bool AMS>
__global__ void __launch_bounds__(256) k_adam_step(float *__restrict__ P, const float *__restrict__ G, float *__restrict__ M,
                                                   float *__restrict__ V, float *__restrict__ VM, long long n, int vec4,
                                                   const AdamCoef *__restrict__ coef, int maximize, int decoupled) {
    const AdamCoef c = *coef;
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x, nth = (long long)gridDim.x * 256;
    long long done = 0;
    if (vec4) {
        // rows of four; every pointer is 16-byte aligned (checked by the caller)
        const long long n4 = n >> 2;
        float4 *P4 = reinterpret_cast<float4 *>(P), *M4 = reinterpret_cast<float4 *>(M);
        float4 *V4 = reinterpret_cast<float4 *>(V), *VM4 = reinterpret_cast<float4 *>(VM);
        const float4 *G4 = reinterpret_cast<const float4 *>(G);
        for (long long i = tid; i < n4; i += nth) {
            float4 p = P4[i], m = M4[i], v = V4[i], vm = AMS ? VM4[i] : float4{0.f, 0.f, 0.f, 0.f};
            const float4 g = G4[i];
            adam1<AMS>(p.x, g.x, m.x, v.x, vm.x, c, maximize, decoupled);
            adam1<AMS>(p.y, g.y, m.y, v.y, vm.y, c, maximize, decoupled);
            adam1<AMS>(p.z, g.z, m.z, v.z, vm.z, c, maximize, decoupled);
            adam1<AMS>(p.w, g.w, m.w, v.w, vm.w, c, maximize, decoupled);
            P4[i] = p;
            M4[i] = m;
            V4[i] = v;
            if (AMS) VM4[i] = vm;
        }
        done = n4 << 2;
    }
    // the scalar tail (at most three elements), or everything when a pointer is not 16-byte aligned
    for (long long i = done + tid; i < n; i += nth) {
        float p = P[i], m = M[i], v = V[i], vm = AMS ? VM[i] : 0.f;
        adam1<AMS>(p, G[i], m, v, vm, c, maximize, decoupled);
        P[i] = p;
        M[i] = m;
        V[i] = v;
        if (AMS) VM[i] = vm;
    }
}

}  // namespace

extern "C" int wfs_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float *max_exp_avg_sq,
                             int64_t n, const double *hyper_dev, float *step_dev, float *coef_dev, int32_t amsgrad,
                             int32_t maximize, int32_t decoupled, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    WFS_REQUIRE(n >= 0, WFS_EINVAL, "negative size");
    WFS_REQUIRE(param && grad && exp_avg && exp_avg_sq && hyper_dev && step_dev && coef_dev, WFS_EINVAL,
                "NULL device pointer");
    WFS_REQUIRE(max_exp_avg_sq || !amsgrad, WFS_EINVAL, "amsgrad needs max_exp_avg_sq");
    WFS_REQUIRE((uintptr_t)coef_dev % 4 == 0, WFS_EINVAL, "unaligned coefficient workspace");
    AdamCoef *coef = reinterpret_cast<AdamCoef *>(coef_dev);
    k_adam_prologue<<<dim3(1), dim3(64), 0, stream>>>(hyper_dev, step_dev, coef);
    WFS_LAUNCH_CHECK();
    if (n == 0) return WFS_OK;                     // the step count still advances, as torch's does
    float *vm = amsgrad ? max_exp_avg_sq : nullptr;
    const bool vec4 = (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq |
                        (uintptr_t)vm) & 15) == 0;
    // at most 512 blocks: C5's 28.7 M elements took 154 us at 512, 166 us at 2048 (profiles/optim_adam_variants_ab.txt)
    long long blocks = wfs_cdiv(vec4 ? wfs_cdiv(n, 4) : n, 256);
    if (blocks > 512) blocks = 512;
    if (amsgrad)
        k_adam_step<true><<<dim3((unsigned)blocks), dim3(256), 0, stream>>>(param, grad, exp_avg, exp_avg_sq, vm, n,
                                                                            vec4 ? 1 : 0, coef, maximize, decoupled);
    else
        k_adam_step<false><<<dim3((unsigned)blocks), dim3(256), 0, stream>>>(param, grad, exp_avg, exp_avg_sq, nullptr, n,
                                                                             vec4 ? 1 : 0, coef, maximize, decoupled);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Hand-over of a batch to a captured step in ONE launch: a replayed HIP graph reads its inputs from fixed buffers, so
// every step starts by copying the batch there -- coordinates, features, labels, the row count -- and the reference's
// forward then permutes the coordinate columns to batch-first (src/models/SPConvNet.py:64).  Five launches (three
// copies, a fill, an index kernel) at ~5 us each become one.
namespace {

struct Perm {
    int v[8];
};

// coords [n, cols] as they are to coords_dst and, columns permuted, to indices_dst (either may be NULL)
__device__ __forceinline__ void load_coords(const int *__restrict__ coords, long long n, int cols, const Perm &perm,
                                            int *__restrict__ coords_dst, int *__restrict__ indices_dst, long long tid,
                                            long long nth) {
    if (cols == 4 && ((reinterpret_cast<uintptr_t>(coords) | reinterpret_cast<uintptr_t>(coords_dst) |
                       reinterpret_cast<uintptr_t>(indices_dst)) & 15) == 0) {
        // the PSD nets' rows (x, y, t, event): one 16-byte row per thread, no division
        const int4 *src = reinterpret_cast<const int4 *>(coords);
        int4 *dst = reinterpret_cast<int4 *>(coords_dst), *idx = reinterpret_cast<int4 *>(indices_dst);
        const int p0 = perm.v[0], p1 = perm.v[1], p2 = perm.v[2], p3 = perm.v[3];
        auto pick = [](const int4 &r, int p) { return p == 0 ? r.x : (p == 1 ? r.y : (p == 2 ? r.z : r.w)); };
        for (long long row = tid; row < n; row += nth) {
            const int4 r = src[row];
            if (dst) dst[row] = r;
            if (idx) idx[row] = int4{pick(r, p0), pick(r, p1), pick(r, p2), pick(r, p3)};
        }
    } else {
        for (long long i = tid; i < n * cols; i += nth) {
            const long long row = i / cols;
            const int col = (int)(i - row * cols);
            if (coords_dst) coords_dst[i] = coords[i];
            if (indices_dst) indices_dst[i] = coords[row * cols + perm.v[col]];
        }
    }
}

__global__ void __launch_bounds__(256) k_load_batch(const int *__restrict__ coords, long long n, int cols, Perm perm,
                                                    int *__restrict__ coords_dst, int *__restrict__ indices_dst,
                                                    const uint4 *__restrict__ feats, uint4 *__restrict__ feats_dst,
                                                    long long feat_words, const unsigned char *__restrict__ feats_tail,
                                                    unsigned char *__restrict__ feats_tail_dst, int tail_bytes,
                                                    const long long *__restrict__ labels, long long *__restrict__ labels_dst,
                                                    long long B, long long *__restrict__ n_valid_dst,
                                                    int *__restrict__ ev_off, int ev_B, int ev_col, int copy_blocks,
                                                    WfsFilterImageJobs images) {
    // blocks past the copy's own count fill filter images (wfs_load_batch_images); the copy keeps its tid / nth
    if ((int)blockIdx.x >= copy_blocks) {
        const int b = (int)blockIdx.x - copy_blocks;
        for (int i = 0; i < images.n; ++i)
            if (b >= images.first_block[i] && b < images.first_block[i + 1])
                wfs_filter_images_block(images.j[i], b - images.first_block[i]);
        return;
    }
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x, nth = (long long)copy_blocks * 256;
    if (tid == 0 && n_valid_dst) *n_valid_dst = n;
    // event offsets of the batch (evrulebook.hip k_event_offsets, same words, same flags): the first WFS_EVENT_FLAG_WORDS
    // blocks walk the batch column of the SOURCE rows -- the captured step then starts with the rulebook build itself
    if (ev_off && blockIdx.x < WFS_EVENT_FLAG_WORDS)
        wfs_event_table_block(coords, n, cols, ev_col, ev_B, ev_off, WFS_EVENT_FLAG_WORDS);
    load_coords(coords, n, cols, perm, coords_dst, indices_dst, tid, nth);
    for (long long i = tid; i < feat_words; i += nth) feats_dst[i] = feats[i];
    for (long long i = tid; i < tail_bytes; i += nth) feats_tail_dst[i] = feats_tail[i];
    for (long long i = tid; i < B; i += nth) labels_dst[i] = labels[i];
}

// Hand-over of a PER-ROW batch (one target row per coordinate row: LitZ, LitEZ, LitSegClassifier, LitSegQuantifier,
// LitWaveform) in one launch.  What differs from k_load_batch: the features are n rows of a [n_cap, row] buffer and
// their source may be a slice of a packed loader buffer (16-byte aligned only at its start: 16-byte lanes when both
// ends are aligned, bytes otherwise); the targets are one row per coordinate row, and every target row in [n, n_cap)
// is filled with the pad element (the criterion's ignore_index, or its float image), so that the padding rows of the
// captured step neither count nor receive a gradient.  E is the target element: unsigned (4 bytes) or unsigned long
// long (8 bytes).
template <typename E>
__global__ void __launch_bounds__(256) k_load_rows_batch(const int *__restrict__ coords, long long n, int cols, Perm perm,
                                                         int *__restrict__ coords_dst, int *__restrict__ indices_dst,
                                                         const unsigned char *__restrict__ feats,
                                                         unsigned char *__restrict__ feats_dst, long long feat_words,
                                                         long long feat_bytes, const E *__restrict__ targets,
                                                         E *__restrict__ targets_dst, long long t_valid, long long t_cap,
                                                         E pad, long long *__restrict__ n_valid_dst,
                                                         int *__restrict__ ev_off, int ev_B, int ev_col, int copy_blocks,
                                                         WfsFilterImageJobs images) {
    if ((int)blockIdx.x >= copy_blocks) {
        const int b = (int)blockIdx.x - copy_blocks;
        for (int i = 0; i < images.n; ++i)
            if (b >= images.first_block[i] && b < images.first_block[i + 1])
                wfs_filter_images_block(images.j[i], b - images.first_block[i]);
        return;
    }
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x, nth = (long long)copy_blocks * 256;
    if (tid == 0 && n_valid_dst) *n_valid_dst = n;
    if (ev_off && blockIdx.x < WFS_EVENT_FLAG_WORDS)
        wfs_event_table_block(coords, n, cols, ev_col, ev_B, ev_off, WFS_EVENT_FLAG_WORDS);
    load_coords(coords, n, cols, perm, coords_dst, indices_dst, tid, nth);
    // features: feat_words 16-byte lanes (0 when an end is misaligned), then the bytes that are left
    const uint4 *f4 = reinterpret_cast<const uint4 *>(feats);
    uint4 *d4 = reinterpret_cast<uint4 *>(feats_dst);
    for (long long i = tid; i < feat_words; i += nth) d4[i] = f4[i];
    for (long long i = feat_words * 16 + tid; i < feat_bytes; i += nth) feats_dst[i] = feats[i];
    // targets: the valid rows' elements, then the pad to the capacity
    for (long long i = tid; i < t_cap; i += nth) targets_dst[i] = i < t_valid ? targets[i] : pad;
}

__global__ void __launch_bounds__(256) k_filter_images(wfs_filter_image_job job) {
    wfs_filter_images_block(job, (int)blockIdx.x);
}

int filter_image_job_ok(const wfs_filter_image_job &j) {
    WFS_REQUIRE(j.K >= 1 && j.K <= 32, WFS_EINVAL, "filter image of K = %d (1 .. 32)", j.K);
    WFS_REQUIRE(j.dtype == WFS_BF16 || j.dtype == WFS_F16, WFS_EINVAL, "filter images are 16-bit (dtype %d)", j.dtype);
    // (the filter may sit anywhere in a flat parameter buffer: 4-byte alignment, as the conv kernels read it)
    WFS_REQUIRE(j.W && ((uintptr_t)j.W & 3) == 0, WFS_EINVAL, "NULL or misaligned filter");
    WFS_REQUIRE((((uintptr_t)j.img_fwd | (uintptr_t)j.img_t) & 15) == 0, WFS_EINVAL, "images must be 16-byte aligned");
    return WFS_OK;
}

// the jobs of a hand-over launch, checked, with the extra blocks each of them owns
int filter_image_jobs(const wfs_filter_image_job *jobs, int njobs, WfsFilterImageJobs &images) {
    WFS_REQUIRE(njobs >= 0 && njobs <= WFS_FILTER_IMAGE_JOBS_MAX && (njobs == 0 || jobs), WFS_EINVAL,
                "%d filter image jobs (0 .. %d)", njobs, WFS_FILTER_IMAGE_JOBS_MAX);
    for (int i = 0; i < njobs; ++i) {
        const int rc = filter_image_job_ok(jobs[i]);
        if (rc != WFS_OK) return rc;
        images.j[i] = jobs[i];
        images.first_block[i + 1] = images.first_block[i] + jobs[i].K;
    }
    images.n = njobs;
    return WFS_OK;
}

}  // namespace

extern "C" size_t wfs_filter_image_bytes(int32_t K) { return K > 0 ? (size_t)K * 2048 : 0; }

extern "C" int wfs_conv_filter_images(const float *W, int32_t K, int32_t dtype, void *img_fwd, void *img_t,
                                      void *stream_) {
    const wfs_filter_image_job job{W, img_fwd, img_t, K, dtype};
    const int rc = filter_image_job_ok(job);
    if (rc != WFS_OK) return rc;
    if (!img_fwd && !img_t) return WFS_OK;
    k_filter_images<<<dim3((unsigned)K), dim3(256), 0, (hipStream_t)stream_>>>(job);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}

extern "C" int wfs_load_batch(const int32_t *coords, int64_t n, int32_t cols, const int32_t *perm_host,
                              int32_t *coords_dst, int32_t *indices_dst, const void *feats, void *feats_dst,
                              int64_t feat_bytes, const int64_t *labels, int64_t *labels_dst, int64_t B,
                              int64_t *n_valid_dst, int32_t *event_offsets, int32_t events, void *stream_) {
    return wfs_load_batch_images(coords, n, cols, perm_host, coords_dst, indices_dst, feats, feats_dst, feat_bytes, labels,
                                 labels_dst, B, n_valid_dst, event_offsets, events, nullptr, 0, stream_);
}

extern "C" int wfs_load_batch_images(const int32_t *coords, int64_t n, int32_t cols, const int32_t *perm_host,
                                     int32_t *coords_dst, int32_t *indices_dst, const void *feats, void *feats_dst,
                                     int64_t feat_bytes, const int64_t *labels, int64_t *labels_dst, int64_t B,
                                     int64_t *n_valid_dst, int32_t *event_offsets, int32_t events,
                                     const wfs_filter_image_job *jobs, int32_t njobs, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    WfsFilterImageJobs images = {};
    const int jrc = filter_image_jobs(jobs, njobs, images);
    if (jrc != WFS_OK) return jrc;
    WFS_REQUIRE(cols >= 1 && cols <= 8, WFS_EINVAL, "bad coordinate width %d", cols);
    WFS_REQUIRE(n >= 0 && B >= 0 && feat_bytes >= 0, WFS_EINVAL, "negative size");
    WFS_REQUIRE((n == 0 || coords) && (feat_bytes == 0 || (feats && feats_dst)) && (B == 0 || (labels && labels_dst)),
                WFS_EINVAL, "NULL device pointer");
    Perm pm;
    for (int c = 0; c < 8; ++c) {
        pm.v[c] = (perm_host && c < cols) ? perm_host[c] : c;
        WFS_REQUIRE(pm.v[c] >= 0 && pm.v[c] < (c < cols ? cols : 8), WFS_EINVAL, "bad column permutation");
    }
    const bool aligned = ((uintptr_t)feats % 16 == 0) && ((uintptr_t)feats_dst % 16 == 0);
    const long long words = aligned ? feat_bytes / 16 : 0;
    const int tail = (int)(feat_bytes - words * 16 > (1 << 30) ? 0 : feat_bytes - words * 16);
    WFS_REQUIRE(aligned || feat_bytes < (1 << 30), WFS_EINVAL, "unaligned feature buffers");
    long long work = n * cols > words ? n * cols : words;
    long long blocks = wfs_cdiv(work > 0 ? work : 1, 256);
    if (blocks > 1024) blocks = 1024;
    WFS_REQUIRE(!event_offsets || events >= 1, WFS_EINVAL, "event offsets of %d events", events);
    if (event_offsets && blocks < WFS_EVENT_FLAG_WORDS) blocks = WFS_EVENT_FLAG_WORDS;
    k_load_batch<<<dim3((unsigned)(blocks + images.first_block[njobs])), dim3(256), 0, stream>>>(
        coords, n, cols, pm, coords_dst, indices_dst, (const uint4 *)feats, (uint4 *)feats_dst, words,
        (const unsigned char *)feats + words * 16, (unsigned char *)feats_dst + words * 16, tail, (const long long *)labels,
        (long long *)labels_dst, B, (long long *)n_valid_dst, event_offsets, events, pm.v[0], (int)blocks, images);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}

extern "C" int wfs_load_rows_batch(const int32_t *coords, int64_t n, int64_t n_cap, int32_t cols, const int32_t *perm_host,
                                   int32_t *coords_dst, int32_t *indices_dst, const void *feats, void *feats_dst,
                                   int64_t row_bytes, const void *targets, void *targets_dst, int64_t target_row_bytes,
                                   int32_t elem, const void *pad_host, int64_t *n_valid_dst, int32_t *event_offsets,
                                   int32_t events, const wfs_filter_image_job *jobs, int32_t njobs, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    WfsFilterImageJobs images = {};
    const int jrc = filter_image_jobs(jobs, njobs, images);
    if (jrc != WFS_OK) return jrc;
    WFS_REQUIRE(cols >= 1 && cols <= 8, WFS_EINVAL, "bad coordinate width %d", cols);
    WFS_REQUIRE(n >= 0 && n_cap >= 0 && row_bytes >= 0 && target_row_bytes >= 0, WFS_EINVAL, "negative size");
    WFS_REQUIRE(n <= n_cap, WFS_EINVAL, "%lld rows, the buffers hold %lld", (long long)n, (long long)n_cap);
    WFS_REQUIRE(n_cap < (1ll << 31) && row_bytes < (1ll << 31) && target_row_bytes < (1ll << 31), WFS_EINVAL,
                "rows or row sizes beyond 2^31");
    WFS_REQUIRE(elem == 4 || elem == 8, WFS_EINVAL, "target elements of %d bytes (4 or 8)", elem);
    WFS_REQUIRE(target_row_bytes % elem == 0, WFS_EINVAL, "target rows of %lld bytes are no multiple of the %d-byte element",
                (long long)target_row_bytes, elem);
    WFS_REQUIRE(n == 0 || coords, WFS_EINVAL, "NULL coordinates");
    WFS_REQUIRE(n * row_bytes == 0 || (feats && feats_dst), WFS_EINVAL, "NULL feature pointer with %lld bytes to copy",
                (long long)(n * row_bytes));
    WFS_REQUIRE(n_cap * target_row_bytes == 0 || (targets_dst && pad_host), WFS_EINVAL,
                "NULL target destination or pad with %lld bytes to write", (long long)(n_cap * target_row_bytes));
    WFS_REQUIRE(n * target_row_bytes == 0 || targets, WFS_EINVAL, "NULL targets");
    WFS_REQUIRE((((uintptr_t)targets | (uintptr_t)targets_dst) & (uintptr_t)(elem - 1)) == 0, WFS_EINVAL,
                "targets are not aligned to their %d-byte element", elem);
    WFS_REQUIRE((((uintptr_t)coords | (uintptr_t)coords_dst | (uintptr_t)indices_dst) & 3) == 0, WFS_EINVAL,
                "coordinates are not 4-byte aligned");
    Perm pm;
    for (int c = 0; c < 8; ++c) {
        pm.v[c] = (perm_host && c < cols) ? perm_host[c] : c;
        WFS_REQUIRE(pm.v[c] >= 0 && pm.v[c] < (c < cols ? cols : 8), WFS_EINVAL, "bad column permutation");
    }
    WFS_REQUIRE(!event_offsets || events >= 1, WFS_EINVAL, "event offsets of %d events", events);
    const long long feat_bytes = n * row_bytes;
    const bool aligned = ((uintptr_t)feats % 16 == 0) && ((uintptr_t)feats_dst % 16 == 0);
    const long long words = aligned ? feat_bytes / 16 : 0;
    const long long t_valid = n * target_row_bytes / elem, t_cap = n_cap * target_row_bytes / elem;
    long long work = n * cols > words ? n * cols : words;
    if (feat_bytes - words * 16 > work) work = feat_bytes - words * 16;
    if (t_cap > work) work = t_cap;
    long long blocks = wfs_cdiv(work > 0 ? work : 1, 256);
    if (blocks > 1024) blocks = 1024;
    if (event_offsets && blocks < WFS_EVENT_FLAG_WORDS) blocks = WFS_EVENT_FLAG_WORDS;
    const dim3 grid((unsigned)(blocks + images.first_block[njobs]));
    unsigned long long pad = 0;
    if (pad_host) memcpy(&pad, pad_host, 8);
    if (elem == 8)
        k_load_rows_batch<unsigned long long><<<grid, dim3(256), 0, stream>>>(
            coords, n, cols, pm, coords_dst, indices_dst, (const unsigned char *)feats, (unsigned char *)feats_dst, words,
            feat_bytes, (const unsigned long long *)targets, (unsigned long long *)targets_dst, t_valid, t_cap, pad,
            (long long *)n_valid_dst, event_offsets, events, pm.v[0], (int)blocks, images);
    else
        k_load_rows_batch<unsigned><<<grid, dim3(256), 0, stream>>>(
            coords, n, cols, pm, coords_dst, indices_dst, (const unsigned char *)feats, (unsigned char *)feats_dst, words,
            feat_bytes, (const unsigned *)targets, (unsigned *)targets_dst, t_valid, t_cap, (unsigned)pad,
            (long long *)n_valid_dst, event_offsets, events, pm.v[0], (int)blocks, images);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}
