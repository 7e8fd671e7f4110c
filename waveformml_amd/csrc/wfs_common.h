// wfs_common.h -- internal helpers of libwfsparse (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "../../include/wfsparse.h"

#define WFS_WAVE 64

void wfs_set_error(const char *fmt, ...);

#define WFS_HIP_CHECK(expr)                                                                  \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            wfs_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__,   \
                          __LINE__);                                                         \
            return WFS_EHIP;                                                                 \
        }                                                                                    \
    } while (0)

#define WFS_LAUNCH_CHECK() WFS_HIP_CHECK(hipGetLastError())

#define WFS_REQUIRE(cond, code, ...)                                                         \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            wfs_set_error(__VA_ARGS__);                                                      \
            return (code);                                                                   \
        }                                                                                    \
    } while (0)

static inline size_t wfs_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static inline int64_t wfs_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// 16-bit storage helpers (round-to-nearest-even through the hardware cvt; NaN stays NaN).  bf16 rows are plain
// unsigned shorts; fp16 rows get a distinct type so that overloads and templates can tell the two apart.
typedef unsigned short wfs_bf16;
struct wfs_f16 {
    unsigned short bits;
};
__device__ __forceinline__ float wfs_ld(const float *p) { return *p; }
__device__ __forceinline__ float wfs_ld(const wfs_bf16 *p) {
    return __uint_as_float(((unsigned)*p) << 16);
}
__device__ __forceinline__ float wfs_ld(const wfs_f16 *p) {
    return (float)__builtin_bit_cast(_Float16, p->bits);
}
__device__ __forceinline__ void wfs_st(float *p, float v) { *p = v; }
__device__ __forceinline__ void wfs_st(wfs_bf16 *p, float v) {
    __bf16 b = (__bf16)v;
    *p = *reinterpret_cast<unsigned short *>(&b);
}
__device__ __forceinline__ void wfs_st(wfs_f16 *p, float v) {
    p->bits = __builtin_bit_cast(unsigned short, (_Float16)v);
}
// one dword = two neighbouring 16-bit elements (low half first)
template <typename H>
__device__ __forceinline__ void wfs_unpack2(unsigned w, float &lo, float &hi);
template <>
__device__ __forceinline__ void wfs_unpack2<wfs_bf16>(unsigned w, float &lo, float &hi) {
    lo = __uint_as_float(w << 16);
    hi = __uint_as_float(w & 0xFFFF0000u);
}
template <>
__device__ __forceinline__ void wfs_unpack2<wfs_f16>(unsigned w, float &lo, float &hi) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    h2 v = __builtin_bit_cast(h2, w);
    lo = (float)v.x;
    hi = (float)v.y;
}
template <typename H>
__device__ __forceinline__ unsigned wfs_pack2(float lo, float hi);
template <>
__device__ __forceinline__ unsigned wfs_pack2<wfs_bf16>(float lo, float hi) {
    wfs_bf16 a, b;
    wfs_st(&a, lo);
    wfs_st(&b, hi);
    return (unsigned)a | ((unsigned)b << 16);
}
template <>
__device__ __forceinline__ unsigned wfs_pack2<wfs_f16>(float lo, float hi) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    h2 v = {(_Float16)lo, (_Float16)hi};
    return __builtin_bit_cast(unsigned, v);
}
// the value a float takes when it is stored in H and read back
template <typename H>
__device__ __forceinline__ float wfs_round_to(float v) {
    H t;
    wfs_st(&t, v);
    return wfs_ld(&t);
}
static inline bool wfs_dtype_ok(int dtype) { return dtype == WFS_F32 || dtype == WFS_BF16 || dtype == WFS_F16; }
static inline int wfs_dtype_bytes(int dtype) { return dtype == WFS_F32 ? 4 : 2; }
// "no reduction was deferred": what an entry point leaves in *defer before it decides otherwise
static inline wfs_dw_job wfs_dw_job_none() { return wfs_dw_job{}; }

// What a host-side column map (kmap_host[k] = table column used for filter offset k, NULL = none) amounts to.  The fast
// kernels know two maps: the identity, and the SubM mirror k -> K-1-k.  Identity wins where both hold (K == 1).
enum { WFS_KMAP_IDENTITY = 0, WFS_KMAP_MIRROR = 1, WFS_KMAP_OTHER = 2 };
static inline int wfs_kmap_kind(const int32_t *kmap_host, int K) {
    bool is_ident = true, is_mirror = true;
    for (int k = 0; k < K && kmap_host; ++k) {
        is_ident = is_ident && kmap_host[k] == k;
        is_mirror = is_mirror && kmap_host[k] == K - 1 - k;
    }
    return is_ident ? WFS_KMAP_IDENTITY : (is_mirror ? WFS_KMAP_MIRROR : WFS_KMAP_OTHER);
}

// Run-time value -> template argument.  f is a generic lambda that returns the int status, so WFS_REQUIRE and
// WFS_LAUNCH_CHECK work inside it:
//     return wfs_with_dtype(dtype, [&](auto t) -> int {
//         using T = decltype(t);
//         k<T><<<grid, block, 0, stream>>>((const T *)X, ...);
//         WFS_LAUNCH_CHECK();
//         return WFS_OK;
//     });
// wfs_with_dtype: f(float{}) / f(wfs_bf16{}) / f(wfs_f16{}); any code other than WFS_F32 and WFS_BF16 takes the fp16
// branch, so the entry points check wfs_dtype_ok themselves.  wfs_with_h16: the same for 16-bit-only launchers.
template <typename F>
static inline int wfs_with_dtype(int dtype, F &&f) {
    if (dtype == WFS_F32) return f(float{});
    if (dtype == WFS_BF16) return f(wfs_bf16{});
    return f(wfs_f16{});
}
template <typename F>
static inline int wfs_with_h16(int dtype, F &&f) {
    if (dtype == WFS_BF16) return f(wfs_bf16{});
    return f(wfs_f16{});
}
// wfs_with_int<V0, V1, ...>: f(std::integral_constant<int, Vi>{}) for the Vi that equals v; any other v takes the LAST
// listed value (the `default:` of the switch this replaces).  Only the listed values are instantiated.
template <int V0, int... Vs, typename F>
static inline int wfs_with_int(int v, F &&f) {
    if constexpr (sizeof...(Vs) == 0) {
        return f(std::integral_constant<int, V0>{});
    } else {
        if (v == V0) return f(std::integral_constant<int, V0>{});
        return wfs_with_int<Vs...>(v, f);
    }
}

// The rows a kernel works on: the capacity its buffers were sized for, cut down to the device-side count where the
// caller passes one (static shapes under graph capture).  The _nonneg form also holds a negative count at 0.
__device__ __forceinline__ long long wfs_valid_rows(long long cap, const long long *dev) {
    long long v = dev ? *dev : cap;
    return v < cap ? v : cap;
}
__device__ __forceinline__ long long wfs_valid_rows_nonneg(long long cap, const long long *dev) {
    long long v = dev ? *dev : cap;
    v = v < cap ? v : cap;
    return v > 0 ? v : 0;
}

// event timing (opt-in; see wfs_timing_enable)
struct WfsTimerScope {
    int timer;
    hipStream_t stream;
    void *rec;
    WfsTimerScope(int timer, hipStream_t stream);
    ~WfsTimerScope();
};

// shape-specialised launchers (conv_mfma.hip); r_dev: optional device-side count of valid rows (<= R)
bool wfs_mfma_gconv32_ok(int K);
int wfs_launch_gconv32_f32(const int *table, int mirror, int K, int identity_k, long long R, const long long *r_dev,
                           const float *X, const float *W, int transpose_w, const float *bias, float *Y,
                           hipStream_t stream, int packed_kl = 0);
// 16-bit rows (dtype WFS_BF16 or WFS_F16)
int wfs_launch_gconv32_h16(const int *table, int mirror, int K, int identity_k, long long R, const long long *r_dev,
                           const void *X, const float *W, int transpose_w, const float *bias, void *Y, int dtype,
                           hipStream_t stream, int packed_kl = 0, const void *image = nullptr);
int wfs_launch_gconv_c2c32(const int *table, const int *kmap, int K, int identity_k, long long R,
                           const long long *r_dev, const void *X, const float *W, const float *bias, void *Y, int dtype,
                           hipStream_t stream);
// wide layers (wide.hip): dW as dense matrix-core products
bool wfs_wide_dw_ok(int K, long long R, int Cs, int Cg, int dtype);
size_t wfs_wide_dw_workspace(int K, long long R, int Cs, int Cg, int dtype);
int wfs_launch_wide_dw(const int *table, const int *kmap_host, int K, int identity_k, long long R, const long long *r_dev,
                       const void *S, int Cs, const void *G, long long G_rows, int Cg, int swap, float *dW, int dtype,
                       void *workspace, size_t workspace_bytes, hipStream_t stream);
size_t wfs_dw_fast_workspace(int K, long long R, int Cs, int Cg);
int wfs_launch_gdw32(const int *table, int K, int identity_k, long long R, const long long *r_dev, const void *S,
                     const void *G, int swap, float *dW, float *part, int dtype, wfs_dw_job *defer, hipStream_t stream,
                     int packed_kl = 0);
// dW and dX of a 32 -> 32 layer with 16-bit rows in ONE launch (conv_mfma.hip k_bwd32_bf16)
bool wfs_bwd32_fused_ok(int K, int packed_kl, int dtype);
int wfs_launch_bwd32_h16(const int *table, int packed_kl, int K, int identity_k, long long R, const long long *r_dev,
                         const void *S, const void *G, const float *W, void *dX, int swap, float *dW, float *part, int dtype,
                         wfs_dw_job *defer, hipStream_t stream, const void *image_t = nullptr);
int wfs_launch_gdw_c32c2(const int *table, int mirror, int K, int identity_k, long long R, const long long *r_dev,
                         const void *S, const void *G, int swap, float *dW, float *part, int dtype,
                         wfs_dw_job *defer, hipStream_t stream);
int wfs_launch_dw_jobs(const wfs_dw_job *jobs, int n, hipStream_t stream);
// first conv (2 -> 32) + BatchNorm backward without a dz tensor: bn.hip's reduce launch, then conv_mfma.hip's
// k_gdw_bnapply_c32c2, which folds the partials, forms dz in registers and contracts it with the gathered input rows
int wfs_launch_bn_bwd_reduce(const void *X, const void *dY, long long N, int C, const float *gamma, const float *beta,
                             const float *save_mean, const float *save_invstd, int relu, float *partial, int dtype,
                             const long long *n_dev, hipStream_t stream, int *nblk_out);
long long wfs_first_bn_slabs(long long R);
int wfs_launch_first_bn_bwd(const int *table, int mirror, int K, int identity_k, long long R, const long long *r_dev,
                            const void *Z, const void *dY, const void *X, const float *gamma, const float *beta,
                            const float *mean, const float *invstd, int relu, const float *partial, int nblk, float *dW,
                            float *dgamma, float *dbeta, float *part, int dtype, wfs_dw_job *defer, hipStream_t stream);
