// 16-bit LDS images of a 32 -> 32 layer's fp32 filter (include/wfsparse.h "filter images"): K * 128 fragments of 16 B,
//   img[k][s][h][col][j] = H(B[16h + 8s + j][col]),  B = W[k] (forward) or W[k]^T (dX),
// byte for byte what conv_mfma.hip's gconv32_bf16_body builds in LDS from W on its own (same wfs_pack2<H> rounding), so a
// block that is handed an image copies it instead of converting the filter again.
#pragma once
#include "wfs_common.h"

struct WfsFilterImageJobs {
    wfs_filter_image_job j[WFS_FILTER_IMAGE_JOBS_MAX];
    int first_block[WFS_FILTER_IMAGE_JOBS_MAX + 1];      // job i owns blocks [first_block[i], first_block[i + 1])
    int n;
};

// fragment u = ((k * 2 + s) * 2 + h) * 32 + col of one image
template <typename H, bool TRANSPOSE_W>
__device__ __forceinline__ uint4 wfs_filter_fragment(const float *__restrict__ W, int u) {
    const int k = u >> 7, s = (u >> 6) & 1, h = (u >> 5) & 1, col = u & 31;
    const int c0 = 16 * h + 8 * s;
    float w[8];
    if (!TRANSPOSE_W) {
#pragma unroll
        for (int j = 0; j < 8; ++j) w[j] = W[((long long)k * 32 + c0 + j) * 32 + col];
    } else {
        const float4 *src = reinterpret_cast<const float4 *>(W + ((long long)k * 32 + col) * 32 + c0);
        const float4 lo = src[0], hi = src[1];
        w[0] = lo.x; w[1] = lo.y; w[2] = lo.z; w[3] = lo.w;
        w[4] = hi.x; w[5] = hi.y; w[6] = hi.z; w[7] = hi.w;
    }
    uint4 v;
    v.x = wfs_pack2<H>(w[0], w[1]);
    v.y = wfs_pack2<H>(w[2], w[3]);
    v.z = wfs_pack2<H>(w[4], w[5]);
    v.w = wfs_pack2<H>(w[6], w[7]);
    return v;
}

// One 256-thread block of a job's image work: block b (0 <= b < K) fills offset b of both images, threads 0 .. 127 the
// forward one, 128 .. 255 the dX one -- one fragment per thread, coalesced 16-byte stores.
__device__ __forceinline__ void wfs_filter_images_block(const wfs_filter_image_job &job, int b) {
    const int t = (int)threadIdx.x, u = b * 128 + (t & 127);
    if (b >= job.K || t >= 256) return;
    uint4 *dst = reinterpret_cast<uint4 *>(t < 128 ? job.img_fwd : job.img_t);
    if (!dst) return;
    if (job.dtype == WFS_F16)
        dst[u] = t < 128 ? wfs_filter_fragment<wfs_f16, false>(job.W, u) : wfs_filter_fragment<wfs_f16, true>(job.W, u);
    else
        dst[u] = t < 128 ? wfs_filter_fragment<wfs_bf16, false>(job.W, u) : wfs_filter_fragment<wfs_bf16, true>(job.W, u);
}
