// wfs_rows.h -- what the row-wise waveform front ends (tcn.hip, tcnc.hip, rnn.hip) share: the dropout generator, rows of a
// runtime dtype (ldt / stt, also segquant.hip's and segloss.hip's), the dropout argument check, the dW pass's block count and the TCNs' record of parameter addresses.
#pragma once
#include "wfs_common.h"

// The dropout generator (include/wfsparse.h, "dropout generator"): the multiplier of an element is 0 with probability p,
// else 1 / (1 - p), decided by a splitmix64 finaliser over seed + counter * golden ratio.  The 64-bit seed is drawn by
// the caller from torch's generator into device memory; the COUNTER is unique per element and is each file's own
// (its drop_mult builds it and forwards here).  Nothing is stored: every pass that needs a mask rebuilds it.
struct Drop {
    unsigned long long seed;
    unsigned threshold;  // drop when the hash's high 32 bits are below p * 2^32
    float scale;         // 1 / (1 - p); 1 when dropout is off
    bool on;
};
__device__ __forceinline__ Drop make_drop(float p, const long long *seed_dev) {
    Drop d;
    d.on = p > 0.f && seed_dev != nullptr;
    d.seed = d.on ? (unsigned long long)*seed_dev : 0ull;
    double th = (double)p * 4294967296.0;
    d.threshold = th >= 4294967295.0 ? 0xFFFFFFFFu : (unsigned)th;
    d.scale = d.on ? 1.f / (1.f - p) : 1.f;
    return d;
}
__device__ __forceinline__ float wfs_drop_mult(const Drop &d, unsigned long long ctr) {
    if (!d.on) return 1.f;
    unsigned long long z = d.seed + ctr * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (unsigned)(z >> 32) < d.threshold ? 0.f : d.scale;
}

// rows of any of the three dtypes (the code is uniform across a launch: no divergence)
__device__ __forceinline__ float ldt(const void *p, long long i, int dt) {
    if (dt == WFS_F32) return ((const float *)p)[i];
    if (dt == WFS_BF16) return wfs_ld((const wfs_bf16 *)p + i);
    return wfs_ld((const wfs_f16 *)p + i);
}
__device__ __forceinline__ void stt(void *p, long long i, int dt, float v) {
    if (dt == WFS_F32)
        ((float *)p)[i] = v;
    else if (dt == WFS_BF16)
        wfs_st((wfs_bf16 *)p + i, v);
    else
        wfs_st((wfs_f16 *)p + i, v);
}

// the entry points' dropout arguments: p in [0, 1), and a seed in device memory whenever p > 0
#define WFS_REQUIRE_DROPOUT(p, seed_dev)                                                      \
    WFS_REQUIRE((p) >= 0.f && (p) < 1.f && ((p) == 0.f || (seed_dev)), WFS_EINVAL,            \
                "dropout %g needs 0 <= p < 1 and a seed", (double)(p))

// blocks of a dW pass over P positions in tiles of `tile`: one more than the full tiles, at most `max_blocks`
static inline int wfs_dw_blocks(long long P, int tile, int max_blocks) {
    return (int)(P / tile + 1 < max_blocks ? P / tile + 1 : max_blocks);
}

// one convolution of a TCN (weight_v, weight_g, bias and their gradient slots): device addresses, 0 = absent
struct TcnParamPtrs {
    const float *v, *g, *b;
    float *dv, *dg, *db;
};
