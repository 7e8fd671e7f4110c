// tcnc.hip -- the multi-channel TemporalConvNet(c0, [c1 .. c_levels], k, dropout) on rows [N][c0][L].
//
// Reference: TemporalWaveformNet builds TemporalConvNet(1, planes, kernel_size, dropout) with planes expanding to
// `expansion_factor` channels and contracting again (src/models/WaveformModels.py:8-45).  Each level i (dilation
// d = 2^i) is the locuslab TemporalBlock (src/models/ConvBlocks.py:114-152):
//
//   h1  = drop(relu(conv1(x)))            conv1: weight-normed Conv1d(cin -> cout, k, dilation d), causal (chomped)
//   h2  = drop(relu(conv2(h1)))           conv2: weight-normed Conv1d(cout -> cout, k, dilation d), causal
//   out = relu(h2 + (cin != cout ? downsample(x) : x))      downsample: Conv1d(cin -> cout, 1)
//
// The single-channel form keeps a whole row in LDS (tcn.hip).  With up to 32 channels a row of 1024 samples is 128 KB
// per activation, so here every launch is a pass over all (row, sample) positions, activations live in HBM as fp32,
// and the filters (at most 32 x 32 x 8 taps) sit in LDS:
//   forward,  per level: k_tcnc_fwd (conv1 + ReLU + dropout), k_tcnc_fwd (conv2 + ReLU + dropout + residual + ReLU)
//   backward, per level: k_tcnc_gate (ReLU / dropout masks of out and h2), k_tcnc_bwd_x (h1's gradient through conv2),
//                        k_tcnc_bwd_x (x's gradient through conv1 plus the residual), k_tcnc_dw (all the level's weight
//                        gradients as per-block partial sums); then ONE k_tcnc_wn_bwd for every convolution of the net.
// The forward keeps r1 = relu(conv1), r2 = relu(conv2) -- BEFORE dropout -- and out of every level (fp32) for the
// backward.  Dropout is a counter-based hash of a 64-bit seed in device memory (wfs_rows.h, with the channel
// in the counter): m(row, conv, channel, t) in {0, 1 / (1 - p)}.  No mask is stored: every pass that needs one -- conv2
// reading h1 = r1 m1, the backward's mask passes, conv2's dW reading h1 -- rebuilds it from the seed.  Weight gradients: each dW block sums a fixed set of positions in a
// fixed order, and the partial sums are added block by block in index order -- no atomics, bit-identical reruns.
#include "wfs_rows.h"

namespace {

constexpr int TB = 256;
constexpr int MAXC = WFS_TCNC_MAX_CHANNELS, MAXK = WFS_TCNC_MAX_K, MAXLV = WFS_TCNC_MAX_LEVELS;
constexpr int CH = 8;                     // output channels per thread of the conv passes
constexpr int DW_TP = 32;                 // positions per staged tile of the dW pass
constexpr int DW_MAXBLK = 1024;           // dW blocks (partial sums per convolution)
constexpr int MAX_GRID = 4096;            // conv passes: grid-stride beyond this many blocks
constexpr int MAXW = MAXC * MAXC * MAXK;  // taps of the largest convolution

// element (row, conv ci = 2 * level + {0, 1}, channel ch, sample t): t < 2^12, ch < 2^5, ci < 2^4
__device__ __forceinline__ float drop_mult(const Drop &d, long long row, int ci, int ch, int t) {
    return wfs_drop_mult(d, ((((unsigned long long)row << 4 | (unsigned)ci) << 5 | (unsigned)ch) << 12) | (unsigned)t);
}

struct FwdArgs {
    const void *X;  // conv input [N][cin][L] (x_dt)
    int x_dt;
    const float *W, *B;  // effective taps [cout][cin][k], bias [cout]
    int cin, cout, k, d, conv;  // conv = 2 * level + {0, 1} (the dropout counter)
    int x_conv;                 // >= 0: X is relu(conv x_conv) before dropout, read as X * m(x_conv); -1: X as it is
    float *H;                   // relu(conv(X)) [N][cout][L], before dropout
    // second convolution of a level only (OUT != NULL): residual and level output
    const void *R;  // the level's input [N][rin][L] (r_dt)
    int r_dt, rin;
    const float *WD, *BD;  // downsample [cout][rin], [cout]; NULL: identity (rin == cout)
    float *OUT;            // relu(H m + residual) [N][cout][L]
    void *Y;               // the same in the rows' dtype (last level), or NULL
    int y_dt;
};

__global__ void __launch_bounds__(TB) k_tcnc_fwd(FwdArgs a, long long N, int L, float drop_p,
                                                 const long long *__restrict__ seed_dev) {
    __shared__ float Ws[MAXW];  // [coutp][cin][k], rows past cout zero
    __shared__ float Bs[MAXC], WDs[MAXC * MAXC], BDs[MAXC];
    const int nch = (a.cout + CH - 1) / CH, coutp = nch * CH, ck = a.cin * a.k;
    for (int i = threadIdx.x; i < coutp * ck; i += TB) Ws[i] = i < a.cout * ck ? a.W[i] : 0.f;
    for (int i = threadIdx.x; i < a.cout; i += TB) Bs[i] = a.B[i];
    if (a.OUT && a.WD) {
        for (int i = threadIdx.x; i < a.cout * a.rin; i += TB) WDs[i] = a.WD[i];
        for (int i = threadIdx.x; i < a.cout; i += TB) BDs[i] = a.BD[i];
    }
    __syncthreads();
    const Drop dr = make_drop(drop_p, seed_dev);
    const long long P = N * L, total = P * nch;
    for (long long g = (long long)blockIdx.x * TB + threadIdx.x; g < total; g += (long long)gridDim.x * TB) {
        const int chunk = (int)(g / P);
        const long long pos = g - chunk * P, n = pos / L;
        const int t = (int)(pos - n * L), co0 = chunk * CH;
        float acc[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) acc[c] = 0.f;
        for (int ci = 0; ci < a.cin; ++ci) {
            const long long base = (n * a.cin + ci) * L;
            for (int j = 0; j < a.k; ++j) {
                const int s = t - (a.k - 1 - j) * a.d;
                float xv = 0.f;
                if (s >= 0) {
                    xv = ldt(a.X, base + s, a.x_dt);
                    if (a.x_conv >= 0) xv *= drop_mult(dr, n, a.x_conv, ci, s);
                }
                const float *w = Ws + (co0 * a.cin + ci) * a.k + j;
#pragma unroll
                for (int c = 0; c < CH; ++c) acc[c] = fmaf(w[c * ck], xv, acc[c]);
            }
        }
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int co = co0 + c;
            if (co >= a.cout) break;
            float v = acc[c] + Bs[co];
            v = v > 0.f ? v : 0.f;
            const long long o = (n * a.cout + co) * L + t;
            a.H[o] = v;
            if (a.OUT) {
                v *= drop_mult(dr, n, a.conv, co, t);
                float r;
                if (a.WD) {
                    r = BDs[co];
                    for (int ci = 0; ci < a.rin; ++ci) r = fmaf(WDs[co * a.rin + ci], ldt(a.R, (n * a.rin + ci) * L + t, a.r_dt), r);
                } else {
                    r = ldt(a.R, o, a.r_dt);
                }
                float y = v + r;
                y = y > 0.f ? y : 0.f;
                a.OUT[o] = y;
                if (a.Y) stt(a.Y, o, a.y_dt, y);
            }
        }
    }
}

// go = G [out > 0];  gz2 = go [r2 > 0] m2   (r2 = relu(z2) before dropout; m2 rebuilt from the seed)
__global__ void __launch_bounds__(TB) k_tcnc_gate(const void *__restrict__ G, int g_dt, const float *__restrict__ OUT,
                                                  const float *__restrict__ R2, float *__restrict__ GO,
                                                  float *__restrict__ GZ2, long long total, int cout, int L, int conv,
                                                  float drop_p, const long long *__restrict__ seed_dev) {
    const Drop dr = make_drop(drop_p, seed_dev);
    for (long long i = (long long)blockIdx.x * TB + threadIdx.x; i < total; i += (long long)gridDim.x * TB) {
        const float go = OUT[i] > 0.f ? ldt(G, i, g_dt) : 0.f;
        GO[i] = go;
        float gz = 0.f;
        if (R2[i] > 0.f) {
            const long long nc = i / L, n = nc / cout;
            gz = go * drop_mult(dr, n, conv, (int)(nc - n * cout), (int)(i - nc * L));
        }
        GZ2[i] = gz;
    }
}

struct BwdXArgs {
    const float *GZ;  // gradient at the conv's pre-activation [N][cout][L]
    const float *W;   // effective taps [cout][cin][k]
    int cin, cout, k, d;
    const float *MASK;  // r = relu(conv mask_conv), the input before dropout: result = [r > 0] m(mask_conv) sum; NULL: none
    int mask_conv;
    const float *GO;  // residual: + (WD ? WD^T GO : GO) ; NULL: none
    const float *WD;  // [cout][cin]
    void *DX;         // [N][cin][L] (dx_dt)
    int dx_dt;
};

// DX[n][ci][s] = sum_co sum_j W[co][ci][j] GZ[n][co][s + (k-1-j) d]  (the transposed causal conv), then the epilogue
__global__ void __launch_bounds__(TB) k_tcnc_bwd_x(BwdXArgs a, long long N, int L, float drop_p,
                                                   const long long *__restrict__ seed_dev) {
    __shared__ float Wt[MAXW];  // [cout][cinp][k], columns past cin zero
    __shared__ float WDs[MAXC * MAXC];
    const int nch = (a.cin + CH - 1) / CH, cinp = nch * CH;
    for (int i = threadIdx.x; i < a.cout * cinp * a.k; i += TB) {
        const int co = i / (cinp * a.k), r = i - co * cinp * a.k, ci = r / a.k, j = r - ci * a.k;
        Wt[i] = ci < a.cin ? a.W[(co * a.cin + ci) * a.k + j] : 0.f;
    }
    if (a.GO && a.WD)
        for (int i = threadIdx.x; i < a.cout * a.cin; i += TB) WDs[i] = a.WD[i];
    __syncthreads();
    const Drop dr = make_drop(drop_p, seed_dev);
    const long long P = N * L, total = P * nch;
    for (long long g = (long long)blockIdx.x * TB + threadIdx.x; g < total; g += (long long)gridDim.x * TB) {
        const int chunk = (int)(g / P);
        const long long pos = g - chunk * P, n = pos / L;
        const int t = (int)(pos - n * L), ci0 = chunk * CH;
        float acc[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) acc[c] = 0.f;
        for (int co = 0; co < a.cout; ++co) {
            const float *gz = a.GZ + (n * a.cout + co) * L;
            for (int j = 0; j < a.k; ++j) {
                const int tt = t + (a.k - 1 - j) * a.d;
                const float gv = tt < L ? gz[tt] : 0.f;
                const float *w = Wt + (co * cinp + ci0) * a.k + j;
#pragma unroll
                for (int c = 0; c < CH; ++c) acc[c] = fmaf(w[c * a.k], gv, acc[c]);
            }
        }
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int ci = ci0 + c;
            if (ci >= a.cin) break;
            const long long o = (n * a.cin + ci) * L + t;
            float v = acc[c];
            if (a.MASK) v = a.MASK[o] > 0.f ? v * drop_mult(dr, n, a.mask_conv, ci, t) : 0.f;
            if (a.GO) {
                if (a.WD) {
                    for (int co = 0; co < a.cout; ++co) v = fmaf(WDs[co * a.cin + ci], a.GO[(n * a.cout + co) * L + t], v);
                } else {
                    v += a.GO[o];
                }
            }
            stt(a.DX, o, a.dx_dt, v);
        }
    }
}

struct DwJob {
    const float *GZ;  // [N][cout][L]
    const void *X;    // the conv's input [N][cin][L] (x_dt)
    int x_dt, cin, cout, k, d;
    int x_conv;   // >= 0: X is relu(conv x_conv) before dropout, read as X * m(x_conv); -1: X as it is
    float *part;  // [nblk][cout][cin * k + 1]: d taps, then d bias
};
struct DwJobs {
    DwJob j[3];
};

// dW[co][ci * k + j] = sum over positions of GZ[co][pos] X[ci][pos - (k-1-j) d];  column cin * k (an input of ones)
// is d bias.  Block b sums tiles b, b + nblk, ...; inside a tile `groups` thread groups take interleaved positions and
// are added in group order at the end.
template <int CO>
__global__ void __launch_bounds__(TB) k_tcnc_dw(DwJobs jobs, long long N, int L, int nblk, float drop_p,
                                                const long long *__restrict__ seed_dev) {
    const DwJob jb = jobs.j[blockIdx.y];
    const Drop dr = make_drop(drop_p, seed_dev);
    if (jb.cout > CO) return;  // (the host picks CO >= every job's cout)
    __shared__ float GZs[CO][DW_TP];
    __shared__ float XS[(MAXC * MAXK + 1) * DW_TP];
    const int ncol = jb.cin * jb.k + 1;
    const int groups = ncol <= TB / 2 ? TB / ncol : 1;
    const long long P = N * L;
    for (int i = threadIdx.x; i < CO * DW_TP; i += TB) (&GZs[0][0])[i] = 0.f;
    float acc[2][CO];
    int col[2], grp[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int s = threadIdx.x + r * TB;
        grp[r] = s / ncol;
        col[r] = s - grp[r] * ncol;
        if (grp[r] >= groups) grp[r] = -1;
#pragma unroll
        for (int c = 0; c < CO; ++c) acc[r][c] = 0.f;
    }
    for (long long tile = blockIdx.x; tile * DW_TP < P; tile += nblk) {
        const long long p0 = tile * DW_TP;
        __syncthreads();
        for (int e = threadIdx.x; e < jb.cout * DW_TP; e += TB) {
            const int co = e / DW_TP, p = e - co * DW_TP;
            const long long pos = p0 + p;
            float v = 0.f;
            if (pos < P) {
                const long long n = pos / L;
                v = jb.GZ[(n * jb.cout + co) * L + (pos - n * L)];
            }
            GZs[co][p] = v;
        }
        for (int e = threadIdx.x; e < ncol * DW_TP; e += TB) {
            const int c = e / DW_TP, p = e - c * DW_TP;
            const long long pos = p0 + p;
            float v = 0.f;
            if (pos < P) {
                if (c == ncol - 1) {
                    v = 1.f;
                } else {
                    const long long n = pos / L;
                    const int t = (int)(pos - n * L), ci = c / jb.k, j = c - ci * jb.k;
                    const int s = t - (jb.k - 1 - j) * jb.d;
                    if (s >= 0) {
                        v = ldt(jb.X, (n * jb.cin + ci) * L + s, jb.x_dt);
                        if (jb.x_conv >= 0) v *= drop_mult(dr, n, jb.x_conv, ci, s);
                    }
                }
            }
            XS[e] = v;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (grp[r] < 0) continue;
            const float *xs = XS + col[r] * DW_TP;
            for (int p = grp[r]; p < DW_TP; p += groups) {
                const float xv = xs[p];
#pragma unroll
                for (int c = 0; c < CO; ++c) acc[r][c] = fmaf(GZs[c][p], xv, acc[r][c]);
            }
        }
    }
    float *out = jb.part + (long long)blockIdx.x * jb.cout * ncol;
    if (groups == 1) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (grp[r] < 0) continue;
#pragma unroll
            for (int c = 0; c < CO; ++c)
                if (c < jb.cout) out[c * ncol + col[r]] = acc[r][c];
        }
        return;
    }
    __syncthreads();  // XS is free: groups x cout x ncol <= 256 x 32 floats
    if (grp[0] >= 0) {
#pragma unroll
        for (int c = 0; c < CO; ++c)
            if (c < jb.cout) XS[(grp[0] * jb.cout + c) * ncol + col[0]] = acc[0][c];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < jb.cout * ncol; e += TB) {
        float v = 0.f;
        for (int gi = 0; gi < groups; ++gi) v += XS[gi * jb.cout * ncol + e];
        out[e] = v;
    }
}

struct ConvDesc {
    int cin, cout, kk, d;
    long long w_off, b_off, p_off;  // into the weights buffer / the partial sums
};
struct ConvTable {
    ConvDesc c[3 * MAXLV];
};

// effective taps of every convolution: w = g v / |v| per output channel (torch.nn.utils.weight_norm, dim 0); the
// downsample has no weight norm (g == 0: w = v).  Block = convolution, thread = output channel.
__global__ void __launch_bounds__(64) k_tcnc_taps(const TcnParamPtrs *__restrict__ pp, ConvTable tab, float *__restrict__ wts) {
    const ConvDesc cd = tab.c[blockIdx.x];
    const TcnParamPtrs p = pp[blockIdx.x];
    const int co = threadIdx.x, n = cd.cin * cd.kk;
    if (co >= cd.cout) return;
    const float *v = p.v + (long long)co * n;
    float scale = 1.f;
    if (p.g) {
        float n2 = 0.f;
        for (int q = 0; q < n; ++q) n2 = fmaf(v[q], v[q], n2);
        scale = p.g[co] / sqrtf(n2);
    }
    for (int q = 0; q < n; ++q) wts[cd.w_off + (long long)co * n + q] = v[q] * scale;
    wts[cd.b_off + co] = p.b ? p.b[co] : 0.f;
}

// block (convolution, output channel): sum the dW blocks' partials in block order, then the weight-norm backward
//   dg = (dw . v) / |v|,   dv = g / |v| (dw - v (dw . v) / |v|^2),   db = the bias column;   downsample: dv = dw.
// In double: dw . v cancels (dg of a wide layer is a small difference of large products), and this is a few hundred
// numbers per block.
__global__ void __launch_bounds__(TB) k_tcnc_wn_bwd(const TcnParamPtrs *__restrict__ pp, ConvTable tab,
                                                    const float *__restrict__ part, int nblk) {
    const ConvDesc cd = tab.c[blockIdx.x];
    const int co = blockIdx.y;
    if (co >= cd.cout) return;
    const TcnParamPtrs p = pp[blockIdx.x];
    const int n = cd.cin * cd.kk, ncol = n + 1;
    __shared__ double dw[MAXC * MAXK + 1];
    __shared__ double red[2][TB];
    const float *q0 = part + cd.p_off + (long long)co * ncol;
    for (int q = threadIdx.x; q < ncol; q += TB) {
        double s = 0.0;
        for (int b = 0; b < nblk; ++b) s += (double)q0[(long long)b * cd.cout * ncol + q];
        dw[q] = s;
    }
    __syncthreads();
    const float *v = p.v + (long long)co * n;
    double dot = 0.0, n2 = 0.0;
    for (int q = threadIdx.x; q < n; q += TB) {
        dot += dw[q] * (double)v[q];
        n2 += (double)v[q] * (double)v[q];
    }
    red[0][threadIdx.x] = dot;
    red[1][threadIdx.x] = n2;
    __syncthreads();
    for (int h = TB / 2; h >= 1; h >>= 1) {
        if (threadIdx.x < h) {
            red[0][threadIdx.x] += red[0][threadIdx.x + h];
            red[1][threadIdx.x] += red[1][threadIdx.x + h];
        }
        __syncthreads();
    }
    dot = red[0][0];
    n2 = red[1][0];
    if (p.g) {
        const double inv = 1.0 / sqrt(n2), g = p.g[co];
        if (p.dv)
            for (int q = threadIdx.x; q < n; q += TB)
                p.dv[(long long)co * n + q] = (float)(g * inv * (dw[q] - (double)v[q] * dot * inv * inv));
        if (p.dg && threadIdx.x == 0) p.dg[co] = (float)(dot * inv);
    } else if (p.dv) {
        for (int q = threadIdx.x; q < n; q += TB) p.dv[(long long)co * n + q] = (float)dw[q];
    }
    if (p.db && threadIdx.x == 0) p.db[co] = (float)dw[n];
}

// the plan: convolutions in parameter order (per level conv1, conv2, then the downsample when cin != cout)
int plan(int32_t c0, const int32_t *channels, int32_t levels, int32_t k, ConvTable *tab, int *n_conv, long long *w_total) {
    WFS_REQUIRE(levels >= 1 && levels <= MAXLV, WFS_EINVAL, "TCN of %d levels: 1 .. %d supported", levels, MAXLV);
    // k = 1 has no causal padding: the torch module's Chomp1d(0) returns an empty tensor, so there is nothing to mirror
    WFS_REQUIRE(k >= 2 && k <= MAXK, WFS_EINVAL, "TCN kernel size %d: 2 .. %d supported", k, MAXK);
    WFS_REQUIRE(channels != nullptr, WFS_EINVAL, "NULL channel list");
    WFS_REQUIRE(c0 >= 1 && c0 <= MAXC, WFS_EINVAL, "TCN input of %d channels: 1 .. %d supported", c0, MAXC);
    int nc = 0;
    long long off = 0;
    for (int lv = 0; lv < levels; ++lv) {
        const int cin = lv == 0 ? c0 : channels[lv - 1], cout = channels[lv], d = 1 << lv;
        WFS_REQUIRE(cout >= 1 && cout <= MAXC, WFS_EINVAL, "TCN level %d has %d channels: 1 .. %d supported", lv, cout, MAXC);
        const int shapes[3][2] = {{cin, k}, {cout, k}, {cin, 1}};
        for (int w = 0; w < (cin != cout ? 3 : 2); ++w) {
            ConvDesc &cd = tab->c[nc++];
            cd.cin = shapes[w][0];
            cd.cout = cout;
            cd.kk = shapes[w][1];
            cd.d = w == 2 ? 0 : d;
            cd.w_off = off;
            off += (long long)cd.cout * cd.cin * cd.kk;
            cd.b_off = off;
            off += cd.cout;
            cd.p_off = 0;
        }
    }
    *n_conv = nc;
    if (w_total) *w_total = off;
    return WFS_OK;
}

unsigned grid_for(long long threads) {
    long long b = (threads + TB - 1) / TB;
    return (unsigned)(b < 1 ? 1 : (b > MAX_GRID ? MAX_GRID : b));
}

int max_channels(int32_t c0, const int32_t *channels, int32_t levels) {
    int m = c0;
    for (int lv = 0; lv < levels; ++lv) m = channels[lv] > m ? channels[lv] : m;
    return m;
}

int check_common(int32_t c0, const int32_t *channels, int32_t levels, int32_t k, int64_t N, int32_t L, int32_t dtype,
                 float dropout_p, const int64_t *seed_dev, ConvTable *tab, int *n_conv, long long *w_total) {
    int rc = plan(c0, channels, levels, k, tab, n_conv, w_total);
    if (rc != WFS_OK) return rc;
    WFS_REQUIRE(L >= 1 && L <= WFS_TCNC_MAX_L, WFS_EINVAL, "row length %d not in [1, %d]", L, WFS_TCNC_MAX_L);
    WFS_REQUIRE(N >= 0 && N <= (1ll << 40) / L, WFS_EINVAL, "%lld rows of %d samples", (long long)N, L);
    WFS_REQUIRE(wfs_dtype_ok(dtype), WFS_EINVAL, "bad dtype %d", dtype);
    WFS_REQUIRE_DROPOUT(dropout_p, seed_dev);
    return WFS_OK;
}

}  // namespace

extern "C" int wfs_tcnc_ok(int32_t c0, const int32_t *channels, int32_t levels, int32_t k, int32_t L, int32_t dtype) {
    ConvTable tab;
    int nc;
    return check_common(c0, channels, levels, k, 1, L, dtype, 0.f, nullptr, &tab, &nc, nullptr);
}

extern "C" size_t wfs_tcnc_weights_floats(int32_t c0, const int32_t *channels, int32_t levels, int32_t k) {
    ConvTable tab;
    int nc;
    long long w = 0;
    if (plan(c0, channels, levels, k, &tab, &nc, &w) != WFS_OK) return 0;
    return (size_t)w;
}

extern "C" int wfs_tcnc_n_conv(int32_t c0, const int32_t *channels, int32_t levels, int32_t k) {
    ConvTable tab;
    int nc = 0;
    if (plan(c0, channels, levels, k, &tab, &nc, nullptr) != WFS_OK) return 0;
    return nc;
}

extern "C" size_t wfs_tcnc_saved_floats(int64_t N, int32_t L, int32_t c0, const int32_t *channels, int32_t levels) {
    ConvTable tab;
    int nc;
    if (plan(c0, channels, levels, 2, &tab, &nc, nullptr) != WFS_OK) return 0;
    size_t s = 0;
    for (int lv = 0; lv < levels; ++lv) s += 3 * (size_t)N * channels[lv] * L;
    return s;
}

extern "C" size_t wfs_tcnc_bwd_workspace_floats(int64_t N, int32_t L, int32_t c0, const int32_t *channels, int32_t levels,
                                                 int32_t k) {
    ConvTable tab;
    int nc;
    if (plan(c0, channels, levels, k, &tab, &nc, nullptr) != WFS_OK) return 0;
    const size_t cm = (size_t)max_channels(c0, channels, levels), nl = (size_t)N * L;
    const int nblk = wfs_dw_blocks((long long)nl, DW_TP, DW_MAXBLK);
    size_t parts = 0;
    for (int c = 0; c < nc; ++c) parts += (size_t)nblk * tab.c[c].cout * (tab.c[c].cin * tab.c[c].kk + 1);
    return 5 * cm * nl + parts;
}

extern "C" int wfs_tcnc_taps_fwd(const void *param_ptrs, int32_t c0, const int32_t *channels, int32_t levels, int32_t k,
                                 float *wts, void *stream_) {
    ConvTable tab;
    int nc;
    int rc = plan(c0, channels, levels, k, &tab, &nc, nullptr);
    if (rc != WFS_OK) return rc;
    WFS_REQUIRE(param_ptrs && wts, WFS_EINVAL, "NULL device pointer");
    k_tcnc_taps<<<dim3(nc), dim3(64), 0, (hipStream_t)stream_>>>((const TcnParamPtrs *)param_ptrs, tab, wts);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}

extern "C" int wfs_tcnc_fwd(const void *X, int64_t N, int32_t L, int32_t c0, const int32_t *channels, int32_t levels,
                            int32_t k, const float *wts, float *saved, void *Y, int32_t dtype, float dropout_p,
                            const int64_t *seed_dev, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    ConvTable tab;
    int nc;
    int rc = check_common(c0, channels, levels, k, N, L, dtype, dropout_p, seed_dev, &tab, &nc, nullptr);
    if (rc != WFS_OK) return rc;
    if (N == 0) return WFS_OK;
    WFS_REQUIRE(X && wts && saved && Y, WFS_EINVAL, "NULL device pointer");
    const long long *seed = (const long long *)seed_dev;
    const long long nl = N * (long long)L;
    const void *xin = X;
    int xdt = dtype, ci = 0;
    float *lv_base = saved;
    for (int lv = 0; lv < levels; ++lv) {
        const ConvDesc &c1 = tab.c[ci], &c2 = tab.c[ci + 1];
        const bool ds = c1.cin != c1.cout;
        const int cout = c1.cout;
        float *H1 = lv_base, *H2 = H1 + cout * nl, *OUT = H2 + cout * nl;
        const unsigned grid = grid_for(nl * ((cout + CH - 1) / CH));
        FwdArgs a = {};
        a.X = xin;
        a.x_dt = xdt;
        a.W = wts + c1.w_off;
        a.B = wts + c1.b_off;
        a.cin = c1.cin;
        a.cout = cout;
        a.k = k;
        a.d = c1.d;
        a.conv = 2 * lv;
        a.x_conv = -1;
        a.H = H1;
        k_tcnc_fwd<<<dim3(grid), dim3(TB), 0, stream>>>(a, N, L, dropout_p, seed);
        WFS_LAUNCH_CHECK();
        FwdArgs b = {};
        b.X = H1;
        b.x_dt = WFS_F32;
        b.W = wts + c2.w_off;
        b.B = wts + c2.b_off;
        b.cin = cout;
        b.cout = cout;
        b.k = k;
        b.d = c2.d;
        b.conv = 2 * lv + 1;
        b.x_conv = 2 * lv;  // conv2 reads h1 = r1 m1
        b.H = H2;
        b.R = xin;
        b.r_dt = xdt;
        b.rin = c1.cin;
        if (ds) {
            b.WD = wts + tab.c[ci + 2].w_off;
            b.BD = wts + tab.c[ci + 2].b_off;
        }
        b.OUT = OUT;
        if (lv == levels - 1) {
            b.Y = Y;
            b.y_dt = dtype;
        }
        k_tcnc_fwd<<<dim3(grid), dim3(TB), 0, stream>>>(b, N, L, dropout_p, seed);
        WFS_LAUNCH_CHECK();
        xin = OUT;
        xdt = WFS_F32;
        ci += ds ? 3 : 2;
        lv_base = OUT + cout * nl;
    }
    return WFS_OK;
}

extern "C" int wfs_tcnc_bwd(const void *X, const void *dY, int64_t N, int32_t L, int32_t c0, const int32_t *channels,
                            int32_t levels, int32_t k, const float *wts, const float *saved, void *dX, float *workspace,
                            const void *param_ptrs, int32_t dtype, float dropout_p, const int64_t *seed_dev,
                            void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    ConvTable tab;
    int nc;
    int rc = check_common(c0, channels, levels, k, N, L, dtype, dropout_p, seed_dev, &tab, &nc, nullptr);
    if (rc != WFS_OK) return rc;
    WFS_REQUIRE(N >= 1, WFS_EINVAL, "the backward needs at least one row (the gradients of an empty batch are zeros)");
    WFS_REQUIRE(X && dY && dX && wts && saved && workspace && param_ptrs, WFS_EINVAL, "NULL device pointer");
    const long long nl = N * (long long)L;
    const int nblk = wfs_dw_blocks(nl, DW_TP, DW_MAXBLK);
    const long long cm = max_channels(c0, channels, levels);
    float *GO = workspace, *GZ2 = GO + cm * nl, *GZ1 = GZ2 + cm * nl, *DXB[2] = {GZ1 + cm * nl, GZ1 + 2 * cm * nl};
    float *part = GZ1 + 3 * cm * nl;
    long long base[MAXLV];  // level offsets inside `saved`
    int cidx[MAXLV];        // first convolution of each level
    {
        long long poff = 0, soff = 0;
        for (int c = 0; c < nc; ++c) {
            tab.c[c].p_off = poff;
            poff += (long long)nblk * tab.c[c].cout * (tab.c[c].cin * tab.c[c].kk + 1);
        }
        int ci = 0;
        for (int lv = 0; lv < levels; ++lv) {
            base[lv] = soff;
            cidx[lv] = ci;
            soff += 3ll * channels[lv] * nl;
            ci += (lv == 0 ? c0 : channels[lv - 1]) != channels[lv] ? 3 : 2;
        }
    }
    const long long *seed = (const long long *)seed_dev;
    const void *G = dY;
    int gdt = dtype;
    for (int lv = levels - 1; lv >= 0; --lv) {
        const ConvDesc &c1 = tab.c[cidx[lv]], &c2 = tab.c[cidx[lv] + 1];
        const bool ds = c1.cin != c1.cout;
        const int cin = c1.cin, cout = c1.cout;
        const float *H1 = saved + base[lv], *H2 = H1 + cout * nl, *OUT = H2 + cout * nl;
        const void *xin = lv == 0 ? X : (const void *)(saved + base[lv - 1] + 2ll * cin * nl);
        const int xdt = lv == 0 ? dtype : WFS_F32;
        k_tcnc_gate<<<dim3(grid_for(cout * nl)), dim3(TB), 0, stream>>>(G, gdt, OUT, H2, GO, GZ2, cout * nl, cout, L,
                                                                        2 * lv + 1, dropout_p, seed);
        WFS_LAUNCH_CHECK();
        BwdXArgs b2 = {};
        b2.GZ = GZ2;
        b2.W = wts + c2.w_off;
        b2.cin = cout;
        b2.cout = cout;
        b2.k = k;
        b2.d = c2.d;
        b2.MASK = H1;
        b2.mask_conv = 2 * lv;
        b2.DX = GZ1;
        b2.dx_dt = WFS_F32;
        k_tcnc_bwd_x<<<dim3(grid_for(nl * ((cout + CH - 1) / CH))), dim3(TB), 0, stream>>>(b2, N, L, dropout_p, seed);
        WFS_LAUNCH_CHECK();
        BwdXArgs b1 = {};
        b1.GZ = GZ1;
        b1.W = wts + c1.w_off;
        b1.cin = cin;
        b1.cout = cout;
        b1.k = k;
        b1.d = c1.d;
        b1.GO = GO;
        b1.WD = ds ? wts + tab.c[cidx[lv] + 2].w_off : nullptr;
        float *dxl = DXB[lv & 1];
        b1.DX = lv == 0 ? dX : (void *)dxl;
        b1.dx_dt = lv == 0 ? dtype : WFS_F32;
        k_tcnc_bwd_x<<<dim3(grid_for(nl * ((cin + CH - 1) / CH))), dim3(TB), 0, stream>>>(b1, N, L, dropout_p, seed);
        WFS_LAUNCH_CHECK();
        DwJobs jobs = {};
        jobs.j[0] = {GZ2, H1, WFS_F32, cout, cout, k, c2.d, 2 * lv, part + c2.p_off};   // h1 = r1 m1
        jobs.j[1] = {GZ1, xin, xdt, cin, cout, k, c1.d, -1, part + c1.p_off};
        if (ds) jobs.j[2] = {GO, xin, xdt, cin, cout, 1, 0, -1, part + tab.c[cidx[lv] + 2].p_off};
        const dim3 grid((unsigned)nblk, ds ? 3u : 2u);
        if (cout <= 8)
            k_tcnc_dw<8><<<grid, dim3(TB), 0, stream>>>(jobs, N, L, nblk, dropout_p, seed);
        else if (cout <= 16)
            k_tcnc_dw<16><<<grid, dim3(TB), 0, stream>>>(jobs, N, L, nblk, dropout_p, seed);
        else
            k_tcnc_dw<32><<<grid, dim3(TB), 0, stream>>>(jobs, N, L, nblk, dropout_p, seed);
        WFS_LAUNCH_CHECK();
        G = dxl;
        gdt = WFS_F32;
    }
    k_tcnc_wn_bwd<<<dim3(nc, MAXC), dim3(TB), 0, stream>>>((const TcnParamPtrs *)param_ptrs, tab, part, nblk);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}
