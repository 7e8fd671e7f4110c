// conv1d.hip -- the dense stack  n x (Conv1d(stride, zero padding, bias) -> BatchNorm1d -> ReLU)  on rows [N][c0][L].
//
// Reference: Conv1DNet (src/models/ConvBlocks.py:176-217), the front end of ConvWaveformNet
// (src/models/WaveformModels.py:108-146): per layer nn.Conv1d(cin, cout, fs, stride = st, padding = pd), nn.BatchNorm1d
// (cout), nn.ReLU.  With z = conv(a_prev) + b, xhat = (z - mean) * invstd, y = gamma * xhat + beta, a = max(0, y):
//
//   forward   one launch per layer + one: launch i folds layer i-1's statistics partials (every block, fixed order),
//             applies BN + ReLU to z_{i-1} ON LOAD, convolves, writes the pre-BN z_i (fp32, kept for the backward) and
//             this layer's per-block partial sums; the last launch normalises z_last into Y.  The block (0, 0) of the
//             launch that folds a layer publishes its mean / invstd (for the backward) and updates running_mean,
//             running_var (unbiased, momentum) and num_batches_tracked on the device.
//   backward  one launch for g_last = dY [y_last > 0] and its partial sums (sum g, sum g xhat), then one launch per
//             layer i = last .. 0 that folds layer i's sums (publishing dgamma_i, dbeta_i), forms
//             dz_i = gamma invstd (g - sum g / M - xhat sum(g xhat) / M) on the fly, and whose blocks take one of two
//             roles: the transposed conv da_{i-1} = conv^T(dz_i) with the ReLU mask of layer i-1 recomputed from
//             z_{i-1} and layer i-1's partial sums; or the per-block partial sums of dW_i and db_i.  One last launch
//             adds all dW / db partials in block order into the gradient slots.  layers + 2 launches.
//
// Statistics: per channel over n_valid x L_out elements, n_valid read from DEVICE memory (NULL: all N rows).  Rows at
// or beyond n_valid are never read: they add nothing to any sum, get z = 0, Y = 0 and dX = 0.  The sums (z, z^2) and
// (g, g xhat) are accumulated, reduced and folded in DOUBLE: E[z^2] - E[z]^2 then keeps ~1e-16 (mean^2 / var) instead
// of the 1e-7 (mean^2 / var) that misses an fp32 bar of 1e-5 once a channel's mean is a few times its deviation, with
// no shift value that every block would have to agree on before the first z exists; the fp64 adds are 2 per output
// against cin x fs fp32 FMAs.  Every sum has a fixed order (lane tree, wave order, block order): no atomics,
// bit-identical reruns.
//
// Work per launch (layer cin -> cout, P = N L_out positions): 2 P cout cin fs flops against 4 P (cin st + cout) bytes
// of fp32 activations -- at the committed plan's widest layer (8 -> 16, fs 4) 1024 flops per 96 bytes, ~10 flop / byte,
// with at most 64 x 64 products per position: too thin and too ragged (cin = 1 .. 16, fs = 2 .. 5) for 16 x 16 x 16
// MFMA tiles, so this is VALU work with the layer's taps in LDS, as tcnc.hip.
#include "wfs_rows.h"

namespace {

constexpr int TB = 256;
constexpr int MAXC = WFS_CONV1D_MAX_CHANNELS, MAXK = WFS_CONV1D_MAX_K, MAXS = WFS_CONV1D_MAX_STRIDE;
constexpr int MAXLY = WFS_CONV1D_MAX_LAYERS, MAXL = WFS_CONV1D_MAX_L;
constexpr int CH = 8;               // channels per thread of the conv passes (a block serves one chunk of CH)
constexpr int ST_MAXBLK = 512;      // position blocks of a conv pass = statistics partials per layer
constexpr int DW_TP = 32;           // positions per staged tile of the dW role
constexpr int DW_MAXBLK = 256;      // dW blocks per column chunk (partial sums per layer)
constexpr int EW_MAXBLK = 2048;     // blocks of the elementwise last forward launch
static_assert(CH * MAXC * MAXK == TB * DW_TP, "the taps of one chunk and the dW tile share one LDS buffer");

// one layer's record of the device pointer table (psd/_fused.py: 7 parameter addresses, then 7 gradient addresses)
struct Conv1dPtrs {
    const float *w, *b, *ga, *be;
    float *rm, *rv;
    long long *nbt;
    float *dw, *db, *dga, *dbe;
    void *unused[3];
};
static_assert(sizeof(Conv1dPtrs) == 14 * sizeof(void *), "pointer record layout");

struct Layer {
    int cin, cout, fs, st, pd, lin, lout;
};
struct Plan {
    Layer ly[MAXLY];
    int n;
};

// The dW role's arithmetic on a chunk of columns, and the accumulator width of a layer.  k_c1d_bwd, its launch and
// wfs_conv1d_arms (which tells the tests what arm a plan reaches) all take them from here.
__host__ __device__ inline int dw_mycols(int ncol, int col0) { return ncol - col0 < TB ? ncol - col0 : TB; }
__host__ __device__ inline int dw_groups(int mycols) { return mycols <= TB / 2 ? TB / mycols : 1; }
inline int dw_co(int cout) { return cout <= 8 ? 8 : (cout <= 16 ? 16 : (cout <= 32 ? 32 : 64)); }
inline int in_chunks(int cin) { return (cin + CH - 1) / CH; }
inline int dw_chunks(int ncol) { return (ncol + TB - 1) / TB; }
inline int out_blocks(long long total) {
    const long long b = (total + TB - 1) / TB;
    return (int)(b > EW_MAXBLK ? EW_MAXBLK : b);
}

// Sums of the per-block partials [nblk][nv] (nv <= 2 MAXC) into tot[nv], computed by EVERY block in the same order:
// slice s adds partials s, s + S, ...; the slices are then added in slice order.
__device__ __forceinline__ void fold(const double *__restrict__ part, int nblk, int nv, double *sl, double *tot) {
    int vp = 1;
    while (vp < nv) vp <<= 1;
    const int S = TB / vp, col = threadIdx.x % vp, s0 = threadIdx.x / vp;
    double a = 0.0;
    if (col < nv)
        for (int p = s0; p < nblk; p += S) a += part[(long long)p * nv + col];
    sl[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x < nv) {
        double t = 0.0;
        for (int q = 0; q < S; ++q) t += sl[q * vp + threadIdx.x];
        tot[threadIdx.x] = t;
    }
    __syncthreads();
}

// Block sums of the per-thread (s, q)[CH] -> dst[(c0 + c) * 2 + {0, 1}]: xor tree over the lanes, then the waves in
// wave order.  Called by every thread of the block.
__device__ __forceinline__ void block_sums(double (&s)[CH], double (&q)[CH], double (*red)[2 * CH], double *dst, int c0,
                                           int C) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            s[c] += __shfl_xor(s[c], off, 64);
            q[c] += __shfl_xor(q[c], off, 64);
        }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            red[wv][c] = s[c];
            red[wv][CH + c] = q[c];
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * CH) {
        double v = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < TB / 64; ++w) v += red[w][threadIdx.x];
        const int c = threadIdx.x % CH, which = threadIdx.x / CH;
        if (c0 + c < C) dst[(c0 + c) * 2 + which] = v;
    }
}

// BN coefficients of one layer in LDS: mean, invstd, gamma, beta
struct BnLds {
    float m[MAXC], is[MAXC], ga[MAXC], be[MAXC];
};

// The statistics of a layer of C channels over M elements per channel: folded from the partials (training; `publish`:
// this block also saves mean / invstd and updates the running statistics) or the running ones (eval).
__device__ __forceinline__ void bn_prologue(const Conv1dPtrs &p, int C, const double *__restrict__ part, int nblk,
                                            long long M, int training, float momentum, float eps, float *stats_out,
                                            bool publish, double *sl, double *tot, BnLds &bn) {
    const int c = threadIdx.x;
    if (training) {
        fold(part, nblk, 2 * C, sl, tot);
        if (c < C) {
            const double cnt = (double)M;
            const double md = M > 0 ? tot[2 * c] / cnt : 0.0;
            double var = M > 0 ? tot[2 * c + 1] / cnt - md * md : 0.0;   // biased, what torch normalises with
            var = var > 0.0 ? var : 0.0;
            const float mean = (float)md, inv = (float)(1.0 / sqrt(var + (double)eps));
            bn.m[c] = mean;
            bn.is[c] = inv;
            if (publish) {
                stats_out[c] = mean;
                stats_out[MAXC + c] = inv;
                if (p.rm && p.rv) {
                    const float unbiased = (float)(M > 1 ? var * (cnt / (cnt - 1.0)) : var);
                    p.rm[c] = (1.f - momentum) * p.rm[c] + momentum * mean;
                    p.rv[c] = (1.f - momentum) * p.rv[c] + momentum * unbiased;
                }
            }
        }
        if (publish && c == 0 && p.nbt) *p.nbt += 1;
    } else if (c < C) {
        const float mean = p.rm[c], inv = (float)(1.0 / sqrt((double)p.rv[c] + (double)eps));
        bn.m[c] = mean;
        bn.is[c] = inv;
        if (publish) {
            stats_out[c] = mean;
            stats_out[MAXC + c] = inv;
        }
    }
    if (c < C) {
        bn.ga[c] = p.ga[c];
        bn.be[c] = p.be[c];
    }
    __syncthreads();
}

struct FwdArgs {
    Layer ly;
    int layer;      // this layer's record of the pointer table
    const void *X;  // the layer's input: the rows (x_dt) or z of the previous layer (fp32)
    int x_dt;
    int has_prev;         // X is z_{layer-1}: BN + ReLU applied on load, statistics from pstat
    const double *pstat;  // [pnblk][cin][2] partials of the previous layer
    int pnblk;
    float pmom, peps;
    float *pstats_out;  // [2][MAXC] mean / invstd of the previous layer, for the backward
    float *Z;           // [N][cout][lout]
    double *stat;       // [gridDim.x][cout][2] this layer's partials (training)
};

__global__ void __launch_bounds__(TB) k_c1d_fwd(FwdArgs a, const Conv1dPtrs *__restrict__ pp, long long N,
                                                const long long *__restrict__ n_dev, int training) {
    __shared__ float Ws[CH * MAXC * MAXK];  // [CH][cin][fs], rows past cout zero
    __shared__ float Bs[CH];
    __shared__ BnLds bn;
    __shared__ double sl[TB], tot[2 * MAXC], red[TB / 64][2 * CH];
    const Layer ly = a.ly;
    const int co0 = blockIdx.y * CH, ck = ly.cin * ly.fs;
    const Conv1dPtrs p = pp[a.layer];
    for (int i = threadIdx.x; i < CH * ck; i += TB) {
        const int co = co0 + i / ck;
        Ws[i] = co < ly.cout ? p.w[(long long)co * ck + (i - (i / ck) * ck)] : 0.f;
    }
    if (threadIdx.x < CH) Bs[threadIdx.x] = (p.b && co0 + threadIdx.x < ly.cout) ? p.b[co0 + threadIdx.x] : 0.f;
    const long long Nv = wfs_valid_rows_nonneg(N, n_dev);
    if (a.has_prev)
        bn_prologue(pp[a.layer - 1], ly.cin, a.pstat, a.pnblk, Nv * ly.lin, training, a.pmom, a.peps, a.pstats_out,
                    blockIdx.x == 0 && blockIdx.y == 0, sl, tot, bn);
    else
        __syncthreads();
    double s[CH], q[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) s[c] = q[c] = 0.0;
    const long long P = N * ly.lout;
    for (long long pos = (long long)blockIdx.x * TB + threadIdx.x; pos < P; pos += (long long)gridDim.x * TB) {
        const long long n = pos / ly.lout;
        const int t = (int)(pos - n * ly.lout);
        const bool valid = n < Nv;
        float acc[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) acc[c] = valid ? Bs[c] : 0.f;
        if (valid) {
            const int s0 = t * ly.st - ly.pd;
            for (int ci = 0; ci < ly.cin; ++ci) {
                const long long base = (n * ly.cin + ci) * ly.lin;
                const float m = bn.m[ci], is = bn.is[ci], ga = bn.ga[ci], be = bn.be[ci];
                for (int j = 0; j < ly.fs; ++j) {
                    const int si = s0 + j;
                    float xv = 0.f;                      // zero padding of the ACTIVATION
                    if (si >= 0 && si < ly.lin) {
                        xv = ldt(a.X, base + si, a.x_dt);
                        if (a.has_prev) {
                            const float y = fmaf(ga, (xv - m) * is, be);      // the backward's mask expression
                            xv = y > 0.f ? y : 0.f;
                        }
                    }
                    const float *w = Ws + ci * ly.fs + j;
#pragma unroll
                    for (int c = 0; c < CH; ++c) acc[c] = fmaf(w[c * ck], xv, acc[c]);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int co = co0 + c;
            if (co < ly.cout) {
                a.Z[(n * ly.cout + co) * ly.lout + t] = acc[c];
                if (valid) {
                    s[c] += (double)acc[c];
                    q[c] += (double)acc[c] * (double)acc[c];
                }
            }
        }
    }
    if (training) block_sums(s, q, red, a.stat + (long long)blockIdx.x * 2 * ly.cout, co0, ly.cout);
}

// Y = relu(bn(z_last)) in the rows' dtype; rows at or beyond the valid count get zeros
__global__ void __launch_bounds__(TB) k_c1d_out(const float *__restrict__ Z, int C, int L, int layer,
                                                const Conv1dPtrs *__restrict__ pp, const double *__restrict__ stat,
                                                int nblk, float momentum, float eps, float *stats_out, void *Y, int y_dt,
                                                long long N, const long long *__restrict__ n_dev, int training) {
    __shared__ BnLds bn;
    __shared__ double sl[TB], tot[2 * MAXC];
    const long long Nv = wfs_valid_rows_nonneg(N, n_dev);
    bn_prologue(pp[layer], C, stat, nblk, Nv * L, training, momentum, eps, stats_out, blockIdx.x == 0, sl, tot, bn);
    const long long total = N * C * L, per = (long long)C * L;
    for (long long i = (long long)blockIdx.x * TB + threadIdx.x; i < total; i += (long long)gridDim.x * TB) {
        const long long n = i / per;
        float y = 0.f;
        if (n < Nv) {
            const int c = (int)((i - n * per) / L);
            y = fmaf(bn.ga[c], (Z[i] - bn.m[c]) * bn.is[c], bn.be[c]);
            y = y > 0.f ? y : 0.f;
        }
        stt(Y, i, y_dt, y);
    }
}

// g_last = dY [y_last > 0] (fp32) and its partial sums (sum g, sum g xhat) per channel
__global__ void __launch_bounds__(TB) k_c1d_bwd_head(const void *__restrict__ dY, int g_dt, const float *__restrict__ Z,
                                                     int C, int L, int layer, const Conv1dPtrs *__restrict__ pp,
                                                     const float *__restrict__ stats, float *__restrict__ G,
                                                     double *__restrict__ ostat, long long N,
                                                     const long long *__restrict__ n_dev) {
    __shared__ BnLds bn;
    __shared__ double red[TB / 64][2 * CH];
    const Conv1dPtrs p = pp[layer];
    if (threadIdx.x < C) {
        bn.m[threadIdx.x] = stats[threadIdx.x];
        bn.is[threadIdx.x] = stats[MAXC + threadIdx.x];
        bn.ga[threadIdx.x] = p.ga[threadIdx.x];
        bn.be[threadIdx.x] = p.be[threadIdx.x];
    }
    __syncthreads();
    const long long Nv = wfs_valid_rows_nonneg(N, n_dev);
    const int c0 = blockIdx.y * CH;
    double s[CH], q[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) s[c] = q[c] = 0.0;
    const long long P = N * L;
    for (long long pos = (long long)blockIdx.x * TB + threadIdx.x; pos < P; pos += (long long)gridDim.x * TB) {
        const long long n = pos / L;
        const int t = (int)(pos - n * L);
        const bool valid = n < Nv;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int ch = c0 + c;
            if (ch >= C) break;
            const long long o = (n * C + ch) * L + t;
            float g = 0.f;
            if (valid) {
                const float xh = (Z[o] - bn.m[ch]) * bn.is[ch];
                if (fmaf(bn.ga[ch], xh, bn.be[ch]) > 0.f) g = ldt(dY, o, g_dt);
                s[c] += (double)g;
                q[c] += (double)g * (double)xh;
            }
            G[o] = g;
        }
    }
    block_sums(s, q, red, ostat + (long long)blockIdx.x * 2 * C, c0, C);
}

struct BwdArgs {
    Layer ly;
    int layer;
    const float *G, *Z;   // g_i and z_i [N][cout][lout]
    const float *stats;   // [2][MAXC] mean / invstd of layer i
    const double *gstat;  // [gnblk][cout][2] partials of (sum g_i, sum g_i xhat_i)
    int gnblk;
    int training;
    const void *Xin;  // the layer's input: the rows (x_dt) or z_{i-1} (fp32)
    int x_dt;
    int has_prev;
    const float *pstats;  // mean / invstd of layer i-1
    float *Gout;          // g_{i-1} [N][cin][lin] (has_prev)
    double *ostat;        // [nbx][cin][2] its partials
    void *dX;             // layer 0: the rows' gradient (dx_dt), or NULL
    int dx_dt;
    int nbx, nchunk;      // role A: position blocks x input-channel chunks (0 blocks when there is nothing to produce)
    float *part;          // role B: [dw_nblk][cout][cin fs + 1] partials of dW (and, last column, db)
    int dw_nblk;
};

// the activation a_{i-1} at (row n, channel ci, sample si) from the layer's input
__device__ __forceinline__ float act_in(const BwdArgs &a, const BnLds &pbn, long long n, int ci, int si) {
    float xv = ldt(a.Xin, (n * a.ly.cin + ci) * a.ly.lin + si, a.x_dt);
    if (a.has_prev) {
        const float y = fmaf(pbn.ga[ci], (xv - pbn.m[ci]) * pbn.is[ci], pbn.be[ci]);
        xv = y > 0.f ? y : 0.f;
    }
    return xv;
}

template <int CO>
__global__ void __launch_bounds__(TB) k_c1d_bwd(BwdArgs a, const Conv1dPtrs *__restrict__ pp, long long N,
                                                const long long *__restrict__ n_dev) {
    __shared__ float buf[TB * DW_TP];         // role A: Wt[cout][CH][fs]; role B: XS[column][DW_TP]
    __shared__ float GZs[MAXC * DW_TP];       // role B: dz tile [cout][DW_TP]
    __shared__ BnLds bn, pbn;                 // layer i (bn.ga holds gamma invstd), layer i-1
    __shared__ float k1[MAXC], k2[MAXC];
    __shared__ double sl[TB], tot[2 * MAXC], red[TB / 64][2 * CH];
    const Layer ly = a.ly;
    const Conv1dPtrs p = pp[a.layer];
    const long long Nv = wfs_valid_rows_nonneg(N, n_dev);
    // ---- both roles: layer i's sums, dz_i = coef (g - k1 - xhat k2)
    fold(a.gstat, a.gnblk, 2 * ly.cout, sl, tot);
    if (threadIdx.x < ly.cout) {
        const int c = threadIdx.x;
        const long long M = Nv * ly.lout;
        const float is = a.stats[MAXC + c];
        bn.m[c] = a.stats[c];
        bn.is[c] = is;
        bn.ga[c] = p.ga[c] * is;
        k1[c] = (a.training && M > 0) ? (float)(tot[2 * c] / (double)M) : 0.f;
        k2[c] = (a.training && M > 0) ? (float)(tot[2 * c + 1] / (double)M) : 0.f;
        if (blockIdx.x == 0) {
            if (p.dbe) p.dbe[c] = (float)tot[2 * c];
            if (p.dga) p.dga[c] = (float)tot[2 * c + 1];
        }
    }
    if (a.has_prev && threadIdx.x < ly.cin) {
        const Conv1dPtrs pq = pp[a.layer - 1];
        const int c = threadIdx.x;
        pbn.m[c] = a.pstats[c];
        pbn.is[c] = a.pstats[MAXC + c];
        pbn.ga[c] = pq.ga[c];
        pbn.be[c] = pq.be[c];
    }
    __syncthreads();
    const int nA = a.nbx * a.nchunk;
    if ((int)blockIdx.x < nA) {
        // ---- role A: da_{i-1}[n][ci][s] = sum_co sum_j W[co][ci][j] dz_i[n][co][t],  t st - pd + j = s
        const int bx = blockIdx.x % a.nbx, ci0 = (blockIdx.x / a.nbx) * CH;
        float *Wt = buf;
        for (int i = threadIdx.x; i < ly.cout * CH * ly.fs; i += TB) {
            const int co = i / (CH * ly.fs), r = i - co * CH * ly.fs, c = r / ly.fs, j = r - c * ly.fs;
            Wt[i] = ci0 + c < ly.cin ? p.w[((long long)co * ly.cin + ci0 + c) * ly.fs + j] : 0.f;
        }
        __syncthreads();
        double s[CH], q[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) s[c] = q[c] = 0.0;
        const long long P = N * ly.lin;
        for (long long pos = (long long)bx * TB + threadIdx.x; pos < P; pos += (long long)a.nbx * TB) {
            const long long n = pos / ly.lin;
            const int si = (int)(pos - n * ly.lin);
            const bool valid = n < Nv;
            float acc[CH];
#pragma unroll
            for (int c = 0; c < CH; ++c) acc[c] = 0.f;
            if (valid) {
                for (int j = 0; j < ly.fs; ++j) {
                    const int tn = si + ly.pd - j;
                    if (tn < 0) break;                                 // larger j: smaller tn
                    const int t = tn / ly.st;
                    if (t * ly.st != tn || t >= ly.lout) continue;
                    for (int co = 0; co < ly.cout; ++co) {
                        const long long o = (n * ly.cout + co) * ly.lout + t;
                        const float xh = (a.Z[o] - bn.m[co]) * bn.is[co];
                        const float dz = bn.ga[co] * (a.G[o] - k1[co] - xh * k2[co]);
                        const float *w = Wt + co * CH * ly.fs + j;
#pragma unroll
                        for (int c = 0; c < CH; ++c) acc[c] = fmaf(w[c * ly.fs], dz, acc[c]);
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const int ci = ci0 + c;
                if (ci >= ly.cin) break;
                const long long o = (n * ly.cin + ci) * ly.lin + si;
                if (a.has_prev) {
                    float g = 0.f;
                    if (valid) {
                        const float xh = (((const float *)a.Xin)[o] - pbn.m[ci]) * pbn.is[ci];
                        if (fmaf(pbn.ga[ci], xh, pbn.be[ci]) > 0.f) g = acc[c];
                        s[c] += (double)g;
                        q[c] += (double)g * (double)xh;
                    }
                    a.Gout[o] = g;
                } else {
                    stt(a.dX, o, a.dx_dt, acc[c]);
                }
            }
        }
        if (a.has_prev) block_sums(s, q, red, a.ostat + (long long)bx * 2 * ly.cin, ci0, ly.cin);
        return;
    }
    // ---- role B: dW[co][ci fs + j] = sum over positions of dz[co][n, t] a_{i-1}[ci][n, t st - pd + j]; the last column
    // (an input of ones) is db.  This block owns up to TB columns and the tiles b, b + dw_nblk, ...; inside a tile
    // `groups` thread groups take interleaved positions and are added in group order at the end.
    const int bb = (int)blockIdx.x - nA, b = bb % a.dw_nblk, col0 = (bb / a.dw_nblk) * TB;
    const int ncol = ly.cin * ly.fs + 1, mycols = dw_mycols(ncol, col0);
    const int groups = dw_groups(mycols);
    int grp = threadIdx.x / mycols;
    const int col = threadIdx.x - grp * mycols;
    if (grp >= groups) grp = -1;
    float *XS = buf;
    float acc[CO];
#pragma unroll
    for (int c = 0; c < CO; ++c) acc[c] = 0.f;
    for (int i = threadIdx.x; i < MAXC * DW_TP; i += TB) GZs[i] = 0.f;
    const long long P = N * ly.lout;
    for (long long tile = b; tile * DW_TP < P; tile += a.dw_nblk) {
        const long long p0 = tile * DW_TP;
        __syncthreads();
        for (int e = threadIdx.x; e < ly.cout * DW_TP; e += TB) {
            const int co = e / DW_TP, pi = e - co * DW_TP;
            const long long pos = p0 + pi;
            float v = 0.f;
            if (pos < P) {
                const long long n = pos / ly.lout;
                if (n < Nv) {
                    const long long o = (n * ly.cout + co) * ly.lout + (pos - n * ly.lout);
                    const float xh = (a.Z[o] - bn.m[co]) * bn.is[co];
                    v = bn.ga[co] * (a.G[o] - k1[co] - xh * k2[co]);
                }
            }
            GZs[e] = v;
        }
        for (int e = threadIdx.x; e < mycols * DW_TP; e += TB) {
            const int cl = e / DW_TP, pi = e - cl * DW_TP, gc = col0 + cl;
            const long long pos = p0 + pi;
            float v = 0.f;
            if (pos < P) {
                const long long n = pos / ly.lout;
                if (n < Nv) {
                    if (gc == ncol - 1) {
                        v = 1.f;
                    } else {
                        const int ci = gc / ly.fs, j = gc - ci * ly.fs;
                        const int si = (int)(pos - n * ly.lout) * ly.st - ly.pd + j;
                        if (si >= 0 && si < ly.lin) v = act_in(a, pbn, n, ci, si);
                    }
                }
            }
            XS[e] = v;
        }
        __syncthreads();
        if (grp >= 0) {
            const float *xs = XS + col * DW_TP;
            for (int pi = grp; pi < DW_TP; pi += groups) {
                const float xv = xs[pi];
#pragma unroll
                for (int c = 0; c < CO; ++c) acc[c] = fmaf(GZs[c * DW_TP + pi], xv, acc[c]);
            }
        }
    }
    float *out = a.part + (long long)b * ly.cout * ncol + col0;
    if (groups == 1) {
        if (grp >= 0) {
#pragma unroll
            for (int c = 0; c < CO; ++c)
                if (c < ly.cout) out[c * ncol + col] = acc[c];
        }
        return;
    }
    // the groups' sums through XS, at most 32 channels at a time: groups x 32 x mycols <= TB x 32 floats
    constexpr int CW = CO < 32 ? CO : 32;
#pragma unroll
    for (int cb = 0; cb < CO; cb += CW) {
        __syncthreads();
        if (grp >= 0) {
#pragma unroll
            for (int c = 0; c < CW; ++c) XS[(grp * CW + c) * mycols + col] = acc[cb + c];
        }
        __syncthreads();
        for (int e = threadIdx.x; e < CW * mycols; e += TB) {
            const int c = e / mycols;
            if (cb + c >= ly.cout) break;
            float v = 0.f;
            for (int gi = 0; gi < groups; ++gi) v += XS[gi * CW * mycols + e];
            out[(cb + c) * ncol + (e - c * mycols)] = v;
        }
    }
}

struct DwDesc {
    int cout, ncol, nblk;
    long long p_off;
};
struct DwTable {
    DwDesc d[MAXLY];
};

// block (layer, output channel): the dW blocks' partials added in block order (in double) into the gradient slots
__global__ void __launch_bounds__(TB) k_c1d_dw_reduce(const Conv1dPtrs *__restrict__ pp, DwTable tab,
                                                      const float *__restrict__ part) {
    const DwDesc d = tab.d[blockIdx.x];
    const int co = blockIdx.y;
    if (co >= d.cout) return;
    const Conv1dPtrs p = pp[blockIdx.x];
    const float *q0 = part + d.p_off + (long long)co * d.ncol;
    for (int q = threadIdx.x; q < d.ncol; q += TB) {
        double s = 0.0;
        for (int b = 0; b < d.nblk; ++b) s += (double)q0[(long long)b * d.cout * d.ncol + q];
        if (q < d.ncol - 1) {
            if (p.dw) p.dw[(long long)co * (d.ncol - 1) + q] = (float)s;
        } else if (p.db) {
            p.db[co] = (float)s;
        }
    }
}

int make_plan(int32_t c0, const int32_t *channels, const int32_t *fs, const int32_t *st, const int32_t *pd,
              int32_t layers, int32_t L, Plan *pl) {
    WFS_REQUIRE(layers >= 1 && layers <= MAXLY, WFS_EINVAL, "conv stack of %d layers: 1 .. %d supported", layers, MAXLY);
    WFS_REQUIRE(channels && fs && st && pd, WFS_EINVAL, "NULL layer description");
    WFS_REQUIRE(c0 >= 1 && c0 <= MAXC, WFS_EINVAL, "conv stack input of %d channels: 1 .. %d supported", c0, MAXC);
    WFS_REQUIRE(L >= 1 && L <= MAXL, WFS_EINVAL, "row length %d not in [1, %d]", L, MAXL);
    int cin = c0, lin = L;
    for (int i = 0; i < layers; ++i) {
        WFS_REQUIRE(channels[i] >= 1 && channels[i] <= MAXC, WFS_EINVAL, "conv layer %d has %d channels: 1 .. %d supported",
                    i, channels[i], MAXC);
        WFS_REQUIRE(fs[i] >= 1 && fs[i] <= MAXK, WFS_EINVAL, "conv layer %d kernel size %d: 1 .. %d supported", i, fs[i], MAXK);
        WFS_REQUIRE(st[i] >= 1 && st[i] <= MAXS, WFS_EINVAL, "conv layer %d stride %d: 1 .. %d supported", i, st[i], MAXS);
        WFS_REQUIRE(pd[i] >= 0 && pd[i] < fs[i], WFS_EINVAL, "conv layer %d padding %d: 0 .. kernel size - 1 supported", i, pd[i]);
        const int num = lin + 2 * pd[i] - fs[i];
        WFS_REQUIRE(num >= 0, WFS_EINVAL, "conv layer %d: kernel %d does not fit %d + 2 x %d samples", i, fs[i], lin, pd[i]);
        Layer &ly = pl->ly[i];
        ly.cin = cin;
        ly.cout = channels[i];
        ly.fs = fs[i];
        ly.st = st[i];
        ly.pd = pd[i];
        ly.lin = lin;
        ly.lout = num / st[i] + 1;
        cin = ly.cout;
        lin = ly.lout;
    }
    pl->n = layers;
    return WFS_OK;
}

int check_common(int32_t c0, const int32_t *channels, const int32_t *fs, const int32_t *st, const int32_t *pd,
                 int32_t layers, int64_t N, int32_t L, int32_t dtype, Plan *pl) {
    int rc = make_plan(c0, channels, fs, st, pd, layers, L, pl);
    if (rc != WFS_OK) return rc;
    WFS_REQUIRE(N >= 0 && N <= (1ll << 40) / ((long long)MAXL * MAXC), WFS_EINVAL, "%lld rows", (long long)N);
    WFS_REQUIRE(wfs_dtype_ok(dtype), WFS_EINVAL, "bad dtype %d", dtype);
    return WFS_OK;
}

int pos_blocks(long long P) {
    long long b = (P + TB - 1) / TB;
    return (int)(b < 1 ? 1 : (b > ST_MAXBLK ? ST_MAXBLK : b));
}

// position blocks of role A of k_c1d_bwd over the layer's input: none when layer 0's input gradient is not wanted
int role_a_blocks(long long N, const Layer &ly, bool wanted) { return wanted ? pos_blocks(N * ly.lin) : 0; }

size_t even(size_t v) { return (v + 1) & ~(size_t)1; }          // doubles follow floats: keep them 8-byte aligned

// `saved`: z of every layer | [layers][2][MAXC] mean / invstd | the forward's statistics partials (doubles)
struct SavedLayout {
    size_t z[MAXLY], stats, part[MAXLY], total;
};
SavedLayout saved_layout(const Plan &pl, long long N) {
    SavedLayout s;
    size_t off = 0;
    for (int i = 0; i < pl.n; ++i) {
        s.z[i] = off;
        off += (size_t)N * pl.ly[i].cout * pl.ly[i].lout;
    }
    s.stats = off;
    off = even(off + (size_t)pl.n * 2 * MAXC);
    for (int i = 0; i < pl.n; ++i) {
        s.part[i] = off;
        off += 2 * (size_t)pos_blocks(N * pl.ly[i].lout) * 2 * pl.ly[i].cout;       // doubles, counted in floats
    }
    s.total = off;
    return s;
}

// backward workspace: g ping-pong | (sum g, sum g xhat) partials ping-pong (doubles) | dW partials of every layer
struct WorkLayout {
    size_t g[2], stat[2], part[MAXLY], total;
    int dw_nblk[MAXLY];
};
WorkLayout work_layout(const Plan &pl, long long N) {
    WorkLayout w;
    size_t gmax = 0;
    for (int i = 0; i < pl.n; ++i) {
        const size_t e = (size_t)N * pl.ly[i].cout * pl.ly[i].lout;
        gmax = e > gmax ? e : gmax;
    }
    gmax = even(gmax);
    w.g[0] = 0;
    w.g[1] = gmax;
    w.stat[0] = 2 * gmax;
    w.stat[1] = w.stat[0] + 2 * (size_t)ST_MAXBLK * 2 * MAXC;
    size_t off = w.stat[1] + 2 * (size_t)ST_MAXBLK * 2 * MAXC;
    for (int i = 0; i < pl.n; ++i) {
        const Layer &ly = pl.ly[i];
        w.dw_nblk[i] = wfs_dw_blocks(N * ly.lout, DW_TP, DW_MAXBLK);
        w.part[i] = off;
        off += (size_t)w.dw_nblk[i] * ly.cout * (ly.cin * ly.fs + 1);
    }
    w.total = off;
    return w;
}

}  // namespace

extern "C" int wfs_conv1d_ok(int32_t c0, const int32_t *channels, const int32_t *fs, const int32_t *st, const int32_t *pd,
                             int32_t layers, int32_t L, int32_t dtype) {
    Plan pl;
    return check_common(c0, channels, fs, st, pd, layers, 1, L, dtype, &pl);
}

extern "C" size_t wfs_conv1d_saved_floats(int64_t N, int32_t L, int32_t c0, const int32_t *channels, const int32_t *fs,
                                          const int32_t *st, const int32_t *pd, int32_t layers) {
    Plan pl;
    if (check_common(c0, channels, fs, st, pd, layers, N, L, WFS_F32, &pl) != WFS_OK) return 0;
    return saved_layout(pl, N).total;
}

extern "C" size_t wfs_conv1d_bwd_workspace_floats(int64_t N, int32_t L, int32_t c0, const int32_t *channels,
                                                  const int32_t *fs, const int32_t *st, const int32_t *pd,
                                                  int32_t layers) {
    Plan pl;
    if (check_common(c0, channels, fs, st, pd, layers, N, L, WFS_F32, &pl) != WFS_OK) return 0;
    return work_layout(pl, N).total;
}

// Host only, launches nothing: what the launches below do with every layer of the plan, out[layers][10] =
//   {L_in, L_out, position blocks of the forward / head pass over N L_out, role A's position blocks when its input
//    gradient is wanted (over N L_in), its input-channel chunks, dW blocks per column chunk, column chunks,
//    columns of the last chunk, thread groups of the last chunk, CO}
// and, after the layers, out[layers * 10] = the blocks of k_c1d_out.  tests/test_conv1d_cases_host.py takes from here
// which arm a case of its table reaches.  Built from what the launches use: make_plan, pos_blocks, work_layout and the
// helpers under Plan.
extern "C" int wfs_conv1d_arms(int64_t N, int32_t L, int32_t c0, const int32_t *channels, const int32_t *fs,
                               const int32_t *st, const int32_t *pd, int32_t layers, int32_t *out) {
    Plan pl;
    int rc = check_common(c0, channels, fs, st, pd, layers, N, L, WFS_F32, &pl);
    if (rc != WFS_OK) return rc;
    WFS_REQUIRE(out, WFS_EINVAL, "NULL output");
    const WorkLayout wl = work_layout(pl, N);
    for (int i = 0; i < layers; ++i) {
        const Layer &ly = pl.ly[i];
        const int ncol = ly.cin * ly.fs + 1, chunks = dw_chunks(ncol), mycols = dw_mycols(ncol, (chunks - 1) * TB);
        int32_t *o = out + 10 * i;
        o[0] = ly.lin;
        o[1] = ly.lout;
        o[2] = pos_blocks(N * ly.lout);
        o[3] = role_a_blocks(N, ly, true);
        o[4] = in_chunks(ly.cin);
        o[5] = wl.dw_nblk[i];
        o[6] = chunks;
        o[7] = mycols;
        o[8] = dw_groups(mycols);
        o[9] = dw_co(ly.cout);
    }
    const Layer &last = pl.ly[layers - 1];
    out[10 * layers] = out_blocks(N * (long long)last.cout * last.lout);
    return WFS_OK;
}

extern "C" int wfs_conv1d_fwd(const void *X, int64_t N, int32_t L, int32_t c0, const int32_t *channels, const int32_t *fs,
                              const int32_t *st, const int32_t *pd, int32_t layers, const void *param_ptrs,
                              const float *momentum, const float *eps, int32_t training, float *saved, void *Y,
                              int32_t dtype, const int64_t *n_valid_dev, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    Plan pl;
    int rc = check_common(c0, channels, fs, st, pd, layers, N, L, dtype, &pl);
    if (rc != WFS_OK) return rc;
    WFS_REQUIRE(momentum && eps, WFS_EINVAL, "NULL momentum / eps list");
    for (int i = 0; i < layers; ++i)
        WFS_REQUIRE(momentum[i] >= 0.f && momentum[i] <= 1.f && eps[i] >= 0.f, WFS_EINVAL,
                    "BatchNorm of layer %d: momentum %g, eps %g", i, (double)momentum[i], (double)eps[i]);
    if (N == 0) return WFS_OK;
    WFS_REQUIRE(X && param_ptrs && saved && Y, WFS_EINVAL, "NULL device pointer");
    const SavedLayout sl = saved_layout(pl, N);
    const Conv1dPtrs *pp = (const Conv1dPtrs *)param_ptrs;
    const long long *n_dev = (const long long *)n_valid_dev;
    for (int i = 0; i < layers; ++i) {
        const Layer &ly = pl.ly[i];
        FwdArgs a = {};
        a.ly = ly;
        a.layer = i;
        a.X = i == 0 ? X : (const void *)(saved + sl.z[i - 1]);
        a.x_dt = i == 0 ? dtype : WFS_F32;
        a.has_prev = i > 0;
        if (i > 0) {
            a.pstat = (const double *)(saved + sl.part[i - 1]);
            a.pnblk = pos_blocks(N * pl.ly[i - 1].lout);
            a.pmom = momentum[i - 1];
            a.peps = eps[i - 1];
            a.pstats_out = saved + sl.stats + (size_t)(i - 1) * 2 * MAXC;
        }
        a.Z = saved + sl.z[i];
        a.stat = (double *)(saved + sl.part[i]);
        const dim3 grid((unsigned)pos_blocks(N * ly.lout), (unsigned)((ly.cout + CH - 1) / CH));
        k_c1d_fwd<<<grid, dim3(TB), 0, stream>>>(a, pp, N, n_dev, training);
        WFS_LAUNCH_CHECK();
    }
    const Layer &last = pl.ly[layers - 1];
    const long long total = N * (long long)last.cout * last.lout;
    k_c1d_out<<<dim3((unsigned)out_blocks(total)), dim3(TB), 0, stream>>>(
        saved + sl.z[layers - 1], last.cout, last.lout, layers - 1, pp, (const double *)(saved + sl.part[layers - 1]),
        pos_blocks(N * last.lout), momentum[layers - 1], eps[layers - 1], saved + sl.stats + (size_t)(layers - 1) * 2 * MAXC,
        Y, dtype, N, n_dev, training);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}

extern "C" int wfs_conv1d_bwd(const void *X, const void *dY, int64_t N, int32_t L, int32_t c0, const int32_t *channels,
                              const int32_t *fs, const int32_t *st, const int32_t *pd, int32_t layers,
                              const void *param_ptrs, int32_t training, const float *saved, void *dX, float *workspace,
                              int32_t dtype, const int64_t *n_valid_dev, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    Plan pl;
    int rc = check_common(c0, channels, fs, st, pd, layers, N, L, dtype, &pl);
    if (rc != WFS_OK) return rc;
    WFS_REQUIRE(N >= 1, WFS_EINVAL, "the backward needs at least one row (the gradients of an empty batch are zeros)");
    WFS_REQUIRE(X && dY && param_ptrs && saved && workspace, WFS_EINVAL, "NULL device pointer");
    const SavedLayout sl = saved_layout(pl, N);
    const WorkLayout wl = work_layout(pl, N);
    const Conv1dPtrs *pp = (const Conv1dPtrs *)param_ptrs;
    const long long *n_dev = (const long long *)n_valid_dev;
    float *G[2] = {workspace + wl.g[0], workspace + wl.g[1]};
    double *ST[2] = {(double *)(workspace + wl.stat[0]), (double *)(workspace + wl.stat[1])};
    const Layer &last = pl.ly[layers - 1];
    int cur = 0;
    int gnblk = pos_blocks(N * last.lout);
    k_c1d_bwd_head<<<dim3((unsigned)gnblk, (unsigned)((last.cout + CH - 1) / CH)), dim3(TB), 0, stream>>>(
        dY, dtype, saved + sl.z[layers - 1], last.cout, last.lout, layers - 1, pp,
        saved + sl.stats + (size_t)(layers - 1) * 2 * MAXC, G[cur], ST[cur], N, n_dev);
    WFS_LAUNCH_CHECK();
    DwTable tab = {};
    int maxc = 0;
    for (int i = layers - 1; i >= 0; --i) {
        const Layer &ly = pl.ly[i];
        BwdArgs a = {};
        a.ly = ly;
        a.layer = i;
        a.G = G[cur];
        a.Z = saved + sl.z[i];
        a.stats = saved + sl.stats + (size_t)i * 2 * MAXC;
        a.gstat = ST[cur];
        a.gnblk = gnblk;
        a.training = training;
        a.Xin = i == 0 ? X : (const void *)(saved + sl.z[i - 1]);
        a.x_dt = i == 0 ? dtype : WFS_F32;
        a.has_prev = i > 0;
        a.nchunk = in_chunks(ly.cin);
        if (i > 0) {
            a.pstats = saved + sl.stats + (size_t)(i - 1) * 2 * MAXC;
            a.Gout = G[cur ^ 1];
            a.ostat = ST[cur ^ 1];
            a.nbx = role_a_blocks(N, ly, true);
        } else {
            a.dX = dX;
            a.dx_dt = dtype;
            a.nbx = role_a_blocks(N, ly, dX != nullptr);
        }
        a.part = workspace + wl.part[i];
        a.dw_nblk = wl.dw_nblk[i];
        const int ncol = ly.cin * ly.fs + 1;
        const unsigned grid = (unsigned)(a.nbx * a.nchunk + a.dw_nblk * dw_chunks(ncol));
        switch (dw_co(ly.cout)) {
        case 8: k_c1d_bwd<8><<<dim3(grid), dim3(TB), 0, stream>>>(a, pp, N, n_dev); break;
        case 16: k_c1d_bwd<16><<<dim3(grid), dim3(TB), 0, stream>>>(a, pp, N, n_dev); break;
        case 32: k_c1d_bwd<32><<<dim3(grid), dim3(TB), 0, stream>>>(a, pp, N, n_dev); break;
        default: k_c1d_bwd<64><<<dim3(grid), dim3(TB), 0, stream>>>(a, pp, N, n_dev); break;
        }
        WFS_LAUNCH_CHECK();
        tab.d[i].cout = ly.cout;
        tab.d[i].ncol = ncol;
        tab.d[i].nblk = a.dw_nblk;
        tab.d[i].p_off = (long long)(wl.part[i] - wl.part[0]);
        maxc = ly.cout > maxc ? ly.cout : maxc;
        gnblk = a.nbx;
        cur ^= 1;
    }
    k_c1d_dw_reduce<<<dim3((unsigned)layers, (unsigned)maxc), dim3(TB), 0, stream>>>(pp, tab, workspace + wl.part[0]);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}
