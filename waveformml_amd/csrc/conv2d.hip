// conv2d.hip -- the dense stack  n x (Conv2d(stride, zero padding, dilation, optional bias) -> BatchNorm2d -> ReLU
// [-> Dropout])  on event maps, and the launch that builds those maps from sparse rows.
//
// Reference: Conv2DBlock (src/models/ConvBlocks.py:220-289) under DenseConvNet (src/models/DenseConvNet.py): COO rows ->
// to_dense -> the block -> LinearBlock.  Per layer nn.Conv2d(cin, cout, (fs, fs), (st, st), pd, (dil, dil), bias or
// none), nn.BatchNorm2d(cout), nn.ReLU, nn.Dropout(p) when the block was built with one.
//
// Layout: every map inside the stack is channels-LAST, [B][H][W][C] = a matrix [M = B H W][C]: a row of the sparse input
// is one contiguous row of the map (wfs_densify_rows is a row copy), and the convolution is an implicit GEMM whose
// contraction index k = (tap, channel) runs over contiguous memory.  Only the stack's OUTPUT is written channels-first
// (NCHW), the order the reference's view(-1, n_linear) flattens.
//
// The three products of a layer are ONE kernel (k_c2d_gemm), a 64 x 64 output tile per block of 4 waves, 32-deep steps
// staged through LDS, fp32 accumulation on the matrix cores: v_mfma_f32_32x32x16_{bf16,f16} for 16-bit rows,
// v_mfma_f32_32x32x2_f32 for fp32 rows (bitwise an fp32 FMA chain: the 1e-5 bar).  Edges in all three GEMM dimensions
// are masked while the tiles are gathered; nothing is padded in memory.
//   forward  z[m][co]   = sum_k a[m @ tap][ci] Wf[co][k]        M = B H' W', K = fs^2 cin,  N = cout
//   dX       da[m'][ci] = sum_k dz[m' @ tap][co] Wt[ci][k]      M = B H W,   K = fs^2 cout, N = cin
//   dW       dW[co][k]  = sum_m dz[m][co] a[m @ tap][ci]        M = cout,    K = B H' W' in slices of 2048, N = fs^2 cin
// Wf / Wt are the filters repacked in the row type by one launch per direction.  The slices of dW are added in slice
// order by the last launch: no float atomics anywhere, bit-identical reruns.
//
// 16-bit rows, FORWARD: a ReLU mask is a discrete decision, and one mask that differs from an exact run moves dX and
// the few-hundred-term dW sums by a whole term (measured: 7 .. 23 % of the tensor's max with one-piece operands).  So
// the forward keeps the filters in THREE 16-bit pieces (exact to fp32) and the activations between layers in TWO (both
// in the row type; the low pieces scaled by 2048 to stay out of fp16's subnormals) and spends 5 MFMAs per step
// (a1 w1, a2 w1, a1 w2, a1 w3, a2 w2): z is an fp32-accurate product.  The backward products are smooth in their
// operands and take one piece each (dz and the filters rounded to the row type).
//
// Launches.  Forward: 1 (repack) + per layer [conv, statistics partials (training only), BN + ReLU + dropout] =
// 3 layers + 1 in training, 2 layers + 1 in eval mode.  Backward: 1 (repack) + per layer [sums of g and g xhat, dz (and
// the db partials), dX (not for layer 0 unless dX is wanted), dW] + 1 (ordered sums into the gradient slots) =
// 4 layers + 1 without dX, 4 layers + 2 with it.
//
// Statistics per channel over M = B H' W' elements, accumulated, reduced and folded in DOUBLE in a fixed order (row
// lanes, then blocks); see conv1d.hip for why fp64.
#include "wfs_rows.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int TB = 256;
constexpr int MAXC = WFS_CONV2D_MAX_CHANNELS, MAXK = WFS_CONV2D_MAX_K, MAXS = WFS_CONV2D_MAX_STRIDE;
constexpr int MAXD = WFS_CONV2D_MAX_DILATION, MAXLY = WFS_CONV2D_MAX_LAYERS, MAXHW = WFS_CONV2D_MAX_HW;
constexpr int CC = 64;              // channels per block of the row-wise passes (one per lane), 4 row lanes per block
constexpr int RL = TB / CC;
constexpr int NRB_MAX = 256;        // row blocks of a pass that leaves per-block partial sums
constexpr int EW_MAXBLK = 1024;     // row blocks of the BN + ReLU pass
constexpr int TM = 64, TN = 64, TK = 32;      // GEMM tile
constexpr int DW_CHUNK = 2048;      // positions per slice of the dW contraction
constexpr float SPLIT_SCALE = 2048.f;   // the low piece of a 16-bit pair is stored times this (fp16: out of the subnormals)
constexpr int COFF = 64;            // offset that keeps the packed (y, x) origins of the position table positive

// one layer's record of the device pointer table (psd/_fused.py: 7 parameter addresses, then 7 gradient addresses)
struct Conv2dPtrs {
    const float *w, *b, *ga, *be;
    float *rm, *rv;
    long long *nbt;
    float *dw, *db, *dga, *dbe;
    void *unused[3];
};
static_assert(sizeof(Conv2dPtrs) == 14 * sizeof(void *), "pointer record layout");

struct Layer {
    int cin, cout, fs, st, pd, dil, hin, win, hout, wout;
};
struct Plan {
    Layer ly[MAXLY];
    int n;
};

template <typename T>
__device__ __forceinline__ float to_f(T v) {
    return wfs_ld(&v);
}

// ---------------------------------------------------------------------------------------------------------------
// the implicit GEMM
struct GemmArgs {
    Layer ly;
    int layer;          // MODE 0: its record's bias is added
    const void *A, *Bm;  // MODE 0: a_{i-1}, Wf;  MODE 1: dz_i, Wt;  MODE 2: dz_i, a_{i-1}
    const void *A2, *B2; // MODE 0, 16-bit rows: the scaled low pieces of a_{i-1} (NULL: exact in one piece) and of Wf
    const void *B3;      // ... and the filters' third piece (scaled twice)
    void *C;            // MODE 0: z (fp32);  MODE 1: da (fp32) or dX (row type, out_row);  MODE 2: partials (fp32)
    int M, N, K;
    int out_row;
};

template <typename T>
__device__ __forceinline__ f32x16 mfma16(s16x8 a, s16x8 b, f32x16 acc) {
    if constexpr (__is_same(T, wfs_f16))
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), acc, 0,
                                                      0, 0);
    else if constexpr (__is_same(T, wfs_bf16))
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc,
                                                       0, 0, 0);
    else
        return acc;
}

__device__ __forceinline__ int div_st(int v, int st) {       // v >= 0, v < 65536, st in 1 .. 3
    return st == 1 ? v : (st == 2 ? v >> 1 : (v * 43691) >> 17);
}

template <typename T, int MODE>
__global__ void __launch_bounds__(TB) k_c2d_gemm(GemmArgs a, const Conv2dPtrs *__restrict__ pp) {
    constexpr bool F32 = sizeof(T) == 4;
    constexpr int PITCH = F32 ? TK + 1 : TK + 8;         // fp32: dword reads down the rows; 16-bit: 16-byte reads
    __shared__ __attribute__((aligned(16))) T As[TM * PITCH];
    __shared__ __attribute__((aligned(16))) T Bs[TN * PITCH];
    // 16-bit forward: the activations in two pieces, the filters in three (value = p1 + p2 / S + p3 / S^2, S =
    // SPLIT_SCALE): z = a1 w1 + (a2 w1 + a1 w2) / S + (a1 w3 + a2 w2) / S^2 -- the filters exact to fp32, the activations
    // to 2^-18 (bf16) / 2^-22 (fp16), so that the ReLU masks are those of an fp32 run ("16-bit rows")
    constexpr bool SPLIT = MODE == 0 && !F32;
    __shared__ __attribute__((aligned(16))) T As2[SPLIT ? TM * PITCH : 8];
    __shared__ __attribute__((aligned(16))) T Bs2[SPLIT ? TN * PITCH : 8];
    __shared__ __attribute__((aligned(16))) T Bs3[SPLIT ? TN * PITCH : 8];
    __shared__ int2 ptab[MODE == 2 ? DW_CHUNK : 1];
    const Layer ly = a.ly;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, wm = w & 1, wn = w >> 1;
    const int tiles_m = (a.M + TM - 1) / TM;
    const int m0 = ((int)blockIdx.x % tiles_m) * TM, n0 = ((int)blockIdx.x / tiles_m) * TN;
    int k_lo = 0, k_hi = a.K;
    if (MODE == 2) {
        k_lo = (int)blockIdx.z * DW_CHUNK;
        k_hi = k_lo + DW_CHUNK < a.K ? k_lo + DW_CHUNK : a.K;
        const int sp = ly.hout * ly.wout;
        for (int i = t; i < k_hi - k_lo; i += TB) {
            const int pos = k_lo + i, b = pos / sp, rem = pos - b * sp, oy = rem / ly.wout, ox = rem - oy * ly.wout;
            ptab[i] = make_int2(b * ly.hin * ly.win,
                                (oy * ly.st - ly.pd + COFF) | ((ox * ly.st - ly.pd + COFF) << 16));
        }
        __syncthreads();
    }
    const T *Ag = (const T *)a.A, *Bg = (const T *)a.Bm;
    const T *Ag2 = (const T *)a.A2, *Bg2 = (const T *)a.B2, *Bg3 = (const T *)a.B3;
    // ---- what a thread keeps across the steps
    // MODE 0 / 1 (contraction fastest): contraction offset kk = t & 31 of the rows (t >> 5) + 8 j
    // MODE 2 (rows fastest):            row t & 63, contraction offsets (t >> 6) + 4 j
    const int kk = t & 31, r8 = t >> 5, row = t & 63, kq = t >> 6;
    int rb[8], ry[8], rx[8];           // MODE 0 / 1: the A rows' (image base, y origin, x origin)
    long long bn_off[8];               // MODE 0 / 1: the B rows' offsets
    int b_c = 0, b_dy = 0, b_dx = 0;   // MODE 2: the B column's (channel, tap reach)
    bool a_ok = false, b_ok = false;   // MODE 2: row / column inside the matrix
    if (MODE != 2) {
        const int sh = MODE == 0 ? ly.hout : ly.hin, sw = MODE == 0 ? ly.wout : ly.win;      // the output rows' image
        const int th = MODE == 0 ? ly.hin : ly.hout, tw = MODE == 0 ? ly.win : ly.wout;      // the image A is read from
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int m = m0 + r8 + 8 * j;
            if (m < a.M) {
                const int b = m / (sh * sw), rem = m - b * sh * sw, y = rem / sw, x = rem - y * sw;
                rb[j] = b * th * tw;
                ry[j] = MODE == 0 ? y * ly.st - ly.pd : y + ly.pd;
                rx[j] = MODE == 0 ? x * ly.st - ly.pd : x + ly.pd;
            } else {
                rb[j] = 0;
                ry[j] = rx[j] = -(1 << 20);          // fails every bounds test below
            }
            const int n = n0 + r8 + 8 * j;
            bn_off[j] = n < a.N ? (long long)n * a.K : -1;
        }
    } else {
        a_ok = m0 + row < a.M;
        const int n = n0 + row;
        b_ok = n < a.N;
        if (b_ok) {
            const int tap = n / ly.cin, ty = tap / ly.fs;
            b_c = n - tap * ly.cin;
            b_dy = ty * ly.dil;
            b_dx = (tap - ty * ly.fs) * ly.dil;
        }
    }
    T ra[8], rbv[8], ra2[SPLIT ? 8 : 1], rb2[SPLIT ? 8 : 1], rb3[SPLIT ? 8 : 1];
    auto fetch = [&](int k0) {
        if (MODE != 2) {
            const int k = k0 + kk;
            const bool kok = k < k_hi;
            const int cs = MODE == 0 ? ly.cin : ly.cout;
            const int tap = k / cs, c = k - tap * cs, ty = tap / ly.fs, dy = ty * ly.dil, dx = (tap - ty * ly.fs) * ly.dil;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                T v = T{};
                if (MODE == 0) {
                    const int iy = ry[j] + dy, ix = rx[j] + dx;
                    T v2 = T{};
                    if (kok && (unsigned)iy < (unsigned)ly.hin && (unsigned)ix < (unsigned)ly.win) {
                        const long long o = (long long)(rb[j] + iy * ly.win + ix) * ly.cin + c;
                        v = Ag[o];
                        if (SPLIT && Ag2) v2 = Ag2[o];
                    }
                    if constexpr (SPLIT) ra2[j] = v2;
                } else {
                    const int ny = ry[j] - dy, nx = rx[j] - dx;
                    if (kok && ny >= 0 && nx >= 0) {
                        const int oy = div_st(ny, ly.st), ox = div_st(nx, ly.st);
                        if (oy * ly.st == ny && ox * ly.st == nx && oy < ly.hout && ox < ly.wout)
                            v = Ag[(long long)(rb[j] + oy * ly.wout + ox) * ly.cout + c];
                    }
                }
                ra[j] = v;
                rbv[j] = (kok && bn_off[j] >= 0) ? Bg[bn_off[j] + k] : T{};
                if constexpr (SPLIT) {
                    rb2[j] = (kok && bn_off[j] >= 0) ? Bg2[bn_off[j] + k] : T{};
                    rb3[j] = (kok && bn_off[j] >= 0) ? Bg3[bn_off[j] + k] : T{};
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int pos = k0 + kq + 4 * j;
                T va = T{}, vb = T{};
                if (pos < k_hi) {
                    if (a_ok) va = Ag[(long long)pos * ly.cout + m0 + row];
                    if (b_ok) {
                        const int2 e = ptab[pos - k_lo];
                        const int iy = (e.y & 0xFFFF) - COFF + b_dy, ix = (e.y >> 16) - COFF + b_dx;
                        if ((unsigned)iy < (unsigned)ly.hin && (unsigned)ix < (unsigned)ly.win)
                            vb = Bg[(long long)(e.x + iy * ly.win + ix) * ly.cin + b_c];
                    }
                }
                ra[j] = va;
                rbv[j] = vb;
            }
        }
    };
    auto park = [&]() {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int o = MODE != 2 ? (r8 + 8 * j) * PITCH + kk : row * PITCH + kq + 4 * j;
            As[o] = ra[j];
            Bs[o] = rbv[j];
            if constexpr (SPLIT) {
                As2[o] = ra2[j];
                Bs2[o] = rb2[j];
                Bs3[o] = rb3[j];
            }
        }
    };
    f32x16 acc, acc2, acc3;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = acc2[i] = acc3[i] = 0.f;
    const int i32 = lane & 31, h = lane >> 5;
    const T *ar = As + (wm * 32 + i32) * PITCH, *br = Bs + (wn * 32 + i32) * PITCH;
    if (k_lo < k_hi) fetch(k_lo);
    for (int k0 = k_lo; k0 < k_hi; k0 += TK) {
        park();
        __syncthreads();
        if (k0 + TK < k_hi) fetch(k0 + TK);          // in flight under the MFMAs
        if constexpr (F32) {
#pragma unroll
            for (int s = 0; s < TK / 2; ++s)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(to_f(ar[2 * s + h]), to_f(br[2 * s + h]), acc, 0, 0, 0);
        } else {
#pragma unroll
            for (int s = 0; s < TK / 16; ++s) {
                const s16x8 av = *reinterpret_cast<const s16x8 *>(ar + 16 * s + 8 * h);
                const s16x8 bv = *reinterpret_cast<const s16x8 *>(br + 16 * s + 8 * h);
                acc = mfma16<T>(av, bv, acc);
                if constexpr (SPLIT) {
                    const int off = (int)(ar - As) + 16 * s + 8 * h, offb = (int)(br - Bs) + 16 * s + 8 * h;
                    const s16x8 av2 = *reinterpret_cast<const s16x8 *>(As2 + off);
                    const s16x8 bv2 = *reinterpret_cast<const s16x8 *>(Bs2 + offb);
                    acc2 = mfma16<T>(av2, bv, acc2);
                    acc2 = mfma16<T>(av, bv2, acc2);
                    acc3 = mfma16<T>(av, *reinterpret_cast<const s16x8 *>(Bs3 + offb), acc3);
                    acc3 = mfma16<T>(av2, bv2, acc3);
                }
            }
        }
        __syncthreads();
    }
    // C/D map of the 32 x 32 MFMA: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const int n = n0 + wn * 32 + i32;
    if (n >= a.N) return;
    float bias = 0.f;
    if (MODE == 0) {
        const float *bp = pp[a.layer].b;
        if (bp) bias = bp[n];
    }
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int m = m0 + wm * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        if (m >= a.M) continue;
        const long long o = ((long long)(MODE == 2 ? (int)blockIdx.z * a.M : 0) + m) * a.N + n;
        if (MODE == 1 && a.out_row)
            wfs_st((T *)a.C + o, acc[reg]);
        else
            ((float *)a.C)[o] = (SPLIT ? acc[reg] + (acc2[reg] + acc3[reg] * (1.f / SPLIT_SCALE)) * (1.f / SPLIT_SCALE) : acc[reg]) + bias;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// filters [cout][cin][taps] (fp32) -> Wf [cout][taps][cin] (forward) or Wt [cin][taps][cout] (dX), in the row type
struct PackDesc {
    int cin, cout, taps;
    long long off;       // element offset of the layer's block in the packed buffer
};
struct PackTable {
    PackDesc d[MAXLY];
};
template <typename T>
__global__ void __launch_bounds__(TB) k_c2d_pack(const Conv2dPtrs *__restrict__ pp, PackTable tab, T *__restrict__ out,
                                                 T *__restrict__ out_lo, T *__restrict__ out_lo2, int transpose) {
    const PackDesc d = tab.d[blockIdx.y];
    const float *w = pp[blockIdx.y].w;
    const long long total = (long long)d.cin * d.cout * d.taps;
    for (long long i = (long long)blockIdx.x * TB + threadIdx.x; i < total; i += (long long)gridDim.x * TB) {
        int co, ci, tap;
        if (!transpose) {
            ci = (int)(i % d.cin);
            tap = (int)((i / d.cin) % d.taps);
            co = (int)(i / ((long long)d.cin * d.taps));
        } else {
            co = (int)(i % d.cout);
            tap = (int)((i / d.cout) % d.taps);
            ci = (int)(i / ((long long)d.cout * d.taps));
        }
        const float v = w[((long long)co * d.cin + ci) * d.taps + tap];
        wfs_st(out + d.off + i, v);
        if (out_lo) {
            const float r1 = (v - wfs_ld(out + d.off + i)) * SPLIT_SCALE;           // exact: a power-of-two scale
            wfs_st(out_lo + d.off + i, r1);
            wfs_st(out_lo2 + d.off + i, (r1 - wfs_ld(out_lo + d.off + i)) * SPLIT_SCALE);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// row-wise passes over a map [M][C]: thread = (row lane t / 64, channel chunk * 64 + t % 64)

// the block's (s, q) of its channels: row lanes added in lane order -> part[(blockIdx.x * C + c) * 2 + {0, 1}]
__device__ __forceinline__ void lanes_to_part(double s, double q, double (*red)[CC][2], double *part, int C, int c) {
    const int rl = threadIdx.x / CC, cl = threadIdx.x % CC;
    red[rl][cl][0] = s;
    red[rl][cl][1] = q;
    __syncthreads();
    if (rl == 0 && c < C) {
        double ts = red[0][cl][0], tq = red[0][cl][1];
#pragma unroll
        for (int r = 1; r < RL; ++r) {
            ts += red[r][cl][0];
            tq += red[r][cl][1];
        }
        part[((long long)blockIdx.x * C + c) * 2] = ts;
        part[((long long)blockIdx.x * C + c) * 2 + 1] = tq;
    }
}

// totals of the partials [nblk][C][2] of this block's channels, the same order in every block: row lane r adds the
// partials r, r + RL, ..., then the lanes are added in lane order.  Result in tot[cl][2] (all threads may read it).
__device__ __forceinline__ void fold(const double *__restrict__ part, int nblk, int C, int c, double (*red)[CC][2],
                                     double (*tot)[2]) {
    const int rl = threadIdx.x / CC, cl = threadIdx.x % CC;
    double s = 0.0, q = 0.0;
    if (c < C)
        for (int p = rl; p < nblk; p += RL) {
            s += part[((long long)p * C + c) * 2];
            q += part[((long long)p * C + c) * 2 + 1];
        }
    red[rl][cl][0] = s;
    red[rl][cl][1] = q;
    __syncthreads();
    if (rl == 0) {
        double ts = red[0][cl][0], tq = red[0][cl][1];
#pragma unroll
        for (int r = 1; r < RL; ++r) {
            ts += red[r][cl][0];
            tq += red[r][cl][1];
        }
        tot[cl][0] = ts;
        tot[cl][1] = tq;
    }
    __syncthreads();
}

__global__ void __launch_bounds__(TB) k_c2d_stats(const float *__restrict__ Z, int M, int C, double *__restrict__ part) {
    __shared__ double red[RL][CC][2];
    const int rl = threadIdx.x / CC, c = blockIdx.y * CC + threadIdx.x % CC;
    double s = 0.0, q = 0.0;
    if (c < C)
        for (int r = blockIdx.x * RL + rl; r < M; r += gridDim.x * RL) {
            const double v = (double)Z[(long long)r * C + c];
            s += v;
            q += v * v;
        }
    lanes_to_part(s, q, red, part, C, c);
}

struct ApplyArgs {
    const float *Z;
    int M, C, sp;        // sp = H' W'
    int layer;
    const double *part;
    int nblk;
    float momentum, eps;
    int training;
    float *stats_out;    // [2][MAXC] mean / invstd, for the backward
    void *out, *out_lo;  // out_lo: the scaled low pieces of a 16-bit activation (NULL: none)
    int out_dt, nchw;    // the next layer's input [M][C], or the stack's output [B][C][H'][W']
    float p;
    const long long *seed_dev;
};

// element counter of the dropout generator: layer << 44 | flat index of the element in the layer's output AS NCHW
__device__ __forceinline__ unsigned long long drop_ctr(int layer, int r, int c, int C, int sp) {
    const int b = r / sp, hw = r - b * sp;
    return ((unsigned long long)layer << 44) | (unsigned long long)(((long long)b * C + c) * sp + hw);
}

__global__ void __launch_bounds__(TB) k_c2d_apply(ApplyArgs a, const Conv2dPtrs *__restrict__ pp) {
    __shared__ double red[RL][CC][2], tot[CC][2];
    const int rl = threadIdx.x / CC, cl = threadIdx.x % CC, c = blockIdx.y * CC + cl;
    const Conv2dPtrs p = pp[a.layer];
    float mean = 0.f, inv = 0.f;
    if (a.training) {
        fold(a.part, a.nblk, a.C, c, red, tot);
        if (c < a.C) {
            const double cnt = (double)a.M, md = tot[cl][0] / cnt;
            double var = tot[cl][1] / cnt - md * md;            // biased, what torch normalises with
            var = var > 0.0 ? var : 0.0;
            mean = (float)md;
            inv = (float)(1.0 / sqrt(var + (double)a.eps));
            if (blockIdx.x == 0 && rl == 0 && p.rm && p.rv) {
                const float unbiased = (float)(a.M > 1 ? var * (cnt / (cnt - 1.0)) : var);
                p.rm[c] = (1.f - a.momentum) * p.rm[c] + a.momentum * mean;
                p.rv[c] = (1.f - a.momentum) * p.rv[c] + a.momentum * unbiased;
            }
        }
        if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && p.nbt) *p.nbt += 1;
    } else if (c < a.C) {
        mean = p.rm[c];
        inv = (float)(1.0 / sqrt((double)p.rv[c] + (double)a.eps));
    }
    if (c >= a.C) return;
    if (blockIdx.x == 0 && rl == 0) {
        a.stats_out[c] = mean;
        a.stats_out[MAXC + c] = inv;
    }
    const float ga = p.ga[c], be = p.be[c];
    const Drop dr = make_drop(a.training ? a.p : 0.f, a.seed_dev);
    for (int r = blockIdx.x * RL + rl; r < a.M; r += gridDim.x * RL) {
        float y = fmaf(ga, (a.Z[(long long)r * a.C + c] - mean) * inv, be);
        y = y > 0.f ? y : 0.f;
        if (dr.on) y *= wfs_drop_mult(dr, drop_ctr(a.layer, r, c, a.C, a.sp));
        long long o = (long long)r * a.C + c;
        if (a.nchw) {
            const int b = r / a.sp;
            o = ((long long)b * a.C + c) * a.sp + (r - b * a.sp);
        }
        stt(a.out, o, a.out_dt, y);
        if (a.out_lo) stt(a.out_lo, o, a.out_dt, (y - ldt(a.out, o, a.out_dt)) * SPLIT_SCALE);
    }
}

struct BnBwdArgs {
    const float *Z;
    const void *dA;      // gradient of the layer's output: dY [B][C][H'][W'] (row type, nchw) or da [M][C] (fp32)
    int da_dt, nchw;
    int M, C, sp, layer;
    const float *stats;  // [2][MAXC]
    int training;
    float p;
    const long long *seed_dev;
    double *gpart;       // [gridDim.x][C][2] partials of (sum g, sum g xhat)
    int gnblk;
    void *DZ;            // [M][C] row type
    int dz_dt;
    double *dbpart;      // [gridDim.x][C][2] partials of (sum dz, unused)
};

// g = dA x dropout multiplier x [y > 0], and xhat
__device__ __forceinline__ float grad_in(const BnBwdArgs &a, const Drop &dr, int r, int c, float mean, float inv, float ga,
                                         float be, float &xh) {
    xh = (a.Z[(long long)r * a.C + c] - mean) * inv;
    if (!(fmaf(ga, xh, be) > 0.f)) return 0.f;
    long long o = (long long)r * a.C + c;
    if (a.nchw) {
        const int b = r / a.sp;
        o = ((long long)b * a.C + c) * a.sp + (r - b * a.sp);
    }
    float g = ldt(a.dA, o, a.da_dt);
    if (dr.on) g *= wfs_drop_mult(dr, drop_ctr(a.layer, r, c, a.C, a.sp));
    return g;
}

__global__ void __launch_bounds__(TB) k_c2d_gsum(BnBwdArgs a, const Conv2dPtrs *__restrict__ pp) {
    __shared__ double red[RL][CC][2];
    const int rl = threadIdx.x / CC, c = blockIdx.y * CC + threadIdx.x % CC;
    const Conv2dPtrs p = pp[a.layer];
    const Drop dr = make_drop(a.training ? a.p : 0.f, a.seed_dev);
    double s = 0.0, q = 0.0;
    if (c < a.C) {
        const float mean = a.stats[c], inv = a.stats[MAXC + c], ga = p.ga[c], be = p.be[c];
        for (int r = blockIdx.x * RL + rl; r < a.M; r += gridDim.x * RL) {
            float xh;
            const float g = grad_in(a, dr, r, c, mean, inv, ga, be, xh);
            s += (double)g;
            q += (double)g * (double)xh;
        }
    }
    lanes_to_part(s, q, red, a.gpart, a.C, c);
}

__global__ void __launch_bounds__(TB) k_c2d_dz(BnBwdArgs a, const Conv2dPtrs *__restrict__ pp) {
    __shared__ double red[RL][CC][2], tot[CC][2];
    const int rl = threadIdx.x / CC, cl = threadIdx.x % CC, c = blockIdx.y * CC + cl;
    const Conv2dPtrs p = pp[a.layer];
    const Drop dr = make_drop(a.training ? a.p : 0.f, a.seed_dev);
    fold(a.gpart, a.gnblk, a.C, c, red, tot);
    double s = 0.0;
    if (c < a.C) {
        if (blockIdx.x == 0 && rl == 0) {
            if (p.dbe) p.dbe[c] = (float)tot[cl][0];
            if (p.dga) p.dga[c] = (float)tot[cl][1];
        }
        const float k1 = a.training ? (float)(tot[cl][0] / (double)a.M) : 0.f;
        const float k2 = a.training ? (float)(tot[cl][1] / (double)a.M) : 0.f;
        const float mean = a.stats[c], inv = a.stats[MAXC + c], ga = p.ga[c], be = p.be[c], coef = ga * inv;
        for (int r = blockIdx.x * RL + rl; r < a.M; r += gridDim.x * RL) {
            float xh;
            const float g = grad_in(a, dr, r, c, mean, inv, ga, be, xh);
            const float dz = coef * (g - k1 - xh * k2);
            stt(a.DZ, (long long)r * a.C + c, a.dz_dt, dz);
            s += (double)dz;
        }
    }
    __syncthreads();
    lanes_to_part(s, 0.0, red, a.dbpart, a.C, c);
}

// block (layer, output channel): the dW slices added in slice order (in double) into conv.weight's gradient, laid out
// [cout][cin][taps]; the db partials into conv.bias's
struct DwDesc {
    int cin, cout, taps, nslice, nrb;
    long long p_off, db_off;      // float offsets from the first layer's partials / double offsets from the first db block
};
struct DwTable {
    DwDesc d[MAXLY];
};
__global__ void __launch_bounds__(TB) k_c2d_dw_reduce(const Conv2dPtrs *__restrict__ pp, DwTable tab,
                                                      const float *__restrict__ part, const double *__restrict__ dbpart) {
    const DwDesc d = tab.d[blockIdx.x];
    const int co = blockIdx.y;
    if (co >= d.cout) return;
    const Conv2dPtrs p = pp[blockIdx.x];
    const int ncol = d.cin * d.taps;
    if (p.dw) {
        const float *q0 = part + d.p_off + (long long)co * ncol;
        for (int q = threadIdx.x; q < ncol; q += TB) {
            double s = 0.0;
            for (int z = 0; z < d.nslice; ++z) s += (double)q0[(long long)z * d.cout * ncol + q];
            const int tap = q / d.cin, ci = q - tap * d.cin;
            p.dw[((long long)co * d.cin + ci) * d.taps + tap] = (float)s;
        }
    }
    if (p.db && threadIdx.x == 0) {
        double s = 0.0;
        for (int b = 0; b < d.nrb; ++b) s += dbpart[d.db_off + ((long long)b * d.cout + co) * 2];
        p.db[co] = (float)s;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// rows [n][C] at coords (x, y, event) -> map [B][H][W][C].  Block (event, x): finds its rows, then writes its W cells.
template <typename T>
__global__ void __launch_bounds__(TB) k_densify(const T *__restrict__ rows, const int *__restrict__ coords, long long n_cap,
                                                int C, int H, int W, const long long *__restrict__ n_dev,
                                                T *__restrict__ out) {
    __shared__ int first[MAXHW], count[MAXHW];
    const int b = blockIdx.x, x = blockIdx.y;
    const long long n = wfs_valid_rows_nonneg(n_cap, n_dev);
    if (threadIdx.x < MAXHW) {
        first[threadIdx.x] = 0x7FFFFFFF;
        count[threadIdx.x] = 0;
    }
    __syncthreads();
    for (long long r = threadIdx.x; r < n; r += TB) {
        const int cx = coords[r * 3], cy = coords[r * 3 + 1], ce = coords[r * 3 + 2];
        if (ce == b && cx == x && cy >= 0 && cy < W) {
            atomicMin(&first[cy], (int)r);
            atomicAdd(&count[cy], 1);
        }
    }
    __syncthreads();
    for (int y = 0; y < W; ++y) {
        T *o = out + (((long long)b * H + x) * W + y) * C;
        const int cnt = count[y];
        if (cnt == 0) {
            for (int c = threadIdx.x; c < C; c += TB) o[c] = T{};
        } else if (cnt == 1) {
            const T *src = rows + (long long)first[y] * C;
            for (int c = threadIdx.x; c < C; c += TB) o[c] = src[c];
        } else {
            // equal coordinates: summed in row order (fp32, rounded once)
            for (int c = threadIdx.x; c < C; c += TB) {
                float s = 0.f;
                for (long long r = first[y]; r < n; ++r)
                    if (coords[r * 3] == x && coords[r * 3 + 1] == y && coords[r * 3 + 2] == b)
                        s += to_f(rows[r * C + c]);
                wfs_st(o + c, s);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
int make_plan(int32_t c0, const int32_t *channels, const int32_t *fs, const int32_t *st, const int32_t *pd,
              const int32_t *dil, int32_t layers, int32_t H, int32_t W, Plan *pl) {
    WFS_REQUIRE(layers >= 1 && layers <= MAXLY, WFS_EINVAL, "conv2d stack of %d layers: 1 .. %d supported", layers, MAXLY);
    WFS_REQUIRE(channels && fs && st && pd && dil, WFS_EINVAL, "NULL layer description");
    WFS_REQUIRE(c0 >= 1 && c0 <= MAXC, WFS_EINVAL, "conv2d stack input of %d channels: 1 .. %d supported", c0, MAXC);
    WFS_REQUIRE(H >= 1 && H <= MAXHW && W >= 1 && W <= MAXHW, WFS_EINVAL, "map %d x %d: 1 .. %d supported", H, W, MAXHW);
    int cin = c0, hin = H, win = W;
    for (int i = 0; i < layers; ++i) {
        WFS_REQUIRE(channels[i] >= 1 && channels[i] <= MAXC, WFS_EINVAL, "conv2d layer %d has %d channels: 1 .. %d supported",
                    i, channels[i], MAXC);
        WFS_REQUIRE(fs[i] >= 1 && fs[i] <= MAXK, WFS_EINVAL, "conv2d layer %d kernel size %d: 1 .. %d supported", i, fs[i], MAXK);
        WFS_REQUIRE(st[i] >= 1 && st[i] <= MAXS, WFS_EINVAL, "conv2d layer %d stride %d: 1 .. %d supported", i, st[i], MAXS);
        WFS_REQUIRE(dil[i] >= 1 && dil[i] <= MAXD, WFS_EINVAL, "conv2d layer %d dilation %d: 1 .. %d supported", i, dil[i], MAXD);
        const int reach = dil[i] * (fs[i] - 1);
        WFS_REQUIRE(pd[i] >= 0 && pd[i] <= reach, WFS_EINVAL, "conv2d layer %d padding %d: 0 .. dilation x (kernel - 1) = %d supported",
                    i, pd[i], reach);
        const int nh = hin + 2 * pd[i] - reach - 1, nw = win + 2 * pd[i] - reach - 1;
        WFS_REQUIRE(nh >= 0 && nw >= 0, WFS_EINVAL, "conv2d layer %d: kernel reach %d does not fit %d x %d + 2 x %d", i, reach + 1,
                    hin, win, pd[i]);
        Layer &ly = pl->ly[i];
        ly.cin = cin;
        ly.cout = channels[i];
        ly.fs = fs[i];
        ly.st = st[i];
        ly.pd = pd[i];
        ly.dil = dil[i];
        ly.hin = hin;
        ly.win = win;
        ly.hout = nh / st[i] + 1;
        ly.wout = nw / st[i] + 1;
        cin = ly.cout;
        hin = ly.hout;
        win = ly.wout;
    }
    pl->n = layers;
    return WFS_OK;
}

int check_common(int32_t c0, const int32_t *channels, const int32_t *fs, const int32_t *st, const int32_t *pd,
                 const int32_t *dil, int32_t layers, int64_t B, int32_t H, int32_t W, int32_t training, int32_t dtype,
                 Plan *pl) {
    int rc = make_plan(c0, channels, fs, st, pd, dil, layers, H, W, pl);
    if (rc != WFS_OK) return rc;
    WFS_REQUIRE(B >= 1 && B <= WFS_CONV2D_MAX_BATCH, WFS_EINVAL, "%lld events: 1 .. %d supported", (long long)B,
                WFS_CONV2D_MAX_BATCH);
    WFS_REQUIRE(wfs_dtype_ok(dtype), WFS_EINVAL, "bad dtype %d", dtype);
    if (training)
        for (int i = 0; i < layers; ++i)
            WFS_REQUIRE(B * pl->ly[i].hout * pl->ly[i].wout >= 2, WFS_EINVAL,
                        "conv2d layer %d: batch statistics need more than one value per channel", i);
    return WFS_OK;
}

// row_blocks and its two caps, launch_gemm's tile counts and work_layout's nslice are restated by wfs_conv2d_arms
// (the tests read from it which arm a case reaches): change them together.
size_t as_floats(size_t elems, int dtype) { return ((elems * wfs_dtype_bytes(dtype) + 7) / 8) * 2; }     // 8-byte granules
int row_blocks(long long M, int cap) {
    long long b = (M + 4 * RL - 1) / (4 * RL);
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}
long long rows_of(const Layer &ly, long long B) { return B * ly.hout * ly.wout; }

// `saved` (floats): z of every layer | [layers][2][MAXC] mean / invstd | the statistics partials (doubles) | the
// activations a_0 .. a_{n-2} (row type) | Wf of every layer (row type)
struct SavedLayout {
    size_t z[MAXLY], stats, part[MAXLY], act[MAXLY], act_lo[MAXLY], wf, wf_lo, wf_lo2, wf_layer[MAXLY], total;
};
SavedLayout saved_layout(const Plan &pl, long long B, int dtype) {
    SavedLayout s;
    size_t off = 0;
    for (int i = 0; i < pl.n; ++i) {
        s.z[i] = off;
        off += ((size_t)rows_of(pl.ly[i], B) * pl.ly[i].cout + 1) & ~(size_t)1;
    }
    s.stats = off;
    off += (size_t)pl.n * 2 * MAXC;
    for (int i = 0; i < pl.n; ++i) {
        s.part[i] = off;
        off += 2 * (size_t)row_blocks(rows_of(pl.ly[i], B), NRB_MAX) * 2 * pl.ly[i].cout;
    }
    for (int i = 0; i < pl.n; ++i) {
        s.act[i] = s.act_lo[i] = off;
        if (i + 1 < pl.n) {
            off += as_floats((size_t)rows_of(pl.ly[i], B) * pl.ly[i].cout, dtype);
            s.act_lo[i] = off;
            if (dtype != WFS_F32) off += as_floats((size_t)rows_of(pl.ly[i], B) * pl.ly[i].cout, dtype);
        }
    }
    s.wf = off;
    size_t we = 0;
    for (int i = 0; i < pl.n; ++i) {
        s.wf_layer[i] = we;
        we += ((size_t)pl.ly[i].cin * pl.ly[i].cout * pl.ly[i].fs * pl.ly[i].fs + 7) & ~(size_t)7;       // 16-byte granules
    }
    off += as_floats(we, dtype);
    s.wf_lo = off;
    if (dtype != WFS_F32) off += as_floats(we, dtype);
    s.wf_lo2 = off;
    if (dtype != WFS_F32) off += as_floats(we, dtype);
    s.total = off;
    return s;
}

// backward workspace (floats): da ping-pong (fp32) | dz (row type) | g partials, db partials of every layer (doubles) |
// Wt of every layer (row type) | dW slices of every layer
struct WorkLayout {
    size_t da[2], dz, gpart, dbpart[MAXLY], wt, wt_layer[MAXLY], part[MAXLY], total;
    int nslice[MAXLY];
};
WorkLayout work_layout(const Plan &pl, long long B, int dtype) {
    WorkLayout w;
    size_t amax = 0;
    for (int i = 0; i < pl.n; ++i) {
        const size_t e = (size_t)rows_of(pl.ly[i], B) * pl.ly[i].cout;
        amax = e > amax ? e : amax;
    }
    amax = (amax + 1) & ~(size_t)1;
    w.da[0] = 0;
    w.da[1] = amax;
    w.dz = 2 * amax;
    size_t off = w.dz + as_floats(amax, dtype);
    w.gpart = off;
    off += 2 * (size_t)NRB_MAX * 2 * MAXC;
    for (int i = 0; i < pl.n; ++i) {
        w.dbpart[i] = off;
        off += 2 * (size_t)row_blocks(rows_of(pl.ly[i], B), NRB_MAX) * 2 * pl.ly[i].cout;
    }
    w.wt = off;
    size_t we = 0;
    for (int i = 0; i < pl.n; ++i) {
        w.wt_layer[i] = we;
        we += ((size_t)pl.ly[i].cin * pl.ly[i].cout * pl.ly[i].fs * pl.ly[i].fs + 7) & ~(size_t)7;
    }
    off += as_floats(we, dtype);
    for (int i = 0; i < pl.n; ++i) {
        const Layer &ly = pl.ly[i];
        w.nslice[i] = (int)((rows_of(ly, B) + DW_CHUNK - 1) / DW_CHUNK);
        w.part[i] = off;
        off += (size_t)w.nslice[i] * ly.cout * ly.cin * ly.fs * ly.fs;
    }
    w.total = off;
    return w;
}

template <typename T, int MODE>
void launch_gemm(const GemmArgs &a, const Conv2dPtrs *pp, int nz, hipStream_t stream) {
    const unsigned tiles = (unsigned)(((a.M + TM - 1) / TM) * ((a.N + TN - 1) / TN));
    k_c2d_gemm<T, MODE><<<dim3(tiles, 1, (unsigned)nz), dim3(TB), 0, stream>>>(a, pp);
}
template <int MODE>
void launch_gemm_dt(int dtype, const GemmArgs &a, const Conv2dPtrs *pp, int nz, hipStream_t stream) {
    wfs_with_dtype(dtype, [&](auto t) -> int {
        launch_gemm<decltype(t), MODE>(a, pp, nz, stream);
        return WFS_OK;
    });
}

void launch_pack(int dtype, const Plan &pl, const size_t *layer_off, const Conv2dPtrs *pp, void *out, void *out_lo,
                 void *out_lo2, int transpose, hipStream_t stream) {
    PackTable tab = {};
    size_t most = 1;
    for (int i = 0; i < pl.n; ++i) {
        const Layer &ly = pl.ly[i];
        tab.d[i].cin = ly.cin;
        tab.d[i].cout = ly.cout;
        tab.d[i].taps = ly.fs * ly.fs;
        tab.d[i].off = (long long)layer_off[i];
        const size_t e = (size_t)ly.cin * ly.cout * ly.fs * ly.fs;
        most = e > most ? e : most;
    }
    size_t blocks = (most + TB - 1) / TB;
    blocks = blocks > 512 ? 512 : blocks;
    const dim3 grid((unsigned)blocks, (unsigned)pl.n);
    if (dtype == WFS_F32)
        k_c2d_pack<float><<<grid, dim3(TB), 0, stream>>>(pp, tab, (float *)out, (float *)nullptr, (float *)nullptr, transpose);
    else if (dtype == WFS_BF16)
        k_c2d_pack<wfs_bf16><<<grid, dim3(TB), 0, stream>>>(pp, tab, (wfs_bf16 *)out, (wfs_bf16 *)out_lo, (wfs_bf16 *)out_lo2,
                                                           transpose);
    else
        k_c2d_pack<wfs_f16><<<grid, dim3(TB), 0, stream>>>(pp, tab, (wfs_f16 *)out, (wfs_f16 *)out_lo, (wfs_f16 *)out_lo2, transpose);
}

int check_dropout(const float *dropout_p, int layers, const int64_t *seed_dev) {
    if (!dropout_p) return WFS_OK;
    for (int i = 0; i < layers; ++i) WFS_REQUIRE_DROPOUT(dropout_p[i], seed_dev);
    return WFS_OK;
}

}  // namespace

extern "C" int wfs_conv2d_ok(int32_t c0, const int32_t *channels, const int32_t *fs, const int32_t *st, const int32_t *pd,
                             const int32_t *dil, int32_t layers, int64_t B, int32_t H, int32_t W, int32_t training,
                             int32_t dtype) {
    Plan pl;
    return check_common(c0, channels, fs, st, pd, dil, layers, B, H, W, training, dtype, &pl);
}

extern "C" size_t wfs_conv2d_saved_floats(int64_t B, int32_t H, int32_t W, int32_t c0, const int32_t *channels,
                                          const int32_t *fs, const int32_t *st, const int32_t *pd, const int32_t *dil,
                                          int32_t layers, int32_t dtype) {
    Plan pl;
    if (check_common(c0, channels, fs, st, pd, dil, layers, B, H, W, 0, dtype, &pl) != WFS_OK) return 0;
    return saved_layout(pl, B, dtype).total;
}

extern "C" size_t wfs_conv2d_bwd_workspace_floats(int64_t B, int32_t H, int32_t W, int32_t c0, const int32_t *channels,
                                                  const int32_t *fs, const int32_t *st, const int32_t *pd,
                                                  const int32_t *dil, int32_t layers, int32_t dtype) {
    Plan pl;
    if (check_common(c0, channels, fs, st, pd, dil, layers, B, H, W, 0, dtype, &pl) != WFS_OK) return 0;
    return work_layout(pl, B, dtype).total;
}

// Host only, launches nothing: what the launches below do with every layer of the plan, out[layers][8] =
//   {M = B H' W', row blocks of the statistics / g-sum / dz passes, row blocks of the BN + ReLU pass,
//    forward GEMM tiles along M, along N, its K steps, dW slices, positions in the last slice}
// tests/test_dense_cases_host.py takes from here which arm a case of its table reaches.  Built from the helpers the
// launches use (row_blocks with NRB_MAX / EW_MAXBLK, launch_gemm's tile counts, the step count of k_c2d_gemm's loop,
// work_layout's nslice): change it together with them.  Refuses what wfs_conv2d_ok refuses for an eval call (there is
// no `training` here, as in the two size queries).
extern "C" int wfs_conv2d_arms(int64_t B, int32_t H, int32_t W, int32_t c0, const int32_t *channels, const int32_t *fs,
                               const int32_t *st, const int32_t *pd, const int32_t *dil, int32_t layers, int32_t dtype,
                               int32_t *out) {
    Plan pl;
    int rc = check_common(c0, channels, fs, st, pd, dil, layers, B, H, W, 0, dtype, &pl);
    if (rc != WFS_OK) return rc;
    WFS_REQUIRE(out, WFS_EINVAL, "NULL output");
    const WorkLayout wl = work_layout(pl, B, dtype);
    for (int i = 0; i < layers; ++i) {
        const Layer &ly = pl.ly[i];
        const long long M = rows_of(ly, B);
        const int K = ly.cin * ly.fs * ly.fs;
        int32_t *o = out + 8 * i;
        o[0] = (int32_t)M;
        o[1] = row_blocks(M, NRB_MAX);
        o[2] = row_blocks(M, EW_MAXBLK);
        o[3] = (int32_t)((M + TM - 1) / TM);
        o[4] = (ly.cout + TN - 1) / TN;
        o[5] = (K + TK - 1) / TK;
        o[6] = wl.nslice[i];
        o[7] = (int32_t)(M - (long long)(wl.nslice[i] - 1) * DW_CHUNK);
    }
    return WFS_OK;
}

extern "C" int wfs_conv2d_fwd(const void *X, int64_t B, int32_t H, int32_t W, int32_t c0, const int32_t *channels,
                              const int32_t *fs, const int32_t *st, const int32_t *pd, const int32_t *dil, int32_t layers,
                              const void *param_ptrs, const float *momentum, const float *eps, const float *dropout_p,
                              const int64_t *seed_dev, int32_t training, float *saved, void *Y, int32_t dtype,
                              void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    Plan pl;
    int rc = check_common(c0, channels, fs, st, pd, dil, layers, B, H, W, training, dtype, &pl);
    if (rc != WFS_OK) return rc;
    WFS_REQUIRE(momentum && eps, WFS_EINVAL, "NULL momentum / eps list");
    for (int i = 0; i < layers; ++i)
        WFS_REQUIRE(momentum[i] >= 0.f && momentum[i] <= 1.f && eps[i] >= 0.f, WFS_EINVAL,
                    "BatchNorm of layer %d: momentum %g, eps %g", i, (double)momentum[i], (double)eps[i]);
    rc = check_dropout(dropout_p, layers, seed_dev);
    if (rc != WFS_OK) return rc;
    WFS_REQUIRE(X && param_ptrs && saved && Y, WFS_EINVAL, "NULL device pointer");
    const SavedLayout sl = saved_layout(pl, B, dtype);
    const Conv2dPtrs *pp = (const Conv2dPtrs *)param_ptrs;
    const int es = wfs_dtype_bytes(dtype);
    char *wf = (char *)(saved + sl.wf);
    const bool split = dtype != WFS_F32;
    char *wf_lo = (char *)(saved + sl.wf_lo);
    char *wf_lo2 = (char *)(saved + sl.wf_lo2);
    launch_pack(dtype, pl, sl.wf_layer, pp, wf, split ? wf_lo : nullptr, split ? wf_lo2 : nullptr, 0, stream);
    WFS_LAUNCH_CHECK();
    for (int i = 0; i < layers; ++i) {
        const Layer &ly = pl.ly[i];
        const int M = (int)rows_of(ly, B);
        GemmArgs g = {};
        g.ly = ly;
        g.layer = i;
        g.A = i == 0 ? X : (const void *)(saved + sl.act[i - 1]);
        g.Bm = wf + sl.wf_layer[i] * es;
        g.A2 = (split && i > 0) ? (const void *)(saved + sl.act_lo[i - 1]) : nullptr;      // the rows are exact in one piece
        g.B2 = split ? wf_lo + sl.wf_layer[i] * es : nullptr;
        g.B3 = split ? wf_lo2 + sl.wf_layer[i] * es : nullptr;
        g.C = saved + sl.z[i];
        g.M = M;
        g.N = ly.cout;
        g.K = ly.cin * ly.fs * ly.fs;
        launch_gemm_dt<0>(dtype, g, pp, 1, stream);
        WFS_LAUNCH_CHECK();
        const unsigned chunks = (unsigned)((ly.cout + CC - 1) / CC);
        const int nrb = row_blocks(M, NRB_MAX);
        if (training) {
            k_c2d_stats<<<dim3((unsigned)nrb, chunks), dim3(TB), 0, stream>>>(saved + sl.z[i], M, ly.cout,
                                                                             (double *)(saved + sl.part[i]));
            WFS_LAUNCH_CHECK();
        }
        ApplyArgs a = {};
        a.Z = saved + sl.z[i];
        a.M = M;
        a.C = ly.cout;
        a.sp = ly.hout * ly.wout;
        a.layer = i;
        a.part = (const double *)(saved + sl.part[i]);
        a.nblk = nrb;
        a.momentum = momentum[i];
        a.eps = eps[i];
        a.training = training;
        a.stats_out = saved + sl.stats + (size_t)i * 2 * MAXC;
        a.out = i + 1 < layers ? (void *)(saved + sl.act[i]) : Y;
        a.out_lo = (split && i + 1 < layers) ? (void *)(saved + sl.act_lo[i]) : nullptr;
        a.out_dt = dtype;
        a.nchw = i + 1 == layers;
        a.p = dropout_p ? dropout_p[i] : 0.f;
        a.seed_dev = (const long long *)seed_dev;
        k_c2d_apply<<<dim3((unsigned)row_blocks(M, EW_MAXBLK), chunks), dim3(TB), 0, stream>>>(a, pp);
        WFS_LAUNCH_CHECK();
    }
    return WFS_OK;
}

extern "C" int wfs_conv2d_bwd(const void *X, const void *dY, int64_t B, int32_t H, int32_t W, int32_t c0,
                              const int32_t *channels, const int32_t *fs, const int32_t *st, const int32_t *pd,
                              const int32_t *dil, int32_t layers, const void *param_ptrs, const float *dropout_p,
                              const int64_t *seed_dev, int32_t training, const float *saved, void *dX, float *workspace,
                              int32_t dtype, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    Plan pl;
    int rc = check_common(c0, channels, fs, st, pd, dil, layers, B, H, W, training, dtype, &pl);
    if (rc != WFS_OK) return rc;
    rc = check_dropout(dropout_p, layers, seed_dev);
    if (rc != WFS_OK) return rc;
    WFS_REQUIRE(X && dY && param_ptrs && saved && workspace, WFS_EINVAL, "NULL device pointer");
    const SavedLayout sl = saved_layout(pl, B, dtype);
    const WorkLayout wl = work_layout(pl, B, dtype);
    const Conv2dPtrs *pp = (const Conv2dPtrs *)param_ptrs;
    const int es = wfs_dtype_bytes(dtype);
    char *wt = (char *)(workspace + wl.wt);
    launch_pack(dtype, pl, wl.wt_layer, pp, wt, nullptr, nullptr, 1, stream);
    WFS_LAUNCH_CHECK();
    DwTable tab = {};
    int maxc = 0, cur = 0;
    for (int i = layers - 1; i >= 0; --i) {
        const Layer &ly = pl.ly[i];
        const int M = (int)rows_of(ly, B);
        const unsigned chunks = (unsigned)((ly.cout + CC - 1) / CC);
        const int nrb = row_blocks(M, NRB_MAX);
        BnBwdArgs b = {};
        b.Z = saved + sl.z[i];
        b.dA = i == layers - 1 ? dY : (const void *)(workspace + wl.da[cur]);
        b.da_dt = i == layers - 1 ? dtype : WFS_F32;
        b.nchw = i == layers - 1;
        b.M = M;
        b.C = ly.cout;
        b.sp = ly.hout * ly.wout;
        b.layer = i;
        b.stats = saved + sl.stats + (size_t)i * 2 * MAXC;
        b.training = training;
        b.p = dropout_p ? dropout_p[i] : 0.f;
        b.seed_dev = (const long long *)seed_dev;
        b.gpart = (double *)(workspace + wl.gpart);
        b.gnblk = nrb;
        b.DZ = workspace + wl.dz;
        b.dz_dt = dtype;
        b.dbpart = (double *)(workspace + wl.dbpart[i]);
        k_c2d_gsum<<<dim3((unsigned)nrb, chunks), dim3(TB), 0, stream>>>(b, pp);
        WFS_LAUNCH_CHECK();
        k_c2d_dz<<<dim3((unsigned)nrb, chunks), dim3(TB), 0, stream>>>(b, pp);
        WFS_LAUNCH_CHECK();
        const void *a_prev = i == 0 ? X : (const void *)(saved + sl.act[i - 1]);
        if (i > 0 || dX) {
            GemmArgs g = {};
            g.ly = ly;
            g.layer = i;
            g.A = workspace + wl.dz;
            g.Bm = wt + wl.wt_layer[i] * es;
            g.C = i > 0 ? (void *)(workspace + wl.da[cur ^ 1]) : dX;
            g.out_row = i == 0;
            g.M = (int)(B * ly.hin * ly.win);
            g.N = ly.cin;
            g.K = ly.cout * ly.fs * ly.fs;
            launch_gemm_dt<1>(dtype, g, pp, 1, stream);
            WFS_LAUNCH_CHECK();
        }
        GemmArgs g = {};
        g.ly = ly;
        g.layer = i;
        g.A = workspace + wl.dz;
        g.Bm = a_prev;
        g.C = workspace + wl.part[i];
        g.M = ly.cout;
        g.N = ly.cin * ly.fs * ly.fs;
        g.K = M;
        launch_gemm_dt<2>(dtype, g, pp, wl.nslice[i], stream);
        WFS_LAUNCH_CHECK();
        tab.d[i].cin = ly.cin;
        tab.d[i].cout = ly.cout;
        tab.d[i].taps = ly.fs * ly.fs;
        tab.d[i].nslice = wl.nslice[i];
        tab.d[i].nrb = nrb;
        tab.d[i].p_off = (long long)(wl.part[i] - wl.part[0]);
        tab.d[i].db_off = (long long)(wl.dbpart[i] - wl.dbpart[0]) / 2;
        maxc = ly.cout > maxc ? ly.cout : maxc;
        cur ^= 1;
    }
    k_c2d_dw_reduce<<<dim3((unsigned)layers, (unsigned)maxc), dim3(TB), 0, stream>>>(
        pp, tab, workspace + wl.part[0], (const double *)(workspace + wl.dbpart[0]));
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}

extern "C" int wfs_densify_rows(const void *rows, const int32_t *coords, int64_t n_cap, int32_t C, int64_t B, int32_t H,
                                int32_t W, const int64_t *n_valid_dev, void *out, int32_t dtype, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    WFS_REQUIRE(C >= 1 && C <= MAXC, WFS_EINVAL, "rows of %d channels: 1 .. %d supported", C, MAXC);
    WFS_REQUIRE(H >= 1 && H <= MAXHW && W >= 1 && W <= MAXHW, WFS_EINVAL, "map %d x %d: 1 .. %d supported", H, W, MAXHW);
    WFS_REQUIRE(B >= 0 && B <= WFS_CONV2D_MAX_BATCH, WFS_EINVAL, "%lld events: 0 .. %d supported", (long long)B,
                WFS_CONV2D_MAX_BATCH);
    WFS_REQUIRE(n_cap >= 0 && n_cap < (1ll << 31), WFS_EINVAL, "%lld rows", (long long)n_cap);
    WFS_REQUIRE(wfs_dtype_ok(dtype), WFS_EINVAL, "bad dtype %d", dtype);
    if (B == 0) return WFS_OK;
    WFS_REQUIRE(out && (n_cap == 0 || (rows && coords)), WFS_EINVAL, "NULL device pointer");
    const dim3 grid((unsigned)B, (unsigned)H);
    const long long *n_dev = (const long long *)n_valid_dev;
    return wfs_with_dtype(dtype, [&](auto t) -> int {
        using T = decltype(t);
        k_densify<T><<<grid, dim3(TB), 0, stream>>>((const T *)rows, coords, n_cap, C, H, W, n_dev, (T *)out);
        WFS_LAUNCH_CHECK();
        return WFS_OK;
    });
}
