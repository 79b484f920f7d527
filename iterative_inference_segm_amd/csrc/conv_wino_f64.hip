// float64 Winograd F(2x2, 3x3) for the strict-parity path (the reference's CPU numerics: Theano floatX
// = float64): the wide 3x3 layers of the float64 mode as
//     input transform  V[xi][c][t] = (B^T d B)[xi]          (HBM-bound, one thread per tile x channel)
//     16 batched GEMMs M[xi][co][t] = sum_c U[xi][c][co] V[xi][c][t]
//                      on v_mfma_f64_16x16x4_f64, both operands streamed global -> LDS by LDS-DMA
//                      into a 2-deep ring (one barrier per 16-channel k-tile)
//     output transform Y = A^T M A + bias (+ skip-add with crop) (+ ReLU), window / placement
// 2.25x fewer fp64 MFMAs than the direct kernel of conv_f64.hip -- the direct form runs the matrix
// pipe 46 % busy (rocprofv3, profiles/r03_pmc.md) at half the fp32 rate, and carries the only
// end-to-end 1e-4 number of the repository (bench.py `strict_f64`).
// Numerics: float64 throughout, error ~1e-15 relative (Winograd's +-1/2 coefficients are exact); the
// exact ties DePool2D's equality masks depend on survive: a patch that is constant along a row or a
// column direction transforms to exact zeros in every other component, so equal outputs stay
// bit-equal (constant pad-100 borders, ReLU zeros).  Tiles are anchored at absolute output
// coordinates of a fixed parity (descriptor tile_y0 / tile_x0), so a windowed launch reproduces the
// full-map launch bit for bit (the loop-invariant / decoder-window eliminations rely on it).
// Same Lasagne Conv2DLayer(3x3, stride 1) call sites as conv_wino.hip (models/fcn8.py:41-71,
// models/fcn_down.py:102-104, models/fcn_up.py:83-86); with IISEG_CONV_UNPOOL the DePool2D mask
// (layers/mylayers.py:88-115) is applied while the input transform loads its patches.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "iiseg.h"
#include "common.h"
#include "conv_common.h"
#include "wino_common.h"

using namespace iiseg;

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

struct Wino64Params {
    const double* x1;
    const double* x2;
    const double* pre;      // UNPOOL: x1 = up (B, C1, h2, w2), pre (B, C1, H, W), pooled (B, C1, h2, w2)
    const double* pooled;
    int h2, w2;
    const double* U;
    const double* bias;
    const double* add;
    double* V;
    double* M;
    double* out;
    int B, C1, C2, H, W;
    int Cout, pad;
    int oy0, ox0, OH, OW;
    int ty0, tx0, nty, ntx;
    int T, Tpad;
    int Kc, Mpad;
    int AH, AW, ay0, ax0;
    int relu;
    int out_ctot, out_c0, out_H, out_W, out_y0, out_x0;
    int n_ttiles, n_mtiles;
};

// U[xi][c][co] = (G g G^T)[xi], g = w[co][c] (cross-correlation, P1)
__global__ void wino64_weight_kernel(const double* __restrict__ w, int64_t so, int64_t sc,
                                     double* __restrict__ U, int Cin, int Cout, int Kc, int Mpad) {
    const int64_t n = (int64_t)Kc * Mpad;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i / Mpad), co = (int)(i % Mpad);
        double g[3][3], u[16];
        const bool real = c < Cin && co < Cout;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) g[a][b] = real ? w[co * so + c * sc + a * 3 + b] : 0.0;
        wino_GgGt(g, u);
#pragma unroll
        for (int x = 0; x < 16; ++x) U[(int64_t)x * n + i] = u[x];
    }
}

// one thread = one tile x 2 channels; lanes run along tiles (coalesced V stores).  UNPOOL: the logical
// input is DePool2D(up = x1, pre, pooled) (layers/mylayers.py:88-115), formed while the patch is
// loaded: element (iy, ix) = pre[iy][ix] == pooled[iy/2][ix/2] ? up[iy/2][ix/2] : 0 inside the
// 2 h2 x 2 w2 region, 0 outside -- the materialised unpooled map (pool_unpool.hip) is not needed.
constexpr int ICH64 = 2;
template <bool UNPOOL>
__global__ __launch_bounds__(256) void wino64_input_kernel(const Wino64Params p) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= p.T) return;
    const WinoTile tile(p, t);
    const int b = tile.b, iy0 = tile.y - p.pad, ix0 = tile.x - p.pad;
    int rowoff[4];
    bool rok[4], cok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        rok[i] = (unsigned)(iy0 + i) < (unsigned)p.H;
        cok[i] = (unsigned)(ix0 + i) < (unsigned)p.W;
        rowoff[i] = (iy0 + i) * p.W + ix0;
    }
    const size_t HW = (size_t)p.H * p.W;
    const size_t xis = (size_t)p.Kc * p.Tpad;
    const int c0 = blockIdx.y * ICH64;
    double pv[ICH64][4][4];
    // all loads first (indices of elements outside the image clamped, masked afterwards)
#pragma unroll
    for (int cc = 0; cc < ICH64; ++cc) {
        const int c = min(c0 + cc, p.Kc - 1);
        if constexpr (UNPOOL) {
            // the 4 x 4 patch touches at most 3 x 3 pooling cells: their pooled / up values loaded
            // once, each element picks its cell by the parity of the patch origin
            const size_t hw2 = (size_t)p.h2 * p.w2;
            const double* prep = p.pre + ((size_t)b * p.C1 + c) * HW;
            const double* poolp = p.pooled + ((size_t)b * p.C1 + c) * hw2;
            const double* upp = p.x1 + ((size_t)b * p.C1 + c) * hw2;
            const int qy0 = iy0 >> 1, qx0 = ix0 >> 1;      // arithmetic shift: floor for iy0 = -pad
            const bool py = iy0 & 1, px = ix0 & 1;
            double pq[3][3], uq[3][3];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const bool ok = (unsigned)(qy0 + i) < (unsigned)p.h2 && (unsigned)(qx0 + j) < (unsigned)p.w2;
                    const int q = ok ? (qy0 + i) * p.w2 + qx0 + j : 0;
                    pq[i][j] = poolp[q];
                    uq[i][j] = ok ? upp[q] : 0.0;
                    if (!ok) pq[i][j] = __builtin_nan("");  // never equal: outside the pooled map -> 0
                }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool ok = rok[i] && cok[j];
                    const double pr = prep[ok ? rowoff[i] + j : 0];
                    const double pa = px ? pq[i >> 1][(j + 1) >> 1] : pq[i >> 1][j >> 1];
                    const double pb = px ? pq[(i + 1) >> 1][(j + 1) >> 1] : pq[(i + 1) >> 1][j >> 1];
                    const double ua = px ? uq[i >> 1][(j + 1) >> 1] : uq[i >> 1][j >> 1];
                    const double ub = px ? uq[(i + 1) >> 1][(j + 1) >> 1] : uq[(i + 1) >> 1][j >> 1];
                    pv[cc][i][j] = (ok && pr == (py ? pb : pa)) ? (py ? ub : ua) : 0.0;
                }
        } else {
            const double* src = c < p.C1 ? p.x1 + ((size_t)b * p.C1 + c) * HW
                                         : p.x2 + ((size_t)b * p.C2 + (c - p.C1)) * HW;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) pv[cc][i][j] = src[(rok[i] && cok[j]) ? rowoff[i] + j : 0];
        }
    }
#pragma unroll
    for (int cc = 0; cc < ICH64; ++cc) {
        const int c = c0 + cc;
        if (c >= p.Kc) break;
        double d[4][4], e[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) d[i][j] = (UNPOOL || (rok[i] && cok[j])) ? pv[cc][i][j] : 0.0;
        wino_Btd(d, e);
        double* v = p.V + (size_t)c * p.Tpad + t;
#pragma unroll
        for (int i = 0; i < 4; ++i) {  // (B^T d) B
            double r[4];
            wino_eB(e[i], r);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[(size_t)(i * 4 + j) * xis] = r[j];
        }
    }
}

// M[xi] = U[xi]^T V[xi]: 64 output channels x 128 tiles per workgroup, 4 waves of 64 x 32 (4 x 2 MFMA
// tiles of 16 x 16), k-tile 16 channels = 4 k-steps.  A rows [c][co] and B rows [c][t] are contiguous
// in HBM: both move by 16-byte LDS-DMA (2 + 4 pieces per thread and k-tile) into a 2-deep LDS ring.
constexpr int GBM = 64, GBN = 128, GBK = 16;
__global__ __launch_bounds__(256, 2) void wino64_gemm_kernel(const Wino64Params p) {
    __shared__ __attribute__((aligned(16))) double smem[2 * GBK * (GBM + GBN)];
    double (*As)[GBK][GBM] = reinterpret_cast<double (*)[GBK][GBM]>(smem);
    double (*Bs)[GBK][GBN] = reinterpret_cast<double (*)[GBK][GBN]>(smem + 2 * GBK * GBM);
    const int per_xi = p.n_ttiles * p.n_mtiles;
    const int xi = blockIdx.x / per_xi;
    const int rr = blockIdx.x - xi * per_xi;
    const int mt = rr % p.n_mtiles, tt = rr / p.n_mtiles;
    const int m0 = mt * GBM, t0 = tt * GBN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    const double* Ax = p.U + (size_t)xi * p.Kc * p.Mpad;
    const double* Bx = p.V + (size_t)xi * p.Kc * p.Tpad;
    const i32x4s s_a = mk_srsrc(Ax, (unsigned)(p.Kc * p.Mpad) * 8u);
    const i32x4s s_b = mk_srsrc(Bx, (unsigned)(p.Kc * p.Tpad) * 8u);
    // piece f = j * 256 + tid of a k-tile: A: row f / 32, 16-byte column f % 32; B: row f / 64, column f % 64
    unsigned aoff[2], boff[4];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int f = j * 256 + tid;
        aoff[j] = (unsigned)((f / 32) * p.Mpad + m0) * 8u + (unsigned)(f % 32) * 16u;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int f = j * 256 + tid;
        boff[j] = (unsigned)((f / 64) * p.Tpad + t0) * 8u + (unsigned)(f % 64) * 16u;
    }
    const unsigned lds_a = __builtin_amdgcn_readfirstlane(lds_addr(&As[0][0][0]) + (unsigned)wave * 1024u);
    const unsigned lds_b = __builtin_amdgcn_readfirstlane(lds_addr(&Bs[0][0][0]) + (unsigned)wave * 1024u);
#define W64_STAGE(KT, BUF)                                                                          \
    {                                                                                               \
        const unsigned soa = __builtin_amdgcn_readfirstlane((unsigned)((KT) * GBK * p.Mpad) * 8u);  \
        const unsigned sob = __builtin_amdgcn_readfirstlane((unsigned)((KT) * GBK * p.Tpad) * 8u);  \
        _Pragma("unroll") for (int j = 0; j < 2; ++j)                                               \
            dma16(s_a, lds_a + (unsigned)((BUF) * GBK * GBM * 8 + j * 4096), aoff[j], soa);         \
        _Pragma("unroll") for (int j = 0; j < 4; ++j)                                               \
            dma16(s_b, lds_b + (unsigned)((BUF) * GBK * GBN * 8 + j * 4096), boff[j], sob);         \
    }
    f64x4 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.0;
    const int nkt = p.Kc / GBK;
    W64_STAGE(0, 0)
    for (int kt = 0; kt < nkt; ++kt) {
        const int buf = kt & 1;
        // k-tile kt has landed (own pieces retired, barrier publishes everyone's) and every wave is
        // done reading the other ring slot, which the next stage overwrites from here on
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (kt + 1 < nkt) W64_STAGE(kt + 1, buf ^ 1)
#pragma unroll
        for (int ks = 0; ks < GBK / 4; ++ks) {
            const int kk = ks * 4 + lq;
            double a[4], b[2];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = As[buf][kk][i * 16 + l15];
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = Bs[buf][kk][wave * 32 + j * 16 + l15];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }
#undef W64_STAGE
    // C/D layout of the f64 16x16x4 MFMA: column = lane & 15, row = (lane >> 4) + 4 r
    double* Mx = p.M + (size_t)xi * p.Mpad * p.Tpad;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                Mx[(size_t)(m0 + i * 16 + lq + 4 * r) * p.Tpad + t0 + wave * 32 + j * 16 + l15] = acc[i][j][r];
}

constexpr int OCH64 = 2;
__global__ __launch_bounds__(256) void wino64_output_kernel(const Wino64Params p) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= p.T) return;
    const WinoTile tile(p, t);
    const int b = tile.b, wy = tile.y - p.oy0, wx = tile.x - p.ox0;  // window coords
    const bool okr[2] = {(unsigned)wy < (unsigned)p.OH, (unsigned)(wy + 1) < (unsigned)p.OH};
    const bool okc[2] = {(unsigned)wx < (unsigned)p.OW, (unsigned)(wx + 1) < (unsigned)p.OW};
    const size_t xis = (size_t)p.Mpad * p.Tpad;
    const size_t OPL = (size_t)p.out_H * p.out_W, APL = (size_t)p.AH * p.AW;
    const int co0 = blockIdx.y * OCH64;
    double mv[OCH64][16], av[OCH64][4];
#pragma unroll
    for (int cc = 0; cc < OCH64; ++cc) {
        const int co = min(co0 + cc, p.Cout - 1);
        const double* m = p.M + (size_t)co * p.Tpad + t;
#pragma unroll
        for (int x = 0; x < 16; ++x) mv[cc][x] = m[(size_t)x * xis];
        if (p.add) {
            const double* ad = p.add + ((size_t)b * p.Cout + co) * APL;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const bool ok = okr[i] && okc[j];
                    const ptrdiff_t idx = (ptrdiff_t)(p.ay0 + wy + i) * p.AW + p.ax0 + wx + j;
                    const double a = ad[ok ? idx : 0];
                    av[cc][i * 2 + j] = ok ? a : 0.0;
                }
        }
    }
#pragma unroll
    for (int cc = 0; cc < OCH64; ++cc) {
        const int co = co0 + cc;
        if (co >= p.Cout) break;
        double s2[2][4];
        wino_Atm(mv[cc], s2);
        const double bias = p.bias ? p.bias[co] : 0.0;
        double* o = p.out + ((size_t)b * p.out_ctot + p.out_c0 + co) * OPL +
                    (ptrdiff_t)(p.out_y0 + wy) * p.out_W + p.out_x0 + wx;
#pragma unroll
        for (int i = 0; i < 2; ++i) {  // (A^T m) A
            double y[2];
            wino_sA(s2[i], y);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (okr[i] && okc[j]) {
                    double v = y[j] + bias;
                    if (p.add) v += av[cc][i * 2 + j];
                    if (p.relu) v = fmax(v, 0.0);
                    o[(ptrdiff_t)i * p.out_W + j] = v;
                }
            }
        }
    }
}

// ---- the transforms again, for tensors within 32-bit byte offsets (every launch of the strict_f64 leg but one) ----
// wino64_input_kernel / wino64_output_kernel above spend their cycles ISSUING, not waiting (PMC: 78-92 % / 58 % of a
// wave's cycles issue-stalled, profiles/r04_pmc_f64.md): per 4 x 4 patch of a channel 48 v_cndmask + 36 64-bit
// address adds around the 32 v_add_f64 of the transform.  Here every per-thread address is a 32-bit byte offset
// computed ONCE (out-of-image elements get the out-of-range offset: the load returns 0.0, no select), the channel
// is a scalar offset of the buffer instruction, and V / M are addressed as wave-uniform base + thread index.
// Same arithmetic in the same order: bit-identical to the kernels above.
constexpr unsigned OOB64 = 0x80000000u;
__device__ __forceinline__ double bld64(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    typedef int i32x2_ __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(double, (i32x2_)__builtin_amdgcn_raw_buffer_load_b64(r, (int)voff, (int)soff, 0));
}
__device__ __forceinline__ void bst64(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff, double v) {
    typedef int i32x2_ __attribute__((ext_vector_type(2)));
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(i32x2_, v), r, (int)voff, (int)soff, 0);
}

constexpr int ICG64 = 4;      // channels per thread (loop, two per trip)
template <bool UNPOOL>
__global__ __launch_bounds__(256) void wino64_input2_kernel(const Wino64Params p) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const bool tok = t < p.T;
    const int tt = tok ? t : 0;
    const int ntt = p.nty * p.ntx;
    const int b = tt / ntt;
    const int r = tt - b * ntt;
    const int tyl = r / p.ntx, txl = r - tyl * p.ntx;
    const int iy0 = p.ty0 + 2 * tyl - p.pad, ix0 = p.tx0 + 2 * txl - p.pad;
    const int HW = p.H * p.W;
    // byte offsets of the 4 x 4 patch inside image b's first channel plane, per source (OOB64: zero padding)
    unsigned pix[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool ok = tok && (unsigned)(iy0 + i) < (unsigned)p.H && (unsigned)(ix0 + j) < (unsigned)p.W;
            pix[i][j] = ok ? 8u * (unsigned)((iy0 + i) * p.W + ix0 + j) : OOB64;
        }
    const unsigned bb1 = 8u * (unsigned)(b * p.C1 * HW), bb2 = 8u * (unsigned)(b * p.C2 * HW);
    unsigned pa1[4][4], pa2[UNPOOL ? 1 : 4][UNPOOL ? 1 : 4];      // ... with the image's offset in each source
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            pa1[i][j] = pix[i][j] != OOB64 ? pix[i][j] + bb1 : OOB64;
            if constexpr (!UNPOOL) pa2[i][j] = pix[i][j] != OOB64 ? pix[i][j] + bb2 : OOB64;
        }
    // V as one buffer: slice (xi, c) is a scalar offset, the tile a fixed per-thread offset
    const __amdgpu_buffer_rsrc_t rV = __builtin_amdgcn_make_buffer_rsrc(
        (void*)p.V, 0, (int)(8u * (unsigned)(16 * p.Kc * p.Tpad)), RSRC_W3);
    const unsigned tv = tok ? 8u * (unsigned)t : OOB64;
    const __amdgpu_buffer_rsrc_t r1 = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(UNPOOL ? p.pre : p.x1), 0, (int)(8u * (unsigned)(p.B * p.C1 * HW)), RSRC_W3);
    const __amdgpu_buffer_rsrc_t r2 = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(p.C2 > 0 ? p.x2 : p.x1), 0, (int)(8u * (unsigned)(p.B * (p.C2 > 0 ? p.C2 : p.C1) * HW)), RSRC_W3);
    // UNPOOL: the 3 x 3 pooling cells the patch touches (pooled / up), byte offsets inside image b's first plane
    const int hw2 = p.h2 * p.w2;
    unsigned qix[UNPOOL ? 3 : 1][UNPOOL ? 3 : 1];
    const int qy0 = iy0 >> 1, qx0 = ix0 >> 1;           // arithmetic shift: floor for iy0 = -pad
    const bool py = iy0 & 1, px = ix0 & 1;
    if constexpr (UNPOOL) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const bool ok = tok && (unsigned)(qy0 + i) < (unsigned)p.h2 && (unsigned)(qx0 + j) < (unsigned)p.w2;
                qix[i][j] = ok ? 8u * (unsigned)((qy0 + i) * p.w2 + qx0 + j) + 8u * (unsigned)(b * p.C1 * hw2) : OOB64;
            }
    }
    const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(UNPOOL ? p.pooled : p.x1), 0, (int)(8u * (unsigned)(p.B * p.C1 * (UNPOOL ? hw2 : HW))), RSRC_W3);
    const __amdgpu_buffer_rsrc_t ru = __builtin_amdgcn_make_buffer_rsrc(
        (void*)p.x1, 0, (int)(8u * (unsigned)(p.B * p.C1 * (UNPOOL ? hw2 : HW))), RSRC_W3);
    const size_t xis = (size_t)p.Kc * p.Tpad;
    const int c0 = blockIdx.y * ICG64;
    for (int cc = 0; cc < ICG64; cc += 2) {
        if (c0 + cc >= p.Kc) break;
        double d[2][4][4];
        // all loads of the two channels first
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int c = min(c0 + cc + h, p.Kc - 1);
            if constexpr (UNPOOL) {
                double pq[3][3], uq[3][3];
                const unsigned soq = 8u * (unsigned)(c * hw2);
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const bool ok = qix[i][j] != OOB64;
                        pq[i][j] = bld64(rq, qix[i][j], soq);
                        uq[i][j] = bld64(ru, qix[i][j], soq);
                        if (!ok) pq[i][j] = __builtin_nan("");     // never equal: outside the pooled map -> 0
                    }
                const unsigned so = 8u * (unsigned)(c * HW);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bool ok = pix[i][j] != OOB64;
                        const double pr = bld64(r1, pa1[i][j], so);
                        const double pa = px ? pq[i >> 1][(j + 1) >> 1] : pq[i >> 1][j >> 1];
                        const double pb = px ? pq[(i + 1) >> 1][(j + 1) >> 1] : pq[(i + 1) >> 1][j >> 1];
                        const double ua = px ? uq[i >> 1][(j + 1) >> 1] : uq[i >> 1][j >> 1];
                        const double ub = px ? uq[(i + 1) >> 1][(j + 1) >> 1] : uq[(i + 1) >> 1][j >> 1];
                        d[h][i][j] = (ok && pr == (py ? pb : pa)) ? (py ? ub : ua) : 0.0;
                    }
            } else {
                const bool s1 = c < p.C1;
                const unsigned so = 8u * (unsigned)((s1 ? c : c - p.C1) * HW);
                if (s1) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) d[h][i][j] = bld64(r1, pa1[i][j], so);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) d[h][i][j] = bld64(r2, pa2[i][j], so);
                }
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int c = c0 + cc + h;
            if (c >= p.Kc) break;
            // (wino_Btd / wino_eB of wino_common.h written out, the only copy left: through the helpers hipcc
            // forms this kernel's 16 scalar store offsets with s_mul instead of adds, 8 % more instructions
            // in a kernel that is bound by issue; the child-process test of test_gpu_f64.py holds it to
            // wino64_input_kernel, which uses them, bit for bit)
            double e[4][4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {  // B^T d
                e[0][j] = d[h][0][j] - d[h][2][j];
                e[1][j] = d[h][1][j] + d[h][2][j];
                e[2][j] = d[h][2][j] - d[h][1][j];
                e[3][j] = d[h][1][j] - d[h][3][j];
            }
            const unsigned sv = 8u * (unsigned)(c * p.Tpad), sx = 8u * (unsigned)(p.Kc * p.Tpad);
#pragma unroll
            for (int i = 0; i < 4; ++i) {  // (B^T d) B
                bst64(rV, tv, sv + (unsigned)(i * 4 + 0) * sx, e[i][0] - e[i][2]);
                bst64(rV, tv, sv + (unsigned)(i * 4 + 1) * sx, e[i][1] + e[i][2]);
                bst64(rV, tv, sv + (unsigned)(i * 4 + 2) * sx, e[i][2] - e[i][1]);
                bst64(rV, tv, sv + (unsigned)(i * 4 + 3) * sx, e[i][1] - e[i][3]);
            }
        }
    }
}

constexpr int OCG64 = 2;      // output channels per thread (loop)
__global__ __launch_bounds__(256) void wino64_output2_kernel(const Wino64Params p) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= p.T) return;
    const WinoTile tile(p, t);
    const int b = tile.b, wy = tile.y - p.oy0, wx = tile.x - p.ox0;  // window coords
    const int OPL = p.out_H * p.out_W, APL = p.AH * p.AW;
    unsigned ooff[2][2], aoff[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const bool ok = (unsigned)(wy + i) < (unsigned)p.OH && (unsigned)(wx + j) < (unsigned)p.OW;
            ooff[i][j] = ok ? 8u * (unsigned)((b * p.out_ctot + p.out_c0) * OPL + (p.out_y0 + wy + i) * p.out_W +
                                              p.out_x0 + wx + j)
                            : OOB64;
            aoff[i][j] = (ok && p.add) ? 8u * (unsigned)(b * p.Cout * APL + (p.ay0 + wy + i) * p.AW + p.ax0 + wx + j)
                                       : OOB64;
        }
    const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(
        (void*)p.out, 0, (int)(8u * (unsigned)(p.B * p.out_ctot * OPL)), RSRC_W3);
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(p.add ? p.add : p.out), 0, p.add ? (int)(8u * (unsigned)(p.B * p.Cout * APL)) : 0, RSRC_W3);
    const __amdgpu_buffer_rsrc_t rM = __builtin_amdgcn_make_buffer_rsrc(
        (void*)p.M, 0, (int)(8u * (unsigned)(16 * p.Mpad * p.Tpad)), RSRC_W3);
    const unsigned tv = 8u * (unsigned)t, sx = 8u * (unsigned)(p.Mpad * p.Tpad);
    const int co0 = blockIdx.y * OCG64;
    for (int cc = 0; cc < OCG64; ++cc) {
        const int co = co0 + cc;
        if (co >= p.Cout) break;
        const unsigned sm = 8u * (unsigned)(co * p.Tpad);
        double mv[16], av[4];
#pragma unroll
        for (int x = 0; x < 16; ++x) mv[x] = bld64(rM, tv, sm + (unsigned)x * sx);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) av[i * 2 + j] = bld64(ra, aoff[i][j], 8u * (unsigned)(co * APL));
        double s2[2][4];
        wino_Atm(mv, s2);
        const double bias = p.bias ? p.bias[co] : 0.0;
#pragma unroll
        for (int i = 0; i < 2; ++i) {  // (A^T m) A
            double y[2];
            wino_sA(s2[i], y);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                double v = y[j] + bias;
                if (p.add) v += av[i * 2 + j];
                if (p.relu) v = fmax(v, 0.0);
                bst64(ro, ooff[i][j], 8u * (unsigned)(co * OPL), v);
            }
        }
    }
}

struct Wino64Geom {
    int Kc, Mpad, ty0, tx0, nty, ntx, T, Tpad;
};

int wino64_geom(const iiseg_conv_desc* d, Wino64Geom& g) {
    WinoTiles w;
    const int st = wino_tiles(d, w, GBK);
    if (st) return st;
    g.Kc = d->C1 + d->C2;
    g.Mpad = round_up(d->Cout, GBM);
    g.ty0 = w.ty0; g.tx0 = w.tx0; g.nty = w.nty; g.ntx = w.ntx;
    const int64_t T = w.T;
    const int64_t Tpad = (T + GBN - 1) / GBN * GBN;
    // one xi-slice of U / V is addressed with 32-bit byte offsets
    if (Tpad * g.Kc * 8 >= (int64_t)1 << 31 || (int64_t)g.Kc * g.Mpad * 8 >= (int64_t)1 << 31)
        return IISEG_ERR_UNSUPPORTED;
    g.T = (int)T;
    g.Tpad = (int)Tpad;
    return IISEG_OK;
}

// ---- deep 1x1 layers (fc6 after iiseg_im2col_f64, fc7, score_fr: models/fcn8.py:75-85) as split-K GEMMs ----
// on wino64_gemm_kernel: the static-tap kernel walks K = 25088 with a gather per element and a barrier pair
// per 16 k (28 TFLOP/s); here x (B, K, OH*OW) is laid out once as V[k][t] and both operands stream by LDS-DMA.
// The packed weights Wp[Kpad][Mpad] of iiseg_conv_pack_f64 ARE the A operand; K slices play the xi role.
struct Gemm64Geom {
    int K, Kpad, Mpad, T, Tpad, S, Kc, OHW;
};

__global__ __launch_bounds__(256) void gemm64_input_kernel(const double* __restrict__ x, double* __restrict__ V,
                                                           int K, int Kpad, int OHW, int T, int Tpad) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int b = t / OHW, px = t - b * OHW;
    const double* xb = x + (size_t)b * K * OHW + px;
    for (int k = blockIdx.y; k < Kpad; k += gridDim.y)
        V[(size_t)k * Tpad + t] = k < K ? xb[(size_t)k * OHW] : 0.0;
}

__global__ __launch_bounds__(256) void gemm64_output_kernel(const double* __restrict__ M,
                                                            const double* __restrict__ bias,
                                                            double* __restrict__ out, int Cout, int OHW, int T,
                                                            int Tpad, int Mpad, int S, int relu) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int b = t / OHW, px = t - b * OHW;
    const size_t ss = (size_t)Mpad * Tpad;
    for (int co = blockIdx.y; co < Cout; co += gridDim.y) {
        const double* m = M + (size_t)co * Tpad + t;
        double v = m[0];
        for (int s = 1; s < S; ++s) v += m[(size_t)s * ss];   // fixed order: deterministic
        if (bias) v += bias[co];
        if (relu) v = fmax(v, 0.0);
        out[((size_t)b * Cout + co) * OHW + px] = v;
    }
}

int gemm64_geom(const iiseg_conv_desc* d, Gemm64Geom& g) {
    if (!d) return IISEG_ERR_NULL;
    if (d->KH != 1 || d->KW != 1 || d->C2 != 0 || d->dil != 1 || d->pad != 0 ||
        (d->flags & (IISEG_CONV_UNPOOL | IISEG_CONV_TRANSPOSED2)))
        return IISEG_ERR_UNSUPPORTED;
    if (d->B <= 0 || d->C1 <= 0 || d->H <= 0 || d->W <= 0 || d->Cout <= 0) return IISEG_ERR_SHAPE;
    // full, dense output only
    if (d->oy0 != 0 || d->ox0 != 0 || d->OH != d->H || d->OW != d->W || d->out_ctot != 0 || d->out_H != 0)
        return IISEG_ERR_UNSUPPORTED;
    g.K = d->C1;
    g.Kpad = d->Kpad;
    g.Mpad = d->Mpad;
    if (g.Kpad < g.K || g.Kpad % GBK || g.Mpad % GBM || g.Mpad < d->Cout) return IISEG_ERR_UNSUPPORTED;
    g.OHW = d->H * d->W;
    const int64_t T = (int64_t)d->B * g.OHW;
    const int64_t Tpad = (T + GBN - 1) / GBN * GBN;
    if (Tpad * g.Kpad * 8 >= (int64_t)1 << 31 || (int64_t)g.Kpad * g.Mpad * 8 >= (int64_t)1 << 31)
        return IISEG_ERR_UNSUPPORTED;
    g.T = (int)T;
    g.Tpad = (int)Tpad;
    // split-K: the divisor S of Kpad / 16 (<= 16) minimising GEMM rounds (512 resident 64 x 128 tiles at the
    // measured 55 TFLOP/s) + the traffic of the S partial products.  S fixes the association of the K sum,
    // so it must NOT depend on the batch: it is chosen for a nominal 3200 pixels (64 images x 7 x 7).
    const int tiles = 25 * (g.Mpad / GBM), units = g.Kpad / GBK;
    const double tile_s = 2.0 * g.Kpad * GBM * GBN / (55e12 / 512);
    const double red_s = 16.0 * g.Mpad * 3200 / 5e12;
    double best = 1e30;
    g.S = 1;
    for (int S = 1; S <= 16; ++S) {
        if (units % S || units / S < 8) continue;
        const double cost = (double)((S * tiles + 511) / 512) / S * tile_s + S * red_s;
        if (cost < best) { best = cost; g.S = S; }
    }
    g.Kc = g.Kpad / g.S;
    return IISEG_OK;
}

}  // namespace

extern "C" int iiseg_conv_gemm_f64_supported(const iiseg_conv_desc* d) {
    Gemm64Geom g;
    return gemm64_geom(d, g) == IISEG_OK ? 1 : 0;
}

extern "C" int64_t iiseg_conv_gemm_f64_workspace_elems(const iiseg_conv_desc* d) {
    Gemm64Geom g;
    if (gemm64_geom(d, g) != IISEG_OK) return 0;
    return (int64_t)g.Tpad * ((int64_t)g.Kpad + (int64_t)g.S * g.Mpad);
}

extern "C" int iiseg_conv_gemm_f64(void* stream, const iiseg_conv_desc* d, const double* x, const double* wp,
                                   const double* bias, double* workspace, double* out) {
    Gemm64Geom g;
    const int st = gemm64_geom(d, g);
    if (st) return st;
    if (!x || !wp || !workspace || !out) return IISEG_ERR_NULL;
    if (((uintptr_t)wp & 15) || ((uintptr_t)workspace & 15)) return IISEG_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    double* V = workspace;
    double* M = workspace + (size_t)g.Kpad * g.Tpad;
    const int tb = (g.T + 255) / 256;
    IISEG_LAUNCH(gemm64_input_kernel, dim3(tb, g.Kpad < 1024 ? g.Kpad : 1024), dim3(256), 0, s, x, V, g.K,
                 g.Kpad, g.OHW, g.T, g.Tpad);
    Wino64Params p = {};
    p.U = wp;
    p.V = V;
    p.M = M;
    p.Kc = g.Kc;
    p.Mpad = g.Mpad;
    p.Tpad = g.Tpad;
    p.T = g.T;
    p.n_ttiles = g.Tpad / GBN;
    p.n_mtiles = g.Mpad / GBM;
    IISEG_LAUNCH(wino64_gemm_kernel, dim3(g.S * p.n_ttiles * p.n_mtiles), dim3(256), 0, s, p);
    const int cy = d->Cout < 1024 ? d->Cout : 1024;
    IISEG_LAUNCH(gemm64_output_kernel, dim3(tb, cy), dim3(256), 0, s, M, bias, out, d->Cout, g.OHW, g.T, g.Tpad,
                 g.Mpad, g.S, (d->flags & IISEG_CONV_RELU) ? 1 : 0);
    return iiseg_check_launch();
}

extern "C" int iiseg_conv_wino_f64_supported(const iiseg_conv_desc* d) {
    Wino64Geom g;
    return wino64_geom(d, g) == IISEG_OK ? 1 : 0;
}

extern "C" int64_t iiseg_conv_wino_f64_weight_elems(const iiseg_conv_desc* d) {
    Wino64Geom g;
    if (wino64_geom(d, g) != IISEG_OK) return 0;
    return (int64_t)16 * g.Kc * g.Mpad;
}

extern "C" int64_t iiseg_conv_wino_f64_workspace_elems(const iiseg_conv_desc* d) {
    Wino64Geom g;
    if (wino64_geom(d, g) != IISEG_OK) return 0;
    return (int64_t)16 * g.Tpad * ((int64_t)g.Kc + g.Mpad);
}

extern "C" int iiseg_conv_wino_pack_f64(void* stream, const iiseg_conv_desc* d, const double* w,
                                        int64_t stride_o, int64_t stride_c, double* U) {
    Wino64Geom g;
    const int st = wino64_geom(d, g);
    if (st) return st;
    if (!w || !U) return IISEG_ERR_NULL;
    const int64_t n = (int64_t)g.Kc * g.Mpad;
    const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    IISEG_LAUNCH(wino64_weight_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, w, stride_o,
                       stride_c, U, d->C1 + d->C2, d->Cout, g.Kc, g.Mpad);
    return iiseg_check_launch();
}

extern "C" int iiseg_conv_wino_f64(void* stream, const iiseg_conv_desc* d, const double* x1,
                                   const double* x2, const double* pre, const double* pooled,
                                   const double* U, const double* bias, const double* add,
                                   double* workspace, double* out) {
    Wino64Geom g;
    const int st = wino64_geom(d, g);
    if (st) return st;
    if (!x1 || !U || !workspace || !out) return IISEG_ERR_NULL;
    if (d->C2 > 0 && !x2) return IISEG_ERR_NULL;
    const bool unpool = (d->flags & IISEG_CONV_UNPOOL) != 0;
    if (unpool && (!pre || !pooled)) return IISEG_ERR_NULL;
    if (((uintptr_t)U & 15) || ((uintptr_t)workspace & 15)) return IISEG_ERR_ALIGN;
    if (add && (d->ay0 < 0 || d->ax0 < 0 || d->ay0 + d->OH > d->AH || d->ax0 + d->OW > d->AW))
        return IISEG_ERR_SHAPE;
    Wino64Params p = {};
    p.x1 = x1; p.x2 = x2; p.pre = pre; p.pooled = pooled; p.h2 = d->H / 2; p.w2 = d->W / 2;
    p.U = U; p.bias = bias; p.add = add;
    p.V = workspace;
    p.M = workspace + (size_t)16 * g.Kc * g.Tpad;
    p.out = out;
    p.B = d->B; p.C1 = d->C1; p.C2 = d->C2; p.H = d->H; p.W = d->W;
    p.Cout = d->Cout; p.pad = d->pad;
    p.oy0 = d->oy0; p.ox0 = d->ox0; p.OH = d->OH; p.OW = d->OW;
    p.ty0 = g.ty0; p.tx0 = g.tx0; p.nty = g.nty; p.ntx = g.ntx;
    p.T = g.T; p.Tpad = g.Tpad; p.Kc = g.Kc; p.Mpad = g.Mpad;
    p.AH = d->AH; p.AW = d->AW; p.ay0 = d->ay0; p.ax0 = d->ax0;
    p.relu = (d->flags & IISEG_CONV_RELU) ? 1 : 0;
    if (wino_out_place(d, p)) return IISEG_ERR_SHAPE;
    p.n_ttiles = g.Tpad / GBN;
    p.n_mtiles = g.Mpad / GBM;
    hipStream_t s = (hipStream_t)stream;
    const int tb = (g.T + 255) / 256;
    // the transforms with 32-bit per-thread offsets where every tensor they address stays below 2 GiB
    static const int t2 = getenv("IISEG_W64_FAST_TRANSFORMS") ? atoi(getenv("IISEG_W64_FAST_TRANSFORMS")) : 1;
    const int64_t lim = (int64_t)1 << 31;
    const int64_t HW8 = (int64_t)d->H * d->W * 8, hw28 = (int64_t)(d->H / 2) * (d->W / 2) * 8;
    const int64_t lim32 = ((int64_t)1 << 32) - 16;            // V / M: unsigned offsets, scalar + per-thread part
    const bool in_fast = t2 && (int64_t)d->B * d->C1 * HW8 < lim && (int64_t)d->B * d->C2 * HW8 < lim &&
                         (!unpool || (int64_t)d->B * d->C1 * hw28 < lim) &&
                         (int64_t)16 * g.Kc * g.Tpad * 8 < lim32;
    const bool out_fast = t2 && (int64_t)d->B * p.out_ctot * p.out_H * p.out_W * 8 < lim &&
                          (!add || (int64_t)d->B * d->Cout * d->AH * d->AW * 8 < lim) &&
                          (int64_t)16 * g.Mpad * g.Tpad * 8 < lim32;
    // (the DePool2D form of the new input transform measured slower than the old one -- 0.204 against 0.17-0.19 ms
    // per launch: 34 loads and the window selects per channel either way -- and is only used on request)
    static const int t2u = getenv("IISEG_W64_FAST_UNPOOL") ? atoi(getenv("IISEG_W64_FAST_UNPOOL")) : 0;
    if (in_fast && (!unpool || t2u)) {
        if (unpool)
            IISEG_LAUNCH(wino64_input2_kernel<true>, dim3(tb, (g.Kc + ICG64 - 1) / ICG64), dim3(256), 0, s, p);
        else
            IISEG_LAUNCH(wino64_input2_kernel<false>, dim3(tb, (g.Kc + ICG64 - 1) / ICG64), dim3(256), 0, s, p);
    } else if (unpool)
        IISEG_LAUNCH(wino64_input_kernel<true>, dim3(tb, (g.Kc + ICH64 - 1) / ICH64), dim3(256), 0, s, p);
    else
        IISEG_LAUNCH(wino64_input_kernel<false>, dim3(tb, (g.Kc + ICH64 - 1) / ICH64), dim3(256), 0, s, p);
    IISEG_LAUNCH(wino64_gemm_kernel, dim3(16 * p.n_ttiles * p.n_mtiles), dim3(256), 0, s, p);
    if (out_fast)
        IISEG_LAUNCH(wino64_output2_kernel, dim3(tb, (d->Cout + OCG64 - 1) / OCG64), dim3(256), 0, s, p);
    else
        IISEG_LAUNCH(wino64_output_kernel, dim3(tb, (d->Cout + OCH64 - 1) / OCH64), dim3(256), 0, s, p);
    return iiseg_check_launch();
}
