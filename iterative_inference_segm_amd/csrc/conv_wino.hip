// Winograd F(2x2, 3x3) convolution for gfx950 (CDNA4), fp32.
//
// The fp32 matrix pipe (v_mfma_f32_32x32x2_f32, 157 TFLOP/s) is what bounds the wide 3x3 layers of
// the hot path, so the way to go faster at full fp32 precision is to issue fewer multiplies:
// Y = A^T [ (G g G^T) . (B^T d B) ] A computes a 2x2 output tile from a 4x4 input tile with 16
// instead of 36 multiplies per (cin, cout) pair (2.25x fewer MFMAs).  Three kernels:
//   1. wino_input_kernel   V[xi][c][t]  = (B^T d B)[xi]          HBM-bound, lanes along tiles
//   2. wino_gemm_kernel    M[xi][co][t] = sum_c U[xi][c][co] * V[xi][c][t]
//                          16 independent GEMMs, MFMA-bound, both operands stream global -> LDS
//                          with 16-byte LDS-DMA (no gather, no VALU address work)
//   3. wino_output_kernel  out = relu(A^T M A + bias + add), cropped to the window
// U = G g G^T is packed once per layer (wino_weight_kernel, computed in double).
//
// Tiles are anchored at ABSOLUTE output coordinates of a fixed parity (desc.tile_y0 / tile_x0, a
// per-layer constant chosen by the caller), so a pixel is produced by the same tile, the same 4x4
// patch and the same fixed-order sums whatever window of the layer is being computed: windowed /
// placed launches stay bit-identical to full-map launches (the property the decoder dead-code
// elimination and the loop-invariant encoder borders rely on).  The caller picks the parity of
// the window it launches most: a 10x10 window at an odd origin is 5x5 tiles instead of 6x6.
//
// Replaces the same Lasagne Conv2DLayer(3x3, stride 1) call sites as conv_taps.hip for layers
// with Cin % 16 == 0 (models/fcn8.py:41-71, models/fcn_down.py:102-104, models/fcn_up.py:83-86);
// fusions kept: two-source channel concat (h first), bias / skip-add / ReLU / window / placement;
// DePool2D input from pre / pooled or from mask bytes; at an even tile anchor the 2x2 max-pool and its
// mask bytes in the output transform (a tile is then one pooling window, its four values in one lane).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <atomic>
#include <type_traits>
#include "iiseg.h"
#include "common.h"
#include "conv_common.h"
#include "wino_common.h"

using namespace iiseg;

namespace {

struct WinoParams {
    const float* x1;
    const float* x2;
    const float* pre;     // unpool mode: x1 = up, pre, pooled (DePool2D operands) ...
    const float* pooled;
    const uint8_t* mask_in;   // ... or x1 = up and the mask bytes (then pre / pooled are unused)
    int h2, w2;
    const float* U;
    const float* bias;
    const float* add;
    float* V;
    float* M;
    float* out;
    int B, C1, C2, H, W;
    int Cout, pad;
    int oy0, ox0, OH, OW;    // output window in conv-output coordinates
    int ty0, tx0, nty, ntx;  // first tile's output row / column (absolute), tile counts
    int T, Tpad;             // B*nty*ntx, padded to the GEMM pixel tile
    int Kc, Mpad;            // channels (multiple of 16), output channels padded to the GEMM tile
    int AH, AW, ay0, ax0;
    int relu;
    int out_ctot, out_c0, out_H, out_W, out_y0, out_x0;
    int n_ttiles, n_mtiles;
    // fused 2x2 max-pool (even tile anchor: a tile IS a pooling window): FULL pooled tensor
    // (B, Cout, pool_H, pool_W) and its DePool2D mask bytes (may be NULL); out may then be NULL
    float* pool;
    uint8_t* mask_out;
    int pool_H, pool_W;
    int mq;                  // M is M[xi][Mpad / 4][Tpad][4] (m_quad below), else M[xi][Mpad][Tpad]
};

// max of a 2x2 window in the order of maxpool2x2 (pool_unpool.hip): same value, same sign of zero
__device__ __forceinline__ float pool4(float v00, float v01, float v10, float v11) {
    const float a = v00 > v01 ? v00 : v01;
    const float b = v10 > v11 ? v10 : v11;
    return a > b ? a : b;
}

// pooled value + mask byte (bit (y & 1) * 2 + (x & 1): pre == pooled) of one whole tile
__device__ __forceinline__ void pool_store(const WinoParams& p, int b, int co, int ay, int ax,
                                           float v00, float v01, float v10, float v11) {
    const float m = pool4(v00, v01, v10, v11);
    const size_t po = ((size_t)b * p.Cout + co) * p.pool_H * p.pool_W + (size_t)(ay >> 1) * p.pool_W + (ax >> 1);
    p.pool[po] = m;
    if (p.mask_out)
        p.mask_out[po] = (uint8_t)((v00 == m ? 1u : 0u) | (v01 == m ? 2u : 0u) |
                                   (v10 == m ? 4u : 0u) | (v11 == m ? 8u : 0u));
}

// ---- 0. weights: U[xi][c][co] = (G g G^T)[xi], g = w[co][c] (cross-correlation, P1) -----------
__global__ void wino_weight_kernel(const float* __restrict__ w, int64_t so, int64_t sc,
                                   float* __restrict__ U, int Cin, int Cout, int Kc, int Mpad) {
    const int64_t n = (int64_t)Kc * Mpad;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i / Mpad), co = (int)(i % Mpad);
        double g[3][3], t[4][3];
        const bool real = c < Cin && co < Cout;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) g[a][b] = real ? (double)w[co * so + c * sc + a * 3 + b] : 0.0;
        wino_Gg(g, t);
#pragma unroll
        for (int a = 0; a < 4; ++a) {  // (G g) G^T
            double u[4];
            wino_tGt(t[a], u);
#pragma unroll
            for (int b = 0; b < 4; ++b) U[(int64_t)(a * 4 + b) * n + i] = (float)u[b];
        }
    }
}

// ---- 1. input transform ------------------------------------------------------------------------
// One thread = one tile x ICH channels; lanes run along tiles (coalesced V stores).
// UNPOOL: the logical input is DePool2D(up = x1, pre, pooled) (layers/mylayers.py:88-115), formed
// while loading the patch: element (iy, ix) = pre == pooled[iy/2, ix/2] ? up[iy/2, ix/2] : 0 inside
// the 2h x 2w region, 0 outside.  PY / PX = parity of the patch origin (uniform over a launch), so
// the 3x3 block of pooled/up values a 4x4 patch touches is indexed at compile time.
// MB (with UNPOOL): the mask comes as bytes (p.mask_in, bit (iy & 1) * 2 + (ix & 1) = pre == pooled,
// written by the pooling conv or pool kernel): up + one byte per 2x2 instead of pre / pooled / up.
constexpr int ICH = 4;
template <bool UNPOOL, int PY, int PX, bool MB = false>
__global__ __launch_bounds__(256) void wino_input_kernel(const WinoParams p) {
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
    // unpool: pooled-plane block rows/cols q = 0..2 cover patch rows (PY + i) >> 1
    constexpr int NQY = UNPOOL ? (PY ? 3 : 2) : 1, NQX = UNPOOL ? (PX ? 3 : 2) : 1;
    const int qy0 = (iy0 - PY) >> 1, qx0 = (ix0 - PX) >> 1;   // floor(iy0 / 2) for either parity
    bool qrok[NQY], qcok[NQX];
    int qoff[NQY];
    if constexpr (UNPOOL) {
#pragma unroll
        for (int i = 0; i < NQY; ++i) {
            qrok[i] = (unsigned)(qy0 + i) < (unsigned)p.h2;
            qoff[i] = (qy0 + i) * p.w2 + qx0;
        }
#pragma unroll
        for (int j = 0; j < NQX; ++j) qcok[j] = (unsigned)(qx0 + j) < (unsigned)p.w2;
    }
    const size_t HW = (size_t)p.H * p.W, hw2 = (size_t)p.h2 * p.w2;
    const size_t xis = (size_t)p.Kc * p.Tpad;
    // Phase 1: every load of the thread's channels, unconditional (offsets of elements outside the
    // image are clamped to element 0 of the plane and masked afterwards) so that all are in
    // flight together; phase 2: transform + store.  (Loads placed after a store could not be
    // moved up: V and the inputs may alias as far as the compiler knows.)
    constexpr int NC_ = UNPOOL ? ICH / 2 : ICH;
    const int c0 = blockIdx.y * NC_;
    float pv[MB ? 1 : NC_][4][4];
    float pq[UNPOOL && !MB ? NC_ : 1][NQY][NQX], uq[UNPOOL ? NC_ : 1][NQY][NQX];
    uint32_t mq[MB ? NC_ : 1][NQY][NQX];
#pragma unroll
    for (int cc = 0; cc < NC_; ++cc) {
        const int c = min(c0 + cc, p.Kc - 1);
        if constexpr (MB) {
            const uint8_t* mp = p.mask_in + ((size_t)b * p.C1 + c) * hw2;
            const float* upp = p.x1 + ((size_t)b * p.C1 + c) * hw2;
#pragma unroll
            for (int i = 0; i < NQY; ++i)
#pragma unroll
                for (int j = 0; j < NQX; ++j) {
                    const int o = (qrok[i] && qcok[j]) ? qoff[i] + j : 0;
                    mq[cc][i][j] = mp[o];
                    uq[cc][i][j] = upp[o];
                }
        } else if constexpr (UNPOOL) {
            const float* prep = p.pre + ((size_t)b * p.C1 + c) * HW;
            const float* poolp = p.pooled + ((size_t)b * p.C1 + c) * hw2;
            const float* upp = p.x1 + ((size_t)b * p.C1 + c) * hw2;
#pragma unroll
            for (int i = 0; i < NQY; ++i)
#pragma unroll
                for (int j = 0; j < NQX; ++j) {
                    const int o = (qrok[i] && qcok[j]) ? qoff[i] + j : 0;
                    pq[cc][i][j] = poolp[o];
                    uq[cc][i][j] = upp[o];
                }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) pv[cc][i][j] = prep[(rok[i] && cok[j]) ? rowoff[i] + j : 0];
        } else {
            const float* src = c < p.C1 ? p.x1 + ((size_t)b * p.C1 + c) * HW
                                        : p.x2 + ((size_t)b * p.C2 + (c - p.C1)) * HW;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) pv[cc][i][j] = src[(rok[i] && cok[j]) ? rowoff[i] + j : 0];
        }
    }
#pragma unroll
    for (int cc = 0; cc < NC_; ++cc) {
        const int c = c0 + cc;
        if (c >= p.Kc) break;
        float d[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if constexpr (MB) {
                    const int qi = (PY + i) >> 1, qj = (PX + j) >> 1;
                    const int bit = ((PY + i) & 1) * 2 + ((PX + j) & 1);
                    const bool ok = rok[i] && cok[j] && qrok[qi] && qcok[qj];
                    d[i][j] = (ok && ((mq[cc][qi][qj] >> bit) & 1u)) ? uq[cc][qi][qj] : 0.f;
                } else if constexpr (UNPOOL) {
                    const int qi = (PY + i) >> 1, qj = (PX + j) >> 1;
                    const bool ok = rok[i] && cok[j] && qrok[qi] && qcok[qj];
                    d[i][j] = (ok && pv[cc][i][j] == pq[cc][qi][qj]) ? uq[cc][qi][qj] : 0.f;
                } else {
                    d[i][j] = (rok[i] && cok[j]) ? pv[cc][i][j] : 0.f;
                }
            }
        float vv[16];
        wino_BtdB(d, vv);
        float* v = p.V + (size_t)c * p.Tpad + t;
#pragma unroll
        for (int x = 0; x < 16; ++x) v[(size_t)x * xis] = vv[x];
    }
}


// LDS-staged input transform for maps with >= 128 tiles per image: a workgroup takes 256
// consecutive tiles of ONE image, stages the input rows they touch (whole rows of the tile grid:
// coalesced loads, ~1.3 loads per tile and channel instead of 16; the DePool2D mask is applied per
// staged element, 3 loads instead of 34 per tile) and every thread reads its 4x4 patch from LDS.
constexpr int ILDS_E = 12, ILDS_CH = 8;   // staged elements per thread, channels per workgroup
// MB: mask bytes instead of pre / pooled, as in wino_input_kernel (2 loads per staged element).
template <bool UNPOOL, int NT, bool MB = false>
__global__ __launch_bounds__(NT) void wino_input_lds_kernel(const WinoParams p, const int chunks) {
    constexpr int ILDS_CAP = ILDS_E * NT;
    __shared__ __attribute__((aligned(16))) float Ls[2][ILDS_CAP];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
    const int ntt = p.nty * p.ntx;
    const int tl0 = chunk * NT, tl = tl0 + tid;
    const bool tvalid = tl < ntt;
    const int row_first = tl0 / p.ntx;
    const int row_last = min(ntt - 1, tl0 + NT - 1) / p.ntx;
    const int NR = 2 * (row_last - row_first + 1) + 2, NC = 2 * p.ntx + 2, NE = NR * NC;
    const int iyb = p.ty0 + 2 * row_first - p.pad, ixb = p.tx0 - p.pad;
    int goff[ILDS_E], qoff[UNPOOL ? ILDS_E : 1];
#pragma unroll
    for (int i = 0; i < ILDS_E; ++i) {
        const int e = i * NT + tid;
        const int r = e / NC, c = e - r * NC;
        const int iy = iyb + r, ix = ixb + c;
        bool ok = e < NE && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
        goff[i] = ok ? iy * p.W + ix : -1;
        if constexpr (UNPOOL) {
            ok = ok && iy < 2 * p.h2 && ix < 2 * p.w2;
            qoff[i] = ok ? (iy >> 1) * p.w2 + (ix >> 1) : -1;
            if constexpr (MB) goff[i] = (iy & 1) * 2 + (ix & 1);   // (pre is not read: the mask bit)
        }
    }
    const int tyl = tl / p.ntx, txl = tl - tyl * p.ntx;
    const int lbase = 2 * (tyl - row_first) * NC + 2 * txl;
    const size_t HW = (size_t)p.H * p.W, hw2 = (size_t)p.h2 * p.w2;
    const size_t xis = (size_t)p.Kc * p.Tpad;
    const int t = b * ntt + tl;
    const int c0 = blockIdx.y * ILDS_CH;
    float v[ILDS_E];

    auto fetch = [&](int c) __attribute__((always_inline)) {
        if constexpr (MB) {
            const uint8_t* mp = p.mask_in + ((size_t)b * p.C1 + c) * hw2;
            const float* upp = p.x1 + ((size_t)b * p.C1 + c) * hw2;
            uint32_t mq[ILDS_E];
            float uq[ILDS_E];
#pragma unroll
            for (int i = 0; i < ILDS_E; ++i) {
                const int qo = qoff[i] >= 0 ? qoff[i] : 0;
                mq[i] = mp[qo];
                uq[i] = upp[qo];
            }
#pragma unroll
            for (int i = 0; i < ILDS_E; ++i)
                v[i] = (qoff[i] >= 0 && ((mq[i] >> goff[i]) & 1u)) ? uq[i] : 0.f;
        } else if constexpr (UNPOOL) {
            const float* prep = p.pre + ((size_t)b * p.C1 + c) * HW;
            const float* poolp = p.pooled + ((size_t)b * p.C1 + c) * hw2;
            const float* upp = p.x1 + ((size_t)b * p.C1 + c) * hw2;
            // all three loads of every staged element unconditionally (offsets of elements outside
            // the 2h x 2w region clamped to 0 and masked afterwards): one batch in flight instead
            // of a dependent branch per element
            float pv[ILDS_E], pq[ILDS_E], uq[ILDS_E];
#pragma unroll
            for (int i = 0; i < ILDS_E; ++i) {
                const int go = qoff[i] >= 0 ? goff[i] : 0, qo = qoff[i] >= 0 ? qoff[i] : 0;
                pv[i] = prep[go];
                pq[i] = poolp[qo];
                uq[i] = upp[qo];
            }
#pragma unroll
            for (int i = 0; i < ILDS_E; ++i) v[i] = (qoff[i] >= 0 && pv[i] == pq[i]) ? uq[i] : 0.f;
        } else {
            const float* src = c < p.C1 ? p.x1 + ((size_t)b * p.C1 + c) * HW
                                        : p.x2 + ((size_t)b * p.C2 + (c - p.C1)) * HW;
            // (unconditional loads at clamped offsets, masked afterwards -- as above: one batch in flight)
            float pv[ILDS_E];
#pragma unroll
            for (int i = 0; i < ILDS_E; ++i) pv[i] = src[goff[i] >= 0 ? goff[i] : 0];
#pragma unroll
            for (int i = 0; i < ILDS_E; ++i) v[i] = goff[i] >= 0 ? pv[i] : 0.f;
        }
    };

    fetch(c0);
    for (int cc = 0; cc < ILDS_CH; ++cc) {
        const int c = c0 + cc;   // Kc is a multiple of 16: always a real (possibly zero-weight) channel
        float* L = Ls[cc & 1];
#pragma unroll
        for (int i = 0; i < ILDS_E; ++i)
            if (i * NT + tid < NE) L[i * NT + tid] = v[i];
        if (cc + 1 < ILDS_CH) fetch(c + 1);
        __syncthreads();
        if (tvalid) {
            float d[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float2 lo = *reinterpret_cast<const float2*>(L + lbase + i * NC);
                const float2 hi = *reinterpret_cast<const float2*>(L + lbase + i * NC + 2);
                d[i][0] = lo.x; d[i][1] = lo.y; d[i][2] = hi.x; d[i][3] = hi.y;
            }
            float e[4][4];
            wino_Btd(d, e);
            float* vo = p.V + (size_t)c * p.Tpad + t;
#pragma unroll
            for (int i = 0; i < 4; ++i) {  // (B^T d) B
                float r[4];
                wino_eB(e[i], r);
#pragma unroll
                for (int j = 0; j < 4; ++j) vo[(size_t)(i * 4 + j) * xis] = r[j];
            }
        }
    }
}

// Streaming input transform (plain and mask-byte inputs, every map size): a thread owns FOUR
// consecutive tiles t = 4q .. 4q + 3 of V's tile axis, so each of the 16 xi values of a channel
// leaves as one 16-byte store (1 KB per wave-instruction instead of 256 B), and a workgroup walks
// `chw` channels with its integer prologue computed once.  t runs over tile rows of all images
// laid end to end (t = gr * ntx + txl, gr = b * nty + tyl), so a workgroup's 4 * NT tiles may
// cover part of one image or many small ones; it stages, per image it touches, the input rows of
// the tile rows it holds (2 * rows + 2 each; element -> (image, iy, ix) is worked out once per
// thread), double-buffered in LDS, and every thread reads its four 4x4 patches from there.
// The next channel's loads are issued before the barrier and the previous channel's stores are
// never waited for, so both stay in flight across it.  Values: the same d, the same B^T d B
// expressions as the kernels above -- V is the same, bit for bit; nothing is written at t >= T.
constexpr int IW_E = 24;   // staged elements per thread (capacity IW_E * NT floats per buffer)

struct IwChunk {           // staged rows of the tiles [t0, t1): image b0 from tile row tyf, then whole images
    int b0, tyf, R0, RI, NR;
};

__host__ __device__ inline IwChunk iw_chunk(int t0, int t1, int ntx, int nty) {
    IwChunk k;
    const int gr0 = t0 / ntx, gr1 = (t1 - 1) / ntx;
    const int b1 = gr1 / nty, tyl = gr1 - b1 * nty;
    k.b0 = gr0 / nty;
    k.tyf = gr0 - k.b0 * nty;
    k.RI = 2 * nty + 2;
    if (k.b0 == b1) {
        k.R0 = 2 * (tyl - k.tyf + 1) + 2;
        k.NR = k.R0;
    } else {
        k.R0 = 2 * (nty - k.tyf) + 2;
        k.NR = k.R0 + (b1 - k.b0 - 1) * k.RI + 2 * (tyl + 1) + 2;
    }
    return k;
}

// packed staging offset: bits 0..19 the offset inside one plane (mask bytes: (offset << 2) | bit),
// bits 20.. the image relative to the chunk's first.  Elements that are zero (outside the map, not
// staged) load offset 0 and have their bit clear in the thread's mask `okm`.
constexpr int IW_PBITS = 20;
static_assert(IW_E <= 32, "one validity bit per staged element");

// TPT = 2 (wino_input_narrow below): TWO consecutive tiles per thread, half the staged elements, offsets and
// results, 8-byte stores -- 24 KB of LDS and a register count that fits beside the GEMM's waves on a compute unit.
template <bool MB, int NT, int TPT = 4>
__global__ __launch_bounds__(NT, TPT == 2 ? 4 : 1) void wino_input_wide_kernel(const WinoParams p, const int chw) {
    static_assert(TPT == 4 || TPT == 2, "a quad or a pair of tiles per thread");
    constexpr int E = IW_E * TPT / 4;   // staged elements per thread
    __shared__ __attribute__((aligned(16))) float Ls[2][E * NT];
    const int tid = threadIdx.x;
    const int tw0 = blockIdx.x * (TPT * NT), tw1 = min(tw0 + TPT * NT, p.T);
    const IwChunk k = iw_chunk(tw0, tw1, p.ntx, p.nty);
    const int NC = 2 * p.ntx + 2, NE = k.NR * NC;
    const int iyb = p.ty0 - p.pad, ixb = p.tx0 - p.pad;
    uint32_t pk[E], okm = 0;
#pragma unroll
    for (int i = 0; i < E; ++i) {
        const int e = i * NT + tid;
        const int r = e / NC, c = e - r * NC;
        int bi = 0, ry = 2 * k.tyf + r;
        if (r >= k.R0) {
            const int r2 = r - k.R0;
            bi = r2 / k.RI;
            ry = r2 - bi * k.RI;
            bi += 1;
        }
        const int iy = iyb + ry, ix = ixb + c;
        bool ok = e < NE && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
        int po = iy * p.W + ix;
        if constexpr (MB) {
            ok = ok && iy < 2 * p.h2 && ix < 2 * p.w2;
            po = (((iy >> 1) * p.w2 + (ix >> 1)) << 2) | ((iy & 1) * 2 + (ix & 1));
        }
        pk[i] = ok ? ((uint32_t)bi << IW_PBITS) | (uint32_t)po : 0u;
        okm |= (ok ? 1u : 0u) << i;
    }
    // the thread's four tiles: first staged element of each 4x4 patch
    const int q4 = tw0 + TPT * tid;
    int lbase[TPT];
#pragma unroll
    for (int j = 0; j < TPT; ++j) {
        const int t = min(q4 + j, tw1 - 1);
        const int gr = t / p.ntx, txl = t - gr * p.ntx;
        const int b = gr / p.nty, ty = gr - b * p.nty;
        const int row = b == k.b0 ? 2 * (ty - k.tyf) : k.R0 + (b - k.b0 - 1) * k.RI + 2 * ty;
        lbase[j] = row * NC + 2 * txl;
    }
    const int nv = min(TPT, tw1 - q4);   // tiles of the quad below T (<= 0: none)
    const int HW = p.H * p.W, hw2 = p.h2 * p.w2;
    const size_t xis = (size_t)p.Kc * p.Tpad;
    const int c0 = blockIdx.y * chw;
    constexpr uint32_t PM = (1u << IW_PBITS) - 1;
    float v[E];
    uint32_t mq[MB ? E : 1];

    // all loads of a channel unconditionally, one batch in flight (32-bit byte offsets from the
    // plane of the chunk's first image); they are masked only where they are written to LDS, one
    // barrier later, so nothing here waits for them
    auto fetch = [&](int c) __attribute__((always_inline)) {
        if constexpr (MB) {
            const uint32_t ist = (uint32_t)(p.C1 * hw2);
            const uint8_t* mp = p.mask_in + ((size_t)k.b0 * p.C1 + c) * hw2;
            const char* upp = reinterpret_cast<const char*>(p.x1 + ((size_t)k.b0 * p.C1 + c) * hw2);
#pragma unroll
            for (int i = 0; i < E; ++i) {
                // (TPT = 2: the offsets are formed again for every channel, not kept in registers across the loop)
                if constexpr (TPT == 2) asm volatile("" : "+v"(pk[i]));
                const uint32_t o = (pk[i] >> IW_PBITS) * ist + ((pk[i] & PM) >> 2);
                mq[i] = mp[o];
                v[i] = *reinterpret_cast<const float*>(upp + 4u * o);
            }
        } else {
            const bool first = c < p.C1;
            const uint32_t ist = (uint32_t)((first ? p.C1 : p.C2) * HW);
            const char* src = reinterpret_cast<const char*>(
                first ? p.x1 + ((size_t)k.b0 * p.C1 + c) * HW
                      : p.x2 + ((size_t)k.b0 * p.C2 + (c - p.C1)) * HW);
#pragma unroll
            for (int i = 0; i < E; ++i)
                v[i] = *reinterpret_cast<const float*>(src + 4u * ((pk[i] >> IW_PBITS) * ist + (pk[i] & PM)));
        }
    };

    // FULL: every quad of the workgroup lies below T (all workgroups but the last along x).  Its
    // loop has no branch between a channel's loads and the stores that follow them, so the wait
    // before the LDS writes counts those 16 stores out and leaves them in flight; the other form's
    // store count depends on the lane, and its waits are for everything.
    auto run = [&](auto FULLC) __attribute__((always_inline)) {
    constexpr bool FULL = decltype(FULLC)::value;
    fetch(c0);
    for (int cc = 0; cc < chw; ++cc) {
        const int c = c0 + cc;
        float* L = Ls[cc & 1];
#pragma unroll
        for (int i = 0; i < E; ++i) {   // (every slot of the buffer: those past the staged rows get 0)
            bool on = (okm >> i) & 1u;
            if constexpr (MB) on = on && ((mq[i] >> (pk[i] & 3u)) & 1u);
            L[i * NT + tid] = on ? v[i] : 0.f;
        }
        if (cc + 1 < chw) fetch(c + 1);
        __syncthreads();
        if constexpr (!FULL)
            if (nv <= 0) continue;
        // row i of B^T d needs two rows of d only (d0 - d2, d1 + d2, d2 - d1, d1 - d3): the four
        // xi planes of one i at a time keep the live values of a thread's four tiles small
        float* vo = p.V + (size_t)c * p.Tpad + q4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            constexpr int RA[4] = {0, 1, 2, 1}, RB[4] = {2, 2, 1, 3};
            float o[4][TPT];
#pragma unroll
            for (int j = 0; j < TPT; ++j) {
                const float* La = L + lbase[j] + RA[i] * NC;
                const float* Lb = L + lbase[j] + RB[i] * NC;
                const float2 alo = *reinterpret_cast<const float2*>(La);
                const float2 ahi = *reinterpret_cast<const float2*>(La + 2);
                const float2 blo = *reinterpret_cast<const float2*>(Lb);
                const float2 bhi = *reinterpret_cast<const float2*>(Lb + 2);
                const float da[4] = {alo.x, alo.y, ahi.x, ahi.y}, db[4] = {blo.x, blo.y, bhi.x, bhi.y};
                // (row i of wino_Btd, written out: the helper takes all four rows of d, and this kernel is
                // built around holding two of them; then wino_eB's expressions on four tiles side by side)
                float e[4];
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) e[jj] = i == 1 ? da[jj] + db[jj] : da[jj] - db[jj];   // B^T d
                o[0][j] = e[0] - e[2];   // (B^T d) B
                o[1][j] = e[1] + e[2];
                o[2][j] = e[2] - e[1];
                o[3][j] = e[1] - e[3];
            }
            if (FULL || nv == TPT) {
#pragma unroll
                for (int x = 0; x < 4; ++x)
                    if constexpr (TPT == 4)
                        *reinterpret_cast<float4*>(vo + (size_t)(i * 4 + x) * xis) =
                            make_float4(o[x][0], o[x][1], o[x][2], o[x][3]);
                    else
                        *reinterpret_cast<float2*>(vo + (size_t)(i * 4 + x) * xis) = make_float2(o[x][0], o[x][1]);
            } else {   // the quad that holds T: the tiles below T, one by one
#pragma unroll
                for (int x = 0; x < 4; ++x)
#pragma unroll
                    for (int j = 0; j < TPT - 1; ++j)
                        if (j < nv) vo[(size_t)(i * 4 + x) * xis + j] = o[x][j];
            }
        }
    }
    };
    if (tw0 + TPT * NT <= p.T) run(std::true_type{});
    else run(std::false_type{});
}

// ---- 2. the 16 GEMMs ---------------------------------------------------------------------------
// SLIM (wino_gemm_slim below): the same loads, MFMAs and stores with less addressing held in vector registers, so
// that four waves per SIMD leave room for a fifth of another kernel.  One lane offset per operand serves every
// LDS-DMA load (the row block of a load, the k-tile, m0 / t0 are wave-uniform and ride on the scalar offset), and one
// LDS read base per operand serves every read (the k row, the 32-column block and the ring slot are constants).
template <int BM, int BN, int WM, int WN, int NBUF, int BK = 16, bool SLIM = false>
__global__ __launch_bounds__(WM * WN * 64, 2) void wino_gemm_kernel(const WinoParams p) {
    constexpr int NCH = BK / 2;
    constexpr int WTM = BM / WM, WTN = BN / WN;
    constexpr int TM = WTM / 32, TN = WTN / 32;
    constexpr int NW = WM * WN, NT = NW * 64;
    constexpr int AV = BK * BM / 4, BV = BK * BN / 4;  // float4 per operand tile
    constexpr int NA = NW == 8 ? 256 : NT;             // threads staging A / B
    constexpr int APT = AV / NA, BPT = BV / 256;
    static_assert((NW == 4 || NW == 8) && AV % NA == 0 && BV % 256 == 0, "tile config");

    __shared__ __attribute__((aligned(16))) float As[NBUF][BK][BM];
    __shared__ __attribute__((aligned(16))) float Bs[NBUF][BK][BN];

    // XCD-aware order: each XCD (bid % 8) walks a contiguous run of (xi, tile) work, inside a
    // run groups of 8 pixel-tiles x all channel-tiles share U and V rows in that XCD's L2
    const int per_xi = p.n_ttiles * p.n_mtiles;
    int xi, tt, mt;
    {
        const int nb = gridDim.x, bid = blockIdx.x;
        const int q = nb / 8, r = nb % 8, xcd = bid % 8, l = bid / 8;
        const int v = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + l;
        xi = v / per_xi;
        const int w = v - xi * per_xi;
        constexpr int GP = 8;
        const int gsize = GP * p.n_mtiles;
        const int g = w / gsize, rr = w % gsize;
        const int gp = min(GP, p.n_ttiles - g * GP);
        tt = g * GP + rr % gp;
        mt = rr / gp;
    }
    const int m0 = mt * BM, t0 = tt * BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int l31 = lane & 31, lh = lane >> 5;

    const __amdgpu_buffer_rsrc_t arsrc = mk_rsrc(p.U + (size_t)xi * p.Kc * p.Mpad, p.Kc * p.Mpad * 4);
    const __amdgpu_buffer_rsrc_t brsrc = mk_rsrc(p.V + (size_t)xi * p.Kc * p.Tpad, p.Kc * p.Tpad * 4);
    const bool bstager = NW == 4 || wave < 4;   // wave-uniform roles
    const bool astager = NW == 4 || wave >= 4;
    const int atid = NW == 8 ? tid - 256 : tid;
    const int awave = NW == 8 ? wave - 4 : wave;
    // SLIM: a 64-lane load covers 64 / RA rows of A (RA lanes per row); a lane's place inside it never changes
    constexpr int RA = BM / 4, RB = BN / 4;
    static_assert(RA <= 64 && RB <= 64 && 64 % RA == 0 && 64 % RB == 0, "whole rows per 64-lane load");
    const unsigned avo = 4u * (unsigned)((lane / RA) * p.Mpad + (lane % RA) * 4);
    const unsigned bvo = 4u * (unsigned)((lane / RB) * p.Tpad + (lane % RB) * 4);
    const int awave_u = __builtin_amdgcn_readfirstlane(awave), bwave_u = __builtin_amdgcn_readfirstlane(wave & 3);
    const unsigned aso = 4u * (unsigned)(awave_u * (64 / RA) * p.Mpad + m0);
    const unsigned bso = 4u * (unsigned)(bwave_u * (64 / RB) * p.Tpad + t0);

    // global -> LDS directly, 16 bytes per lane: thread-linear == LDS-linear
#define WINO_STAGE(KT, BUF)                                                                        \
    {                                                                                              \
        if (astager)                                                                               \
            static_for<0, APT>([&](auto J) __attribute__((always_inline)) {                        \
                constexpr int j = decltype(J)::value;                                              \
                const int f = j * NA + atid;                                                       \
                const int row = f / (BM / 4), c4 = f % (BM / 4);                                   \
                if constexpr (SLIM)                                                                \
                __builtin_amdgcn_raw_ptr_buffer_load_lds(                                          \
                    arsrc,                                                                         \
                    (__attribute__((address_space(3))) void*)(&As[BUF][0][0] + (j * NA + awave_u * 64) * 4), \
                    16, (int)avo, (int)(aso + 4u * (unsigned)(((KT) * BK + j * NA / RA) * p.Mpad)), 0, 0); \
                else                                                                               \
                __builtin_amdgcn_raw_ptr_buffer_load_lds(                                          \
                    arsrc,                                                                         \
                    (__attribute__((address_space(3))) void*)(&As[BUF][0][0] + (j * NA + awave * 64) * 4), \
                    16, (int)(4u * (unsigned)(((KT) * BK + row) * p.Mpad + m0 + c4 * 4)), 0, 0, 0); \
            });                                                                                    \
        if (bstager)                                                                               \
            static_for<0, BPT>([&](auto J) __attribute__((always_inline)) {                        \
                constexpr int j = decltype(J)::value;                                              \
                const int f = j * 256 + (tid & 255);                                               \
                const int row = f / (BN / 4), c4 = f % (BN / 4);                                   \
                if constexpr (SLIM)                                                                \
                __builtin_amdgcn_raw_ptr_buffer_load_lds(                                          \
                    brsrc,                                                                         \
                    (__attribute__((address_space(3))) void*)(&Bs[BUF][0][0] + (j * 256 + bwave_u * 64) * 4), \
                    16, (int)bvo, (int)(bso + 4u * (unsigned)(((KT) * BK + j * 256 / RB) * p.Tpad)), 0, 0); \
                else                                                                               \
                __builtin_amdgcn_raw_ptr_buffer_load_lds(                                          \
                    brsrc,                                                                         \
                    (__attribute__((address_space(3))) void*)(&Bs[BUF][0][0] + (j * 256 + (wave & 3) * 64) * 4), \
                    16, (int)(4u * (unsigned)(((KT) * BK + row) * p.Tpad + t0 + c4 * 4)), 0, 0, 0); \
            });                                                                                    \
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nkt = p.Kc / BK;
    // NBUF-deep ring of LDS tiles: tile kt+NBUF-1 is requested while tile kt is multiplied, so a
    // global -> LDS transfer has NBUF-1 tiles of MFMA work to land.  vmcnt counts this wave's
    // own outstanding DMA ops, in order: leaving one stage's worth in flight means every older
    // stage has landed.
    constexpr int OPS_A = APT, OPS_B = BPT;
#define WINO_WAIT_ONE_STAGE_IN_FLIGHT()                                                            \
    {                                                                                              \
        if constexpr (NW == 8) {                                                                   \
            if (astager) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(OPS_A) : "memory");              \
            else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(OPS_B) : "memory");                      \
        } else {                                                                                   \
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(OPS_A + OPS_B) : "memory");                   \
        }                                                                                          \
    }
    WINO_STAGE(0, 0)
    if constexpr (NBUF == 3) {
        if (nkt > 1) {
            WINO_STAGE(1, 1)
            WINO_WAIT_ONE_STAGE_IN_FLIGHT()
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();

    int buf = 0;
    for (int kt = 0; kt < nkt; ++kt) {
        const bool more = kt + NBUF - 1 < nkt;
        int sbuf = buf + NBUF - 1;               // ring slot of the tile requested now
        if (sbuf >= NBUF) sbuf -= NBUF;
        float a[2][TM], b[2][TN];
        // (SLIM: the lane's column in k row lh of this ring slot; As[buf][kk][..] is then ap[a constant])
        const float* ap = &As[SLIM ? buf : 0][lh][wm * WTM + l31];
        const float* bp = &Bs[SLIM ? buf : 0][lh][wn * WTN + l31];
#pragma unroll
        for (int i = 0; i < TM; ++i) a[0][i] = SLIM ? ap[i * 32] : As[buf][lh][wm * WTM + i * 32 + l31];
#pragma unroll
        for (int j = 0; j < TN; ++j) b[0][j] = SLIM ? bp[j * 32] : Bs[buf][lh][wn * WTN + j * 32 + l31];
        static_for<0, NCH>([&](auto CH) __attribute__((always_inline)) {
            constexpr int ch = decltype(CH)::value;
            if constexpr (ch + 1 < NCH) {
                const int kk = (ch + 1) * 2 + lh;
#pragma unroll
                for (int i = 0; i < TM; ++i)
                    a[(ch + 1) & 1][i] = SLIM ? ap[(ch + 1) * 2 * BM + i * 32] : As[buf][kk][wm * WTM + i * 32 + l31];
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    b[(ch + 1) & 1][j] = SLIM ? bp[(ch + 1) * 2 * BN + j * 32] : Bs[buf][kk][wn * WTN + j * 32 + l31];
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ch & 1][i], b[ch & 1][j],
                                                                     acc[i][j], 0, 0, 0);
            if constexpr (ch == 0) {
                if (more) WINO_STAGE(kt + NBUF - 1, sbuf)
            }
            __builtin_amdgcn_sched_barrier(0);
        });
        if (NBUF == 3 && more) {
            WINO_WAIT_ONE_STAGE_IN_FLIGHT()
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();
        if (++buf == NBUF) buf = 0;
    }
#undef WINO_STAGE
#undef WINO_WAIT_ONE_STAGE_IN_FLIGHT

    // rows of the C/D layout are channels, columns (lane & 31) are tiles
    float* Mx = p.M + (size_t)xi * p.Mpad * p.Tpad;
    if (p.mq) {
        // M[xi][co / 4][t][4]: a lane's registers r & 3 = 0..3 are four consecutive channels of one
        // tile, one 16-byte store; the lane's byte offset is formed once, the quad row (i, r >> 2)
        // and the column block j are wave-uniform and ride on the scalar offset
        const __amdgpu_buffer_rsrc_t mr = mk_rsrc(Mx, p.Mpad * p.Tpad * 4);
        const unsigned qrow = 16u * (unsigned)p.Tpad;   // bytes of one channel quad over all tiles
        const unsigned lo = (unsigned)((m0 + wm * WTM) / 4 + lh) * qrow + 16u * (unsigned)(t0 + wn * WTN + l31);
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 v = {acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2],
                                     acc[i][j][4 * q + 3]};
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), mr, (int)lo,
                                                           (int)((unsigned)(i * 8 + 2 * q) * qrow + 512u * j), 0);
                }
        return;
    }
    // M[xi][co][t]
    if constexpr (SLIM) {
        // a scalar base per (wave, i, r, j) and ONE 32-bit lane offset, 4 * lh rows and the column
        // (16 * Tpad bytes fit: wino_geometry bounds Tpad * Kc * 4, Kc >= 16), not a 64-bit address per store
        const int wm_u = __builtin_amdgcn_readfirstlane(wm), wn_u = __builtin_amdgcn_readfirstlane(wn);
        char* mb = reinterpret_cast<char*>(Mx + (size_t)(m0 + wm_u * WTM) * p.Tpad + t0 + wn_u * WTN);
        const unsigned lo = 4u * (unsigned)(4 * lh * p.Tpad + l31);
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    *reinterpret_cast<float*>(mb + ((size_t)(i * 32 + (r & 3) + 8 * (r >> 2)) * p.Tpad + j * 32) * 4 + lo) =
                        acc[i][j][r];
        return;
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int t = t0 + wn * WTN + j * 32 + l31;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = m0 + wm * WTM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                Mx[(size_t)co * p.Tpad + t] = acc[i][j][r];
            }
    }
}

// ---- 2+3 fused: one workgroup walks all 16 xi of its (channel, tile) block ------------------------
// M_xi lives in registers only: after the K loop of each xi it is folded into the four output
// accumulators Y_ab += AT[a][i] * AT[b][j] * M_xi (coefficients 0 / +-1, xi = 4i + j), so the
// products never travel to HBM and the output transform costs 4 FMAs per element per xi.
template <int BM, int BN, int WM, int WN, int BK, int MINW>
__global__ __launch_bounds__(WM * WN * 64, MINW) void wino_fused_kernel(const WinoParams p) {
    constexpr int NCH = BK / 2;
    constexpr int WTM = BM / WM, WTN = BN / WN;
    constexpr int TM = WTM / 32, TN = WTN / 32;
    constexpr int NT = WM * WN * 64;
    constexpr int AV = BK * BM / 4, BV = BK * BN / 4;
    constexpr int APT = AV / NT, BPT = BV / NT;
    static_assert(AV % NT == 0 && BV % NT == 0, "tile config");

    __shared__ __attribute__((aligned(16))) float As[2][BK][BM];
    __shared__ __attribute__((aligned(16))) float Bs[2][BK][BN];

    int tt, mt;
    tile_of_block(blockIdx.x, gridDim.x, p.n_ttiles, p.n_mtiles, tt, mt);
    const int m0 = mt * BM, t0 = tt * BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int l31 = lane & 31, lh = lane >> 5;
    const int nkt = p.Kc / BK;
    const size_t ustride = (size_t)p.Kc * p.Mpad, vstride = (size_t)p.Kc * p.Tpad;
    const int ubytes = p.Kc * p.Mpad * 4, vbytes = p.Kc * p.Tpad * 4;

    // stage k-tile KT of transform point XI into LDS buffer BUF (global -> LDS, 16 B per lane)
#define WINO_STAGE(XI, KT, BUF)                                                                    \
    {                                                                                              \
        const __amdgpu_buffer_rsrc_t ar = mk_rsrc(p.U + (size_t)(XI) * ustride, ubytes);           \
        const __amdgpu_buffer_rsrc_t br = mk_rsrc(p.V + (size_t)(XI) * vstride, vbytes);           \
        static_for<0, APT>([&](auto J) __attribute__((always_inline)) {                            \
            constexpr int j = decltype(J)::value;                                                  \
            const int f = j * NT + tid;                                                            \
            const int row = f / (BM / 4), c4 = f % (BM / 4);                                       \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(                                              \
                ar, (__attribute__((address_space(3))) void*)(&As[BUF][0][0] + (j * NT + wave * 64) * 4), \
                16, (int)(4u * (unsigned)(((KT) * BK + row) * p.Mpad + m0 + c4 * 4)), 0, 0, 0);    \
        });                                                                                        \
        static_for<0, BPT>([&](auto J) __attribute__((always_inline)) {                            \
            constexpr int j = decltype(J)::value;                                                  \
            const int f = j * NT + tid;                                                            \
            const int row = f / (BN / 4), c4 = f % (BN / 4);                                       \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(                                              \
                br, (__attribute__((address_space(3))) void*)(&Bs[BUF][0][0] + (j * NT + wave * 64) * 4), \
                16, (int)(4u * (unsigned)(((KT) * BK + row) * p.Tpad + t0 + c4 * 4)), 0, 0, 0);    \
        });                                                                                        \
    }

    f32x16 acc[TM][TN], Y[4][TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                acc[i][j][r] = 0.f;
                Y[0][i][j][r] = Y[1][i][j][r] = Y[2][i][j][r] = Y[3][i][j][r] = 0.f;
            }

    WINO_STAGE(0, 0, 0)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    int xi = 0, kt = 0;              // the k-tile being multiplied
    const int total = 16 * nkt;
    for (int s = 0; s < total; ++s) {
        const int buf = s & 1;
        int nxi = xi, nkt1 = kt + 1;  // the k-tile being staged
        if (nkt1 == nkt) { nkt1 = 0; ++nxi; }
        const bool more = s + 1 < total;
        float a[2][TM], b[2][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) a[0][i] = As[buf][lh][wm * WTM + i * 32 + l31];
#pragma unroll
        for (int j = 0; j < TN; ++j) b[0][j] = Bs[buf][lh][wn * WTN + j * 32 + l31];
        static_for<0, NCH>([&](auto CH) __attribute__((always_inline)) {
            constexpr int ch = decltype(CH)::value;
            if constexpr (ch + 1 < NCH) {
                const int kk = (ch + 1) * 2 + lh;
#pragma unroll
                for (int i = 0; i < TM; ++i) a[(ch + 1) & 1][i] = As[buf][kk][wm * WTM + i * 32 + l31];
#pragma unroll
                for (int j = 0; j < TN; ++j) b[(ch + 1) & 1][j] = Bs[buf][kk][wn * WTN + j * 32 + l31];
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ch & 1][i], b[ch & 1][j],
                                                                     acc[i][j], 0, 0, 0);
            if constexpr (ch == 0) {
                if (more) WINO_STAGE(nxi, nkt1, buf ^ 1)
            }
            __builtin_amdgcn_sched_barrier(0);
        });
        if (nkt1 == 0) {
            // M_xi complete: Y_ab += AT[a][xi/4] * AT[b][xi%4] * M_xi,  AT = [1 1 1 0; 0 1 -1 -1]
            const int wi = xi >> 2, wj = xi & 3;
            const float r0 = wi < 3 ? 1.f : 0.f, r1 = wi == 0 ? 0.f : (wi == 1 ? 1.f : -1.f);
            const float c0 = wj < 3 ? 1.f : 0.f, c1 = wj == 0 ? 0.f : (wj == 1 ? 1.f : -1.f);
            const float k00 = r0 * c0, k01 = r0 * c1, k10 = r1 * c0, k11 = r1 * c1;
            // coefficients are 0 / +-1 and wave-uniform: skip the accumulators xi does not reach
#define WINO_FOLD(Q, KQ)                                                                            \
            if ((KQ) != 0.f) {                                                                      \
                _Pragma("unroll") for (int i = 0; i < TM; ++i)                                      \
                _Pragma("unroll") for (int j = 0; j < TN; ++j)                                      \
                _Pragma("unroll") for (int r = 0; r < 16; ++r)                                      \
                    Y[Q][i][j][r] = fmaf((KQ), acc[i][j][r], Y[Q][i][j][r]);                        \
            }
            WINO_FOLD(0, k00)
            WINO_FOLD(1, k01)
            WINO_FOLD(2, k10)
            WINO_FOLD(3, k11)
#undef WINO_FOLD
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        }
        xi = nxi;
        kt = nkt1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
#undef WINO_STAGE

    // epilogue: rows of the C/D layout are channels, columns (lane & 31) are tiles.  A tile's two
    // pixels of a row go out as ONE 8-byte store (lanes are consecutive tiles: 256 contiguous bytes
    // per 32 lanes) wherever both columns are inside the window; the channel offsets are formed once
    // per (i, r) from 32-bit products.
    const int ntt = p.nty * p.ntx;
    const size_t OPL = (size_t)p.out_H * p.out_W, APL = (size_t)p.AH * p.AW;
    // The tile's BM bias values go through LDS (free after the last k-tile's barrier): read from global per
    // (i, r) each of them is a vector load that cannot move above the stores in front of it -- 16 TM TN
    // dependent memory round trips at the end of every workgroup; LDS reads are not held back by global stores.
    float* Lbias = &As[0][0][0];
    for (int f = tid; f < BM; f += NT) Lbias[f] = (p.bias && m0 + f < p.Cout) ? p.bias[m0 + f] : 0.f;
    __syncthreads();
    float bias_r[TM][16];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) bias_r[i][r] = Lbias[wm * WTM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int t = t0 + wn * WTN + j * 32 + l31;
        if (t >= p.T) continue;
        const int b = t / ntt;
        const int rr = t - b * ntt;
        const int tyl = rr / p.ntx, txl = rr - tyl * p.ntx;
        const int wy = p.ty0 + 2 * tyl - p.oy0, wx = p.tx0 + 2 * txl - p.ox0;
        const bool rok[2] = {(unsigned)wy < (unsigned)p.OH, (unsigned)(wy + 1) < (unsigned)p.OH};
        const bool cok[2] = {(unsigned)wx < (unsigned)p.OW, (unsigned)(wx + 1) < (unsigned)p.OW};
        const bool pair = cok[0] && cok[1];
        const bool whole = p.pool && rok[1] && cok[1];   // even anchor: the tile is a pooling window
        float* ob = p.out ? p.out + ((size_t)b * p.out_ctot + p.out_c0) * OPL +
                                (ptrdiff_t)(p.out_y0 + wy) * p.out_W + p.out_x0 + wx
                          : nullptr;
        const float* ab = p.add ? p.add + (size_t)b * p.Cout * APL +
                                      (ptrdiff_t)(p.ay0 + wy) * p.AW + p.ax0 + wx
                                : nullptr;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = m0 + wm * WTM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (co >= p.Cout) continue;
                const float bias = bias_r[i][r];
                float* oc = ob ? ob + (size_t)co * OPL : nullptr;
                const float* ac = ab ? ab + (size_t)co * APL : nullptr;
                if (whole) {   // all four inside the window: values for the pool (+ the plain stores)
                    float v[2][2];
#pragma unroll
                    for (int a = 0; a < 2; ++a) {
                        v[a][0] = Y[2 * a][i][j][r] + bias;
                        v[a][1] = Y[2 * a + 1][i][j][r] + bias;
                        if (ac) {
                            const f32x2u a2 = *reinterpret_cast<const f32x2u*>(ac + a * p.AW);
                            v[a][0] += a2[0];
                            v[a][1] += a2[1];
                        }
                        if (p.relu) {
                            v[a][0] = fmaxf(v[a][0], 0.f);
                            v[a][1] = fmaxf(v[a][1], 0.f);
                        }
                        if (oc) *reinterpret_cast<f32x2u*>(oc + (size_t)a * p.out_W) = f32x2u{v[a][0], v[a][1]};
                    }
                    pool_store(p, b, co, p.oy0 + wy, p.ox0 + wx, v[0][0], v[0][1], v[1][0], v[1][1]);
                    continue;
                }
                if (!oc) continue;
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    if (!rok[a]) continue;
                    float v0 = Y[2 * a][i][j][r] + bias, v1 = Y[2 * a + 1][i][j][r] + bias;
                    if (pair) {
                        if (ac) {
                            const f32x2u a2 = *reinterpret_cast<const f32x2u*>(ac + a * p.AW);
                            v0 += a2[0];
                            v1 += a2[1];
                        }
                        if (p.relu) {
                            v0 = fmaxf(v0, 0.f);
                            v1 = fmaxf(v1, 0.f);
                        }
                        *reinterpret_cast<f32x2u*>(oc + (size_t)a * p.out_W) = f32x2u{v0, v1};
                    } else {
                        if (cok[0]) {
                            if (ac) v0 += ac[a * p.AW];
                            if (p.relu) v0 = fmaxf(v0, 0.f);
                            oc[(size_t)a * p.out_W] = v0;
                        }
                        if (cok[1]) {
                            if (ac) v1 += ac[a * p.AW + 1];
                            if (p.relu) v1 = fmaxf(v1, 0.f);
                            oc[(size_t)a * p.out_W + 1] = v1;
                        }
                    }
                }
            }
    }
}

// ---- 3. output transform + epilogue ------------------------------------------------------------
// QUAD: M is M[xi][Mpad / 4][Tpad][4] -- the thread's four channels of one xi are one 16-byte load
// (a quad that straddles Cout is read whole: rows up to Mpad exist) -- and a tile row with both
// columns inside the window is one 8-byte store.  Same arithmetic, same bits as the other form.
constexpr int OCH = 4;
template <bool QUAD>
__global__ __launch_bounds__(256) void wino_output_kernel(const WinoParams p) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= p.T) return;
    const WinoTile tile(p, t);
    const int b = tile.b, wy = tile.y - p.oy0, wx = tile.x - p.ox0;  // window coords
    const bool okr[2] = {(unsigned)wy < (unsigned)p.OH, (unsigned)(wy + 1) < (unsigned)p.OH};
    const bool okc[2] = {(unsigned)wx < (unsigned)p.OW, (unsigned)(wx + 1) < (unsigned)p.OW};
    const size_t xis = (size_t)p.Mpad * p.Tpad;
    const size_t OPL = (size_t)p.out_H * p.out_W, APL = (size_t)p.AH * p.AW;
    const int co0 = blockIdx.y * OCH;
    // All loads of the thread's OCH channels first (M, skip-add; channel index clamped instead of
    // branching), then the stores: `out` may alias `M` / `add` as far as the compiler knows, so
    // loads placed after a store could not be moved up and every channel would be a round trip.
    float mv[OCH][16], av[OCH][4], bv[OCH];
    if constexpr (QUAD) {
        static_assert(OCH == 4, "one channel quad per thread");
        // a buffer descriptor per slice (a slice fits 32-bit byte offsets: m_quad) and ONE byte offset
        // per thread, the same in all 16
        const unsigned mo = 16u * ((unsigned)blockIdx.y * (unsigned)p.Tpad + (unsigned)t);
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            const f32x4 q = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                mk_rsrc(p.M + (size_t)x * xis, p.Mpad * p.Tpad * 4), (int)mo, 0, 0));
#pragma unroll
            for (int cc = 0; cc < OCH; ++cc) mv[cc][x] = q[cc];
        }
    }
#pragma unroll
    for (int cc = 0; cc < OCH; ++cc) {
        const int co = min(co0 + cc, p.Cout - 1);
        if constexpr (QUAD) {
            bv[cc] = p.bias ? p.bias[co] : 0.f;
        } else {
            const float* m = p.M + (size_t)co * p.Tpad + t;
#pragma unroll
            for (int x = 0; x < 16; ++x) mv[cc][x] = m[(size_t)x * xis];
        }
        if (p.add) {
            const float* ad = p.add + ((size_t)b * p.Cout + co) * APL;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const bool ok = okr[i] && okc[j];
                    const ptrdiff_t idx = (ptrdiff_t)(p.ay0 + wy + i) * p.AW + p.ax0 + wx + j;
                    const float a = ad[ok ? idx : 0];
                    // (QUAD: a value outside the window is neither stored nor pooled -- a pooled tile
                    // lies inside it whole, wino_pool_ok -- and selecting here would wait for this
                    // channel's loads before the next channel's are issued)
                    av[cc][i * 2 + j] = QUAD || ok ? a : 0.f;
                }
        }
    }
    // QUAD: the first channel's address once per thread, the others one plane further each
    float* const ob = QUAD && p.out ? p.out + ((size_t)b * p.out_ctot + p.out_c0 + co0) * OPL +
                                          (ptrdiff_t)(p.out_y0 + wy) * p.out_W + p.out_x0 + wx
                                    : nullptr;
    const bool pair = okc[0] && okc[1];
#pragma unroll
    for (int cc = 0; cc < OCH; ++cc) {
        const int co = co0 + cc;
        if (co >= p.Cout) break;
        float s2[2][4];
        wino_Atm(mv[cc], s2);
        float bias;
        float* o;
        if constexpr (QUAD) {
            bias = bv[cc];
            o = ob ? ob + cc * OPL : nullptr;
        } else {
            bias = p.bias ? p.bias[co] : 0.f;
            o = p.out ? p.out + ((size_t)b * p.out_ctot + p.out_c0 + co) * OPL +
                            (ptrdiff_t)(p.out_y0 + wy) * p.out_W + p.out_x0 + wx
                      : nullptr;
        }
        float vt[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {  // (A^T m) A
            float y[2];
            wino_sA(s2[i], y);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                float v = y[j] + bias;
                if (p.add) v += av[cc][i * 2 + j];
                if (p.relu) v = fmaxf(v, 0.f);
                vt[i][j] = v;
                if constexpr (!QUAD)
                    if (o && okr[i] && okc[j]) o[(ptrdiff_t)i * p.out_W + j] = v;
            }
            if constexpr (QUAD) {
                if (o && okr[i]) {
                    float* orow = o + (ptrdiff_t)i * p.out_W;
                    if (pair) {
                        *reinterpret_cast<f32x2u*>(orow) = f32x2u{vt[i][0], vt[i][1]};
                    } else {   // a tile cut by the window's edge
                        if (okc[0]) orow[0] = vt[i][0];
                        if (okc[1]) orow[1] = vt[i][1];
                    }
                }
            }
        }
        // even anchor: the tile is one pooling window; a tile cut by the window's end is the map's
        // unpaired last row / column (the caller launches whole windows) and has no pooled value
        if (p.pool && okr[1] && okc[1])
            pool_store(p, b, co, p.oy0 + wy, p.ox0 + wx, vt[0][0], vt[0][1], vt[1][0], vt[1][1]);
    }
}

// geometry shared by the sizing queries and the launcher
struct WinoGeom {
    int Kc, Mpad, bm, ty0, tx0, nty, ntx, T, Tpad;
};

int wino_geom(const iiseg_conv_desc* d, WinoGeom& g) {
    WinoTiles w;
    const int st = wino_tiles(d, w, 16);
    if (st) return st;
    g.Kc = d->C1 + d->C2;
    g.bm = d->Cout > 128 ? 256 : (d->Cout > 64 ? 128 : 64);
    g.Mpad = round_up(d->Cout, g.bm);
    g.ty0 = w.ty0; g.tx0 = w.tx0; g.nty = w.nty; g.ntx = w.ntx;
    const int64_t T = w.T;
    const int64_t Tpad = (T + 127) / 128 * 128;
    // buffer descriptors address one xi-slice of U / V with 32-bit byte offsets
    if (Tpad * g.Kc * 4 >= (int64_t)1 << 31 || (int64_t)g.Kc * g.Mpad * 4 >= (int64_t)1 << 31)
        return IISEG_ERR_UNSUPPORTED;
    g.T = (int)T;
    g.Tpad = (int)Tpad;
    return IISEG_OK;
}

// IISEG_WINO_INPUT_WIDE (default 1; iiseg_conv_wino_input_wide): 0 = the per-tile / LDS-staged kernels
// with one-dword stores everywhere (same bits: A/B timing, tests); 2 = also for the classes iw_shape leaves out
std::atomic<int> g_input_wide{-1};

int input_wide_setting() {
    int v = g_input_wide.load();
    if (v < 0) {
        v = getenv("IISEG_WINO_INPUT_WIDE") ? (atoi(getenv("IISEG_WINO_INPUT_WIDE")) != 0) : 1;
        g_input_wide.store(v);
    }
    return v;
}

// IISEG_WINO_INPUT_NARROW (default 1; iiseg_conv_wino_input_narrow): 1 = the streaming kernel with two tiles per
// thread (TPT = 2: half the registers and LDS, 8-byte stores; same bits) wherever the streaming kernel runs and the
// halved staging buffer holds every workgroup's rows; 0 = four tiles per thread everywhere
std::atomic<int> g_input_narrow{-1};

int input_narrow_setting() {
    int v = g_input_narrow.load();
    if (v < 0) {
        v = getenv("IISEG_WINO_INPUT_NARROW") ? (atoi(getenv("IISEG_WINO_INPUT_NARROW")) != 0) : 1;
        g_input_narrow.store(v);
    }
    return v;
}

// IISEG_WINO_M_QUAD (default 1; iiseg_conv_wino_m_quad): 0 = the products stay M[slice][Mpad][Tpad] with
// one-dword stores and loads on both sides (same bits: A/B timing, tests)
std::atomic<int> g_m_quad{-1};

int m_quad_setting() {
    int v = g_m_quad.load();
    if (v < 0) {
        v = getenv("IISEG_WINO_M_QUAD") ? (atoi(getenv("IISEG_WINO_M_QUAD")) != 0) : 1;
        g_m_quad.store(v);
    }
    return v;
}

// IISEG_WINO_GEMM_SLIM (default 1; iiseg_conv_wino_gemm_slim): 0 = the 256x128 and 128x128 GEMM tiles (Winograd layers
// and the split-K GEMM) keep their addressing in vector registers (114 of them, 120 allocated: four waves per SIMD fill the file
// but for 32); 1 = the SLIM form of wino_gemm_kernel (84, 88 allocated: 160 left).  Same loads, MFMAs, stores and bits.
std::atomic<int> g_gemm_slim{-1};

int gemm_slim_setting() {
    int v = g_gemm_slim.load();
    if (v < 0) {
        v = getenv("IISEG_WINO_GEMM_SLIM") ? (atoi(getenv("IISEG_WINO_GEMM_SLIM")) != 0) : 1;
        g_gemm_slim.store(v);
    }
    return v;
}

// The layout of a GEMM's products, for its producer and its consumer alike: channel quads,
// M[slice][Mpad / 4][Tpad][4], when the setting allows and one slice fits the 32-bit byte offsets of
// the producers' buffer descriptor (Mpad is a multiple of 64 everywhere: quads are whole).
int m_quad(int Mpad, int Tpad) {
    return m_quad_setting() && Mpad % 4 == 0 && (int64_t)Mpad * Tpad * 4 < (int64_t)1 << 31 ? 1 : 0;
}

// every workgroup's staged rows fit its LDS buffer (exact: the same iw_chunk the kernel runs)
bool iw_fits(const WinoParams& p, int nt, int tpt) {
    const int NC = 2 * p.ntx + 2;
    for (int t0 = 0; t0 < p.T; t0 += tpt * nt) {
        const int t1 = t0 + tpt * nt < p.T ? t0 + tpt * nt : p.T;
        if ((int64_t)iw_chunk(t0, t1, p.ntx, p.nty).NR * NC > (int64_t)(IW_E * tpt / 4) * nt) return false;
    }
    return true;
}

int ilds_nt(const WinoParams& p);
constexpr int IW_NT = 256;   // threads per workgroup of the streaming kernel

// Channels per workgroup of the streaming kernel for this call, 0 = it does not apply.  It takes
// plain and mask-byte inputs (`mb`; the pre / pooled form of DePool2D keeps the kernels above)
// whose planes and image strides fit its packed 32-bit offsets.  Two classes measured no gain at
// batch 64 and keep their kernels unless the setting is 2 (profiles/r09_wino_input_ab.txt):
//  - launches of fewer than 4096 tiles, too few quads to fill the chip (2048 channels of 5 x 5
//    tiles, T = 1600: 0.045 -> 0.064 ms; 1024 of 7 x 7, T = 3136: 0.048 -> 0.057 ms; from T = 5184 up
//    it gains);
//  - plain maps whose tiles per image fill the LDS-staged kernel's workgroups exactly: that kernel
//    then already stores at this one's rate (256 channels of 32 x 32 tiles: 0.287 -> 0.299 ms).
// `tpt`: tiles per thread of the launch, 2 under wino_input_narrow where the halved staging still fits.
int iw_shape(const WinoParams& p, bool unpool, bool mb, int* tpt) {
    const int setting = input_wide_setting();
    if (!setting || (unpool && !mb)) return 0;
    if (setting != 2) {
        if (p.T < 4096) return 0;
        const int lnt = mb ? 0 : ilds_nt(p);
        if (lnt && (p.nty * p.ntx) % lnt == 0) return 0;
    }
    const int64_t HW = (int64_t)p.H * p.W, cmax = p.C1 > p.C2 ? p.C1 : p.C2;
    if (HW > (1 << IW_PBITS) || (int64_t)p.B * cmax * HW >= (int64_t)1 << 30) return 0;
    // channels per workgroup: as many as still leave about 8 waves for each of the 256 CUs
    const int64_t waves1 = ((int64_t)p.T + 255) / 256 * p.Kc;   // with one channel per workgroup
    int ch = 8;
    if (p.Kc % 32 == 0 && waves1 / 32 >= 2048) ch = 32;
    else if (waves1 / 16 >= 2048) ch = 16;
    *tpt = input_narrow_setting() && iw_fits(p, IW_NT, 2) ? 2 : 4;
    return *tpt == 2 || iw_fits(p, IW_NT, 4) ? ch : 0;
}

// tiles per workgroup of the LDS-staged kernel (one image per workgroup), 0 = the per-tile kernel
int ilds_nt(const WinoParams& p) {
    static const int lds = getenv("IISEG_WINO_INPUT_LDS") ? atoi(getenv("IISEG_WINO_INPUT_LDS")) : 1;
    const int ntt = p.nty * p.ntx;
    // tiles per workgroup (one image per workgroup): the size that leaves the fewest idle lanes
    int nt = 0;
    double best = 0.0;
    for (int cand = 256; cand >= 128; cand >>= 1) {
        // rows of the tile grid a chunk can span, and the staged region they need
        const int span = (cand - 1 + p.ntx - 1) / p.ntx + 1;
        const int rows = span < p.nty ? span : p.nty;
        if ((2 * rows + 2) * (2 * p.ntx + 2) > ILDS_E * cand) continue;
        const double util = (double)ntt / (((ntt + cand - 1) / cand) * cand);
        if (util > best + 0.02) { best = util; nt = cand; }
    }
    return lds && nt && best >= 0.8 && p.Kc % ILDS_CH == 0 ? nt : 0;
}

void launch_wino_input(hipStream_t s, const WinoParams& p, bool unpool) {
    const bool mb = unpool && p.mask_in;
    int tpt = 4;
    if (const int chw = iw_shape(p, unpool, mb, &tpt)) {
        const dim3 g2((p.T + tpt * IW_NT - 1) / (tpt * IW_NT), p.Kc / chw);
        if (mb && tpt == 2) IISEG_LAUNCH((wino_input_wide_kernel<true, IW_NT, 2>), g2, dim3(IW_NT), 0, s, p, chw);
        else if (mb) IISEG_LAUNCH((wino_input_wide_kernel<true, IW_NT>), g2, dim3(IW_NT), 0, s, p, chw);
        else if (tpt == 2) IISEG_LAUNCH((wino_input_wide_kernel<false, IW_NT, 2>), g2, dim3(IW_NT), 0, s, p, chw);
        else IISEG_LAUNCH((wino_input_wide_kernel<false, IW_NT>), g2, dim3(IW_NT), 0, s, p, chw);
        return;
    }
    const int nt = ilds_nt(p);
    const int ntt = p.nty * p.ntx;
    if (nt) {
        const int chunks = (ntt + nt - 1) / nt;
        const dim3 g2(p.B * chunks, p.Kc / ILDS_CH);
#define WINO_ILDS(U, N, ...) IISEG_LAUNCH((wino_input_lds_kernel<U, N, ##__VA_ARGS__>), g2, dim3(N), 0, s, p, chunks)
        if (mb) { if (nt == 256) WINO_ILDS(true, 256, true); else if (nt == 128) WINO_ILDS(true, 128, true); else WINO_ILDS(true, 64, true); }
        else if (unpool) { if (nt == 256) WINO_ILDS(true, 256); else if (nt == 128) WINO_ILDS(true, 128); else WINO_ILDS(true, 64); }
        else { if (nt == 256) WINO_ILDS(false, 256); else if (nt == 128) WINO_ILDS(false, 128); else WINO_ILDS(false, 64); }
#undef WINO_ILDS
        return;
    }
    const int nc = unpool ? ICH / 2 : ICH;   // channels per thread
    const dim3 grid((p.T + 255) / 256, (p.Kc + nc - 1) / nc), block(256);
    if (!unpool) {
        IISEG_LAUNCH((wino_input_kernel<false, 0, 0>), grid, block, 0, s, p);
        return;
    }
    const int py = (p.ty0 - p.pad) & 1, px = (p.tx0 - p.pad) & 1;  // patch-origin parity
    if (mb) {
        if (py && px) IISEG_LAUNCH((wino_input_kernel<true, 1, 1, true>), grid, block, 0, s, p);
        else if (py) IISEG_LAUNCH((wino_input_kernel<true, 1, 0, true>), grid, block, 0, s, p);
        else if (px) IISEG_LAUNCH((wino_input_kernel<true, 0, 1, true>), grid, block, 0, s, p);
        else IISEG_LAUNCH((wino_input_kernel<true, 0, 0, true>), grid, block, 0, s, p);
        return;
    }
    if (py && px) IISEG_LAUNCH((wino_input_kernel<true, 1, 1>), grid, block, 0, s, p);
    else if (py) IISEG_LAUNCH((wino_input_kernel<true, 1, 0>), grid, block, 0, s, p);
    else if (px) IISEG_LAUNCH((wino_input_kernel<true, 0, 1>), grid, block, 0, s, p);
    else IISEG_LAUNCH((wino_input_kernel<true, 0, 0>), grid, block, 0, s, p);
}

}  // namespace

// Output transform + epilogue for the 16 slices of products that another GEMM kernel wrote in the layout
// m_quad(Mpad, Tpad) gives (the bf16-operand path of conv_wino_bf16.hip): same kernel, tile geometry
// recomputed from `d`.
int iiseg_wino_output_launch(hipStream_t s, const iiseg_conv_desc* d, const float* M, int Mpad,
                             int Tpad, const float* bias, const float* add, float* out) {
    WinoParams p = {};
    p.M = const_cast<float*>(M);
    p.bias = bias; p.add = add; p.out = out;
    p.B = d->B; p.Cout = d->Cout; p.pad = d->pad;
    p.oy0 = d->oy0; p.ox0 = d->ox0; p.OH = d->OH; p.OW = d->OW;
    WinoTiles w;
    const int st = wino_tiles(d, w, 1);
    if (st) return st;
    p.ty0 = w.ty0; p.tx0 = w.tx0; p.nty = w.nty; p.ntx = w.ntx;
    p.T = (int)w.T;
    p.Tpad = Tpad; p.Mpad = Mpad;
    p.AH = d->AH; p.AW = d->AW; p.ay0 = d->ay0; p.ax0 = d->ax0;
    p.relu = (d->flags & IISEG_CONV_RELU) ? 1 : 0;
    if (wino_out_place(d, p)) return IISEG_ERR_SHAPE;
    p.mq = m_quad(Mpad, Tpad);
    const dim3 og((p.T + 255) / 256, (d->Cout + OCH - 1) / OCH);
    if (p.mq) IISEG_LAUNCH(wino_output_kernel<true>, og, dim3(256), 0, s, p);
    else IISEG_LAUNCH(wino_output_kernel<false>, og, dim3(256), 0, s, p);
    return iiseg_check_launch();
}

// the layout launch_gemm_bf16 (conv_wino_bf16.hip) writes for the two consumers in this file
int iiseg_wino_m_quad_layout(int Mpad, int Tpad) { return m_quad(Mpad, Tpad); }

extern "C" int iiseg_conv_wino_supported(const iiseg_conv_desc* d) {
    WinoGeom g;
    return wino_geom(d, g) == IISEG_OK ? 1 : 0;
}

extern "C" int iiseg_conv_wino_input_wide(int on) {
    if (on >= 0) g_input_wide.store(on > 1 ? 2 : on);
    return input_wide_setting();
}

extern "C" int iiseg_conv_wino_input_narrow(int on) {
    if (on >= 0) g_input_narrow.store(on ? 1 : 0);
    return input_narrow_setting();
}

extern "C" int iiseg_conv_wino_gemm_slim(int on) {
    if (on >= 0) g_gemm_slim.store(on ? 1 : 0);
    return gemm_slim_setting();
}

extern "C" int iiseg_conv_wino_m_quad(int on) {
    if (on >= 0) g_m_quad.store(on ? 1 : 0);
    return m_quad_setting();
}

// path as iiseg_conv_wino_input_path returns it; *tpt: tiles per thread where it is the streaming kernel
static int wino_input_path(const iiseg_conv_desc* d, int mask_bytes, int* tpt) {
    WinoGeom g;
    const int st = wino_geom(d, g);
    if (st) return st;
    WinoParams p = {};
    const bool unpool = (d->flags & IISEG_CONV_UNPOOL) != 0;
    if (mask_bytes && !unpool) return IISEG_ERR_UNSUPPORTED;
    p.B = d->B; p.C1 = d->C1; p.C2 = d->C2; p.H = d->H; p.W = d->W;
    p.nty = g.nty; p.ntx = g.ntx; p.T = g.T; p.Tpad = g.Tpad; p.Kc = g.Kc;
    if (iw_shape(p, unpool, mask_bytes != 0, tpt)) return 2;
    *tpt = 0;
    return ilds_nt(p) ? 1 : 0;
}

extern "C" int iiseg_conv_wino_input_path(const iiseg_conv_desc* d, int mask_bytes) {
    int tpt;
    return wino_input_path(d, mask_bytes, &tpt);
}

extern "C" int iiseg_conv_wino_input_tiles(const iiseg_conv_desc* d, int mask_bytes) {
    int tpt = 0;
    const int path = wino_input_path(d, mask_bytes, &tpt);
    return path < 0 ? path : tpt;
}

extern "C" int64_t iiseg_conv_wino_weight_elems(const iiseg_conv_desc* d) {
    WinoGeom g;
    if (wino_geom(d, g) != IISEG_OK) return 0;
    return (int64_t)16 * g.Kc * g.Mpad;
}

extern "C" int64_t iiseg_conv_wino_workspace_elems(const iiseg_conv_desc* d) {
    WinoGeom g;
    if (wino_geom(d, g) != IISEG_OK) return 0;
    return (int64_t)16 * g.Tpad * ((int64_t)g.Kc + g.Mpad);
}

extern "C" int iiseg_conv_wino_pack_f32(void* stream, const iiseg_conv_desc* d, const float* w,
                                        int64_t stride_o, int64_t stride_c, float* U) {
    WinoGeom g;
    const int st = wino_geom(d, g);
    if (st) return st;
    if (!w || !U) return IISEG_ERR_NULL;
    const int64_t n = (int64_t)g.Kc * g.Mpad;
    const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    IISEG_LAUNCH(wino_weight_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, w,
                       stride_o, stride_c, U, d->C1 + d->C2, d->Cout, g.Kc, g.Mpad);
    return iiseg_check_launch();
}

// the fused pool needs a tile to BE a pooling window: even tile anchor, even window origin, and an
// even extent unless the window ends at the map's last (unpaired) row / column
static bool wino_pool_ok(const iiseg_conv_desc* d) {
    WinoGeom g;
    if (wino_geom(d, g) != IISEG_OK) return false;
    const int fullH = d->H + 2 * d->pad - 2, fullW = d->W + 2 * d->pad - 2;
    if ((d->tile_y0 | d->tile_x0 | d->oy0 | d->ox0) & 1) return false;
    if ((d->OH & 1) && d->oy0 + d->OH != fullH) return false;
    if ((d->OW & 1) && d->ox0 + d->OW != fullW) return false;
    return true;
}

extern "C" int iiseg_conv_wino_pool_supported(const iiseg_conv_desc* d) {
    return wino_pool_ok(d) ? 1 : 0;
}

static int wino_run(void* stream, const iiseg_conv_desc* d, const float* x1, const float* x2,
                    const float* pre, const float* pooled, const uint8_t* mask_in, const float* U,
                    const float* bias, const float* add, float* workspace, float* out,
                    float* pool_out, uint8_t* mask_out, uint32_t stages) {
    WinoGeom g;
    const int st = wino_geom(d, g);
    if (st) return st;
    if (!x1 || !U || !workspace || !(out || pool_out)) return IISEG_ERR_NULL;
    if (d->C2 > 0 && !x2) return IISEG_ERR_NULL;
    const bool unpool = (d->flags & IISEG_CONV_UNPOOL) != 0;
    if (mask_in && !unpool) return IISEG_ERR_UNSUPPORTED;
    if (unpool && !mask_in && (!pre || !pooled)) return IISEG_ERR_NULL;
    if (mask_out && !pool_out) return IISEG_ERR_UNSUPPORTED;
    if (pool_out && !wino_pool_ok(d)) return IISEG_ERR_UNSUPPORTED;
    if (((uintptr_t)U & 15) || ((uintptr_t)workspace & 15)) return IISEG_ERR_ALIGN;
    WinoParams p = {};
    p.x1 = x1;
    p.x2 = x2;
    p.pre = mask_in ? nullptr : pre;
    p.pooled = mask_in ? nullptr : pooled;
    p.mask_in = mask_in;
    p.pool = pool_out;
    p.mask_out = mask_out;
    p.pool_H = (d->H + 2 * d->pad - 2) / 2;
    p.pool_W = (d->W + 2 * d->pad - 2) / 2;
    p.h2 = d->H / 2;
    p.w2 = d->W / 2;
    p.U = U;
    p.bias = bias;
    p.add = add;
    p.V = workspace;
    p.M = workspace + (size_t)16 * g.Kc * g.Tpad;
    p.out = out;
    p.B = d->B; p.C1 = d->C1; p.C2 = d->C2; p.H = d->H; p.W = d->W;
    p.Cout = d->Cout; p.pad = d->pad;
    p.oy0 = d->oy0; p.ox0 = d->ox0; p.OH = d->OH; p.OW = d->OW;
    p.ty0 = g.ty0; p.tx0 = g.tx0; p.nty = g.nty; p.ntx = g.ntx;
    p.T = g.T; p.Tpad = g.Tpad; p.Kc = g.Kc; p.Mpad = g.Mpad;
    p.AH = d->AH; p.AW = d->AW; p.ay0 = d->ay0; p.ax0 = d->ax0;
    if (add && (d->ay0 < 0 || d->ax0 < 0 || d->ay0 + d->OH > d->AH || d->ax0 + d->OW > d->AW))
        return IISEG_ERR_SHAPE;
    p.relu = (d->flags & IISEG_CONV_RELU) ? 1 : 0;
    if (wino_out_place(d, p)) return IISEG_ERR_SHAPE;
    p.n_ttiles = g.Tpad / 128;
    p.n_mtiles = g.Mpad / g.bm;
    p.mq = m_quad(g.Mpad, g.Tpad);
    hipStream_t s = (hipStream_t)stream;
    const int tb = (g.T + 255) / 256;
    if (stages & IISEG_WINO_FUSED) {
        if (g.Kc % 32) return IISEG_ERR_UNSUPPORTED;  // the fused kernel's k-tile is 32 channels
        // input transform, then GEMMs + output transform in one kernel (M stays in registers)
        if (stages & IISEG_WINO_INPUT)
            launch_wino_input(s, p, unpool);
        if (stages & IISEG_WINO_GEMM) {
            if (g.bm == 64) {   // narrow layers (Cout <= 64): 64-channel tiles, 4 waves of 64 x 32
                p.n_mtiles = g.Mpad / 64;
                IISEG_LAUNCH((wino_fused_kernel<64, 128, 1, 4, 32, 2>),
                                   dim3(p.n_ttiles * p.n_mtiles), dim3(256), 0, s, p);
                return iiseg_check_launch();
            }
            p.n_mtiles = g.Mpad / 128;
            // short K loops (<= 128 channels): two independent 4-wave workgroups per CU hide the
            // per-xi fold better than one 8-wave workgroup (scripts/bench_wino.py)
            // ... and, for any K, when the 8-wave kernel's few long workgroups would leave CUs idle
            // in the last round (work per CU is quantised in whole workgroups)
            const int w0 = p.n_ttiles * p.n_mtiles, w2 = (g.Tpad / 64) * p.n_mtiles;
            const double cost0 = (w0 + 255) / 256, cost2 = 0.5 * 1.03 * ((w2 + 255) / 256);
            // IISEG_WINO_FUSED_BK=64: 64-channel stages (same bits); measured slower (conv2_2 1.38 ->
            // 1.71 ms: one workgroup per CU instead of two), 32 stays the default
            static const int bk64 = getenv("IISEG_WINO_FUSED_BK") ? atoi(getenv("IISEG_WINO_FUSED_BK")) == 64 : 0;
            const bool big = bk64 && g.Kc % 64 == 0;
            if (g.Kc <= 128 || cost2 < cost0) {
                p.n_ttiles = g.Tpad / 64;
                if (big)
                    IISEG_LAUNCH((wino_fused_kernel<128, 64, 2, 2, 64, 2>),
                                       dim3(p.n_ttiles * p.n_mtiles), dim3(256), 0, s, p);
                else
                IISEG_LAUNCH((wino_fused_kernel<128, 64, 2, 2, 32, 2>),
                                   dim3(p.n_ttiles * p.n_mtiles), dim3(256), 0, s, p);
            } else if (big)
                IISEG_LAUNCH((wino_fused_kernel<128, 128, 2, 4, 64, 2>),
                                   dim3(p.n_ttiles * p.n_mtiles), dim3(512), 0, s, p);
            else
            IISEG_LAUNCH((wino_fused_kernel<128, 128, 2, 4, 32, 2>),
                               dim3(p.n_ttiles * p.n_mtiles), dim3(512), 0, s, p);
        }
        return iiseg_check_launch();
    }
    if (stages & IISEG_WINO_INPUT)
        launch_wino_input(s, p, unpool);
    const int grid = 16 * p.n_ttiles * p.n_mtiles;
    if (stages & IISEG_WINO_GEMM) {
        static const int nbuf = getenv("IISEG_WINO_NBUF") ? atoi(getenv("IISEG_WINO_NBUF")) : 2;
        int bm = g.bm;
        if (bm == 64) {
            IISEG_LAUNCH((wino_gemm_kernel<64, 128, 1, 4, 2>), dim3(grid), dim3(256), 0, s, p);
            bm = 0;
        }
        if (bm == 256) {
            // few, long 256x128 workgroups quantise badly over 256 CUs: fall back to 128x128
            // tiles (about 6 % less MFMA-efficient) when that fills the last round better
            // IISEG_WINO_GEMM_KEEP256=1: never fall back (A/B of this rule with two batches in flight,
            // where the other engine's kernels fill a launch's last round; same k order, same bits)
            static const int keep256 = getenv("IISEG_WINO_GEMM_KEEP256") ? atoi(getenv("IISEG_WINO_GEMM_KEEP256")) : 0;
            const int w256 = grid, w128 = 2 * grid;
            if (!keep256 && 0.5 * 1.06 * ((w128 + 255) / 256) < (double)((w256 + 255) / 256)) bm = 128;
        }
        const int grid2 = bm ? 16 * p.n_ttiles * (g.Mpad / bm) : 0;
        if (bm) p.n_mtiles = g.Mpad / bm;
        // IISEG_WINO_GEMM_BK=32: 32-channel k-tiles (same k order, same bits).  Tried because the bf16
        // kernels are paced per LDS-DMA stage; the fp32 GEMM is not -- measured 2.5 %
        // SLOWER (conv6_1 1.133 -> 1.198 ms, A/B on one device), so 16 stays the default.
        static const int bk32 = getenv("IISEG_WINO_GEMM_BK") ? atoi(getenv("IISEG_WINO_GEMM_BK")) == 32 : 0;
        if (bm && bk32 && g.Kc % 32 == 0 && nbuf != 3) {
            if (bm == 256)
                IISEG_LAUNCH((wino_gemm_kernel<256, 128, 4, 2, 2, 32>), dim3(grid), dim3(512), 0, s, p);
            else
                IISEG_LAUNCH((wino_gemm_kernel<128, 128, 2, 2, 2, 32>), dim3(grid2), dim3(256), 0, s, p);
        } else
        if (bm == 0) {
        } else if (bm == 256 && nbuf == 3)
            IISEG_LAUNCH((wino_gemm_kernel<256, 128, 4, 2, 3>), dim3(grid), dim3(512), 0, s, p);
        else if (bm == 256 && gemm_slim_setting())
            IISEG_LAUNCH((wino_gemm_kernel<256, 128, 4, 2, 2, 16, true>), dim3(grid), dim3(512), 0, s, p);
        else if (bm == 256)
            IISEG_LAUNCH((wino_gemm_kernel<256, 128, 4, 2, 2>), dim3(grid), dim3(512), 0, s, p);
        else if (nbuf == 3)
            IISEG_LAUNCH((wino_gemm_kernel<128, 128, 2, 2, 3>), dim3(grid2), dim3(256), 0, s, p);
        else if (gemm_slim_setting())
            IISEG_LAUNCH((wino_gemm_kernel<128, 128, 2, 2, 2, 16, true>), dim3(grid2), dim3(256), 0, s, p);
        else
            IISEG_LAUNCH((wino_gemm_kernel<128, 128, 2, 2, 2>), dim3(grid2), dim3(256), 0, s, p);
    }
    if (stages & IISEG_WINO_OUTPUT) {
        const dim3 og(tb, (d->Cout + OCH - 1) / OCH);
        if (p.mq) IISEG_LAUNCH(wino_output_kernel<true>, og, dim3(256), 0, s, p);
        else IISEG_LAUNCH(wino_output_kernel<false>, og, dim3(256), 0, s, p);
    }
    return iiseg_check_launch();
}

extern "C" int iiseg_conv_wino_f32(void* stream, const iiseg_conv_desc* d, const float* x1,
                                   const float* x2, const float* pre, const float* pooled,
                                   const float* U, const float* bias,
                                   const float* add, float* workspace, float* out,
                                   uint32_t stages) {
    return wino_run(stream, d, x1, x2, pre, pooled, nullptr, U, bias, add, workspace, out, nullptr,
                    nullptr, stages);
}

extern "C" int iiseg_conv_wino_mask_f32(void* stream, const iiseg_conv_desc* d, const float* x1,
                                        const float* x2, const float* pre, const float* pooled,
                                        const uint8_t* mask_in, const float* U, const float* bias,
                                        const float* add, float* workspace, float* out,
                                        float* pool_out, uint8_t* mask_out, uint32_t stages) {
    return wino_run(stream, d, x1, x2, pre, pooled, mask_in, U, bias, add, workspace, out, pool_out,
                    mask_out, stages);
}

// ================================================================================================
// im2col + split-K GEMM for 'valid' KxK convolutions with a small output map (FCN-8's fc6: 7x7 over
// 13x13 -> 7x7, K = 25088): the table-driven gather of conv_igemm.hip tops out at 78 TFLOP/s there,
// the gather-free GEMM kernel above runs at 125-134.  The S split-K slices ride on the kernel's
// batch index (slice s = rows [s*Kc, (s+1)*Kc) of Wp and of the im2col matrix, contiguous in both),
// so that S * tiles fills the 256 CUs evenly; the output kernel sums the S partial products in a
// fixed order, adds bias, applies ReLU and writes NCHW.
// ================================================================================================
namespace {

struct GemmConvGeom {
    int K, Kpad, Mpad, bm, T, Tpad, S, Kc;
};

__global__ __launch_bounds__(256) void gemm_im2col_kernel(const float* __restrict__ x,
                                                          float* __restrict__ V, int B, int C, int H,
                                                          int W, int KH, int KW, int OH, int OW, int K,
                                                          int Kpad, int T, int Tpad) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int OHW = OH * OW;
    const int b = t / OHW, r = t - b * OHW;
    const int oy = r / OW, ox = r - oy * OW;
    const int KK = KH * KW;
    const float* xb = x + (size_t)b * C * H * W + (size_t)oy * W + ox;
    for (int k = blockIdx.y; k < Kpad; k += gridDim.y) {
        float v = 0.f;
        if (k < K) {
            const int c = k / KK, tap = k - c * KK;
            const int ky = tap / KW, kx = tap - ky * KW;
            v = xb[(size_t)c * H * W + ky * W + kx];
        }
        V[(size_t)k * Tpad + t] = v;
    }
}

// QUAD: M[s][Mpad / 4][Tpad][4], a thread sums one channel quad (a quad that straddles Cout is read
// whole: rows up to Mpad exist); each channel's sum runs over the slices in the same fixed order
template <bool QUAD>
__global__ __launch_bounds__(256) void gemm_output_kernel(const float* __restrict__ M,
                                                          const float* __restrict__ bias,
                                                          float* __restrict__ out, int Cout, int OHW,
                                                          int T, int Tpad, int Mpad, int S, int relu) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int b = t / OHW, px = t - b * OHW;
    const size_t ss = (size_t)Mpad * Tpad;
    if constexpr (QUAD) {
        for (int q = blockIdx.y; 4 * q < Cout; q += gridDim.y) {
            const float* m = M + ((size_t)q * Tpad + t) * 4;
            f32x4 v = *reinterpret_cast<const f32x4*>(m);
            for (int s = 1; s < S; ++s) v += *reinterpret_cast<const f32x4*>(m + (size_t)s * ss);
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
                const int co = 4 * q + cc;
                if (co >= Cout) break;
                float w = v[cc];
                if (bias) w += bias[co];
                if (relu) w = fmaxf(w, 0.f);
                out[((size_t)b * Cout + co) * OHW + px] = w;
            }
        }
        return;
    }
    for (int co = blockIdx.y; co < Cout; co += gridDim.y) {
        const float* m = M + (size_t)co * Tpad + t;
        float v = m[0];
        for (int s = 1; s < S; ++s) v += m[(size_t)s * ss];   // fixed order: deterministic
        if (bias) v += bias[co];
        if (relu) v = fmaxf(v, 0.f);
        out[((size_t)b * Cout + co) * OHW + px] = v;
    }
}

int gemm_conv_geom(const iiseg_conv_desc* d, GemmConvGeom& g) {
    if (!d) return IISEG_ERR_NULL;
    if (d->pad != 0 || d->dil != 1 || d->C2 != 0 ||
        (d->flags & (IISEG_CONV_UNPOOL | IISEG_CONV_TRANSPOSED2)))
        return IISEG_ERR_UNSUPPORTED;
    const int fullH = d->H - d->KH + 1, fullW = d->W - d->KW + 1;
    if (fullH <= 0 || fullW <= 0) return IISEG_ERR_SHAPE;
    // full, dense output only
    if (d->oy0 != 0 || d->ox0 != 0 || d->OH != fullH || d->OW != fullW || d->out_ctot != 0 ||
        d->out_H != 0)
        return IISEG_ERR_UNSUPPORTED;
    g.K = d->C1 * d->KH * d->KW;
    g.Kpad = d->Kpad;
    g.Mpad = d->Mpad;
    if (g.Kpad < g.K || g.Kpad % 16 || g.Mpad % 128 || g.Mpad < d->Cout) return IISEG_ERR_UNSUPPORTED;
    g.bm = g.Mpad % 256 == 0 ? 256 : 128;
    const int64_t T = (int64_t)d->B * fullH * fullW;
    const int64_t Tpad = (T + 127) / 128 * 128;
    if (Tpad * g.Kpad * 4 >= (int64_t)1 << 31 || (int64_t)g.Kpad * g.Mpad * 4 >= (int64_t)1 << 31)
        return IISEG_ERR_UNSUPPORTED;
    g.T = (int)T;
    g.Tpad = (int)Tpad;
    // split-K: the divisor S of Kpad/16 (<= 16) minimising  GEMM time (rounds of 256 CUs at the
    // measured 131 TFLOP/s) + the traffic of writing and re-reading the S partial products (5 TB/s).
    // S fixes the association of the K sum, so it must NOT depend on the batch: it is chosen for a
    // nominal 3200 output pixels (64 images x 7x7, the fc6 / fc7 case) whatever the real T is,
    // which keeps an image's result independent of the images it is batched with.
    const int tiles = 25 * (g.Mpad / g.bm), units = g.Kpad / 16;
    const double tile_s = 2.0 * g.Kpad * g.bm * 128 / (131e12 / 256);
    const double red_s = 8.0 * g.Mpad * 3200 / 5e12;
    double best = 1e30;
    g.S = 1;
    for (int S = 1; S <= 16; ++S) {
        if (units % S || units / S < 8) continue;
        const double cost = (double)((S * tiles + 255) / 256) / S * tile_s + S * red_s;
        if (cost < best) { best = cost; g.S = S; }
    }
    g.Kc = g.Kpad / g.S;
    return IISEG_OK;
}

void launch_gemm_output(hipStream_t s, const float* M, const float* bias, float* out, int Cout, int OHW,
                        int T, int Tpad, int Mpad, int S, int relu) {
    const int tb = (T + 255) / 256;
    if (m_quad(Mpad, Tpad)) {
        const int nq = (Cout + 3) / 4;
        IISEG_LAUNCH(gemm_output_kernel<true>, dim3(tb, nq < 1024 ? nq : 1024), dim3(256), 0, s, M, bias,
                           out, Cout, OHW, T, Tpad, Mpad, S, relu);
    } else {
        IISEG_LAUNCH(gemm_output_kernel<false>, dim3(tb, Cout < 1024 ? Cout : 1024), dim3(256), 0, s, M,
                           bias, out, Cout, OHW, T, Tpad, Mpad, S, relu);
    }
}

}  // namespace

// bias + ReLU + NCHW store of a GEMM result (S = 1; the layout m_quad gives) for the bf16 GEMM path
int iiseg_gemm_output_launch(hipStream_t s, const float* M, const float* bias, float* out, int Cout,
                             int OHW, int T, int Tpad, int Mpad, int relu) {
    launch_gemm_output(s, M, bias, out, Cout, OHW, T, Tpad, Mpad, 1, relu);
    return iiseg_check_launch();
}

extern "C" int iiseg_conv_gemm_supported(const iiseg_conv_desc* d) {
    GemmConvGeom g;
    return gemm_conv_geom(d, g) == IISEG_OK ? 1 : 0;
}

extern "C" int64_t iiseg_conv_gemm_workspace_elems(const iiseg_conv_desc* d) {
    GemmConvGeom g;
    if (gemm_conv_geom(d, g) != IISEG_OK) return 0;
    return (int64_t)g.Tpad * ((int64_t)g.Kpad + (int64_t)g.S * g.Mpad);
}

extern "C" int iiseg_conv_gemm_f32(void* stream, const iiseg_conv_desc* d, const float* x,
                                   const float* wp, const float* bias, float* workspace,
                                   float* out, uint32_t stages) {
    GemmConvGeom g;
    const int st = gemm_conv_geom(d, g);
    if (st) return st;
    if (!x || !wp || !workspace || !out) return IISEG_ERR_NULL;
    if (((uintptr_t)wp & 15) || ((uintptr_t)workspace & 15)) return IISEG_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    float* V = workspace;
    float* M = workspace + (size_t)g.Kpad * g.Tpad;
    const int OH = d->OH, OW = d->OW, tb = (g.T + 255) / 256;
    if (stages & IISEG_WINO_INPUT)
        IISEG_LAUNCH(gemm_im2col_kernel, dim3(tb, g.Kpad < 1024 ? g.Kpad : 1024), dim3(256), 0,
                           s, x, V, d->B, d->C1, d->H, d->W, d->KH, d->KW, OH, OW, g.K, g.Kpad, g.T,
                           g.Tpad);
    WinoParams p = {};
    p.U = wp;
    p.V = V;
    p.M = M;
    p.Kc = g.Kc;
    p.Mpad = g.Mpad;
    p.Tpad = g.Tpad;
    p.T = g.T;
    p.n_ttiles = g.Tpad / 128;
    p.n_mtiles = g.Mpad / g.bm;
    p.mq = m_quad(g.Mpad, g.Tpad);
    const int grid = g.S * p.n_ttiles * p.n_mtiles;
    if (stages & IISEG_WINO_GEMM) {
        if (g.bm == 256 && gemm_slim_setting())
            IISEG_LAUNCH((wino_gemm_kernel<256, 128, 4, 2, 2, 16, true>), dim3(grid), dim3(512), 0, s, p);
        else if (g.bm == 256)
            IISEG_LAUNCH((wino_gemm_kernel<256, 128, 4, 2, 2>), dim3(grid), dim3(512), 0, s, p);
        else if (gemm_slim_setting())
            IISEG_LAUNCH((wino_gemm_kernel<128, 128, 2, 2, 2, 16, true>), dim3(grid), dim3(256), 0, s, p);
        else
            IISEG_LAUNCH((wino_gemm_kernel<128, 128, 2, 2, 2>), dim3(grid), dim3(256), 0, s, p);
    }
    if (stages & IISEG_WINO_OUTPUT)
        launch_gemm_output(s, M, bias, out, d->Cout, OH * OW, g.T, g.Tpad, g.Mpad, g.S,
                           (d->flags & IISEG_CONV_RELU) ? 1 : 0);
    return iiseg_check_launch();
}
