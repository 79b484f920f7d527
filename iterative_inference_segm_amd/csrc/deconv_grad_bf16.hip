// Backward of the K = 3, stride-2 transposed convolution with the products on the 16-bit matrix pipe (deconv='bf16':
// FC-DenseNet's five TransitionUp layers).  Notation of deconv_grad.hip: x (B,Cin,H,W),
// W[Cin][Cout][3][3], `full` is (2H + 1) x (2W + 1), g = dL/d(window (oy0, ox0, OH, OW) of full), gf = g at the
// window's offset inside full and zero elsewhere.  For a, c in {0, 1, 2}:
//
//   dW[ci][co][2-a][2-c] = sum_{b,i,j}  bf16(x[b][ci][i][j])     * bf16(gf[b][co][2i+a][2j+c])
//   gx[b][ci][i][j]      = sum_{co,a,c} bf16(W[ci][co][2-a][2-c]) * bf16(gf[b][co][2i+a][2j+c])
//   db[co]               = sum g                                    (the unrounded fp32 values)
//
// Every operand is fp32 in memory and rounded once, to nearest even, as it is staged into LDS (W from the layer's
// own parameter: there is no packed image); a product of two bf16 values is exact in fp32, and the fp32 sums run in
// an order the descriptor fixes.  No atomics: the same inputs give the same bits.  Every global load is at a
// clamped, always valid address; what lies outside the map, the window or the channel count is replaced by zero
// when it is stored to LDS.
//
// Both kernels work on a tile of TI x TJ = 4 x 16 input pixels and hold the (2 TI + 1) x (2 TJ + 1) piece of gf it
// reaches as four parity planes P[py][px][r][q] = gf[2r + py][2q + px] (py = 0: TI + 1 rows, px = 0: TJ + 1
// columns): tap (a, c) at tile pixel (i, j) reads P[a & 1][c & 1][i + (a >> 1)][j + (c >> 1)], so every tap is a
// unit-stride run and the stride-2 gather happens once, in the LDS address of the staging store.
//
// wgrad (deconv_wgrad_bf16_kernel): conv_wgrad_bf16.hip's co16 scheme.  k = pixels, A = g (rows co), B = x (columns
//   ci), nine accumulators per 16 x 16 channel pair on v_mfma_f32_16x16x32_bf16; the k-group of a lane is 8
//   consecutive j of one tile row, two rows per group pair: two k-steps per tile.  A workgroup owns 32 output x 64
//   input channels and a slab of tiles; wave w of eight multiplies output group w & 1 with input group w >> 1.  LDS,
//   twice: g [32 co][9 plane rows][40] bf16 (px = 0 at 0..16, px = 1 at 24..39; 180-dword channels) and x [64
//   ci][4][16] (36-dword channels): 63 KiB.  A fragment of x or of a px plane is one 16-byte read; the c = 2 taps
//   shift the px = 0 run by one element (v_alignbyte).  All eight waves load tile t + 1 into registers, multiply tile
//   t out of one image, then round and store into the other: one barrier per tile.  Slabs over the tiles of (b, row,
//   column) by split_slabs; one slab writes dW and db themselves, several go to the workspace [slab][nW + Cout] and a
//   finalize launch adds them in slab order in fp32.  db: the workgroups behind the channel blocks, one output channel
//   per wave and the slab's share of the window's pixels -- a sum of this file's own, in its own order.
// dgrad (deconv_dgrad_bf16_kernel): k = (co, tap), A = W (rows ci), B = g (columns: the 16 pixels of a tile row).  A
//   workgroup owns one tile x 64 input channels and walks the output channels in k-tiles of 32.  LDS per k-tile: g as
//   [co chunk of 8][9 plane rows][33 plane columns] 16-byte words (a lane's fragment: 8 co of one pixel) and W as
//   [tap][co chunk][64 ci (+ 1)] words, 55 KiB.  The stager loads 8 channel planes per gf position, coalesced along
//   the row, and packs them into one LDS store; the W tile is read from the fp32 parameter in runs of 288 consecutive
//   floats per input channel (32 co x 9 taps) and turned by its 2-byte LDS stores.  Wave w multiplies tile row w & 3
//   with the two 16-channel groups 2 (w >> 2), + 1.  The loads of k-tile t + 1 are issued before the products of
//   k-tile t and stored after them, between two barriers.  No split over co, no workspace.
#include "mma16_common.h"

namespace {

constexpr int TI = 4, TJ = 16;                           // input pixel tile
constexpr int GH = 2 * TI + 1, GW = 2 * TJ + 1;          // the piece of gf it reaches
constexpr int GPIX = GH * GW;                            // 297
constexpr int GN = (GPIX + 63) / 64;                     // positions lane + 64 n of it
constexpr int NWAVE = 8;

struct db_params {
    int B, Cin, Cout, H, W;
    int oy0, ox0, OH, OW;
    int tilesY, tilesX;
    int ncob, ncib;               // wgrad: channel blocks (output, input); dgrad: ncib only
    int nslab;                    // wgrad
    long long T, tps;             // tiles in all, per slab
    long long pps;                // window pixels (of B OH OW) per slab: db
    long long nW, S;              // Cin Cout 9, nW + Cout
    int nkt;                      // dgrad: k-tiles
};

// ---------------------------------------------------------------- weight gradient
namespace wg {
constexpr int COB = 32, CIB = 64;                        // channel block: output, input
constexpr int NG = COB / NWAVE, NX = CIB / NWAVE;        // channels a wave stages: w, w + 8, ...
constexpr int GROW = 40, PX1 = 24;                       // bf16 per plane row; where its px = 1 half starts
constexpr int GLD = GH * GROW;                           // bf16 per g channel: 180 dwords
constexpr int XLD = TI * TJ + 8;                         // bf16 per x channel: 36 dwords
constexpr int TARGET_WORKGROUPS = 512;                   // two per CU
constexpr int MIN_TILES_PER_SLAB = 4;                    // 256 pixels: below that a split buys a finalize launch only
static_assert(TI * TJ == 64 && TJ + 1 <= PX1 && PX1 + TJ <= GROW && GROW % 8 == 0 && PX1 % 8 == 0 && GLD % 8 == 0 &&
              XLD % 8 == 0, "one x pixel per lane; 16-byte fragment reads");
static_assert(2 * (COB * GLD + CIB * XLD) * 2 <= 65536, "LDS");
}  // namespace wg

__global__ __launch_bounds__(512) void deconv_wgrad_bf16_kernel(db_params p, const float* __restrict__ x,
                                                                const float* __restrict__ g, float* __restrict__ dst,
                                                                float* __restrict__ dbdst) {
    using namespace wg;
    __shared__ __attribute__((aligned(16))) unsigned short gs[2][COB * GLD];
    __shared__ __attribute__((aligned(16))) unsigned short xs[2][CIB * XLD];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int slab = blockIdx.y, nblk = p.ncob * p.ncib;
    const size_t gplane = (size_t)p.OH * p.OW, xplane = (size_t)p.H * p.W;
    float* out = p.nslab == 1 ? dst : dst + (long long)slab * p.S;

    if ((int)blockIdx.x >= nblk) {
        // ---- db: one output channel per wave, this slab's share of the window's pixels ----
        const int co = ((int)blockIdx.x - nblk) * NWAVE + wave;
        if (co >= p.Cout) return;
        const long long NP = (long long)p.B * (long long)gplane;
        const long long q0 = min(NP, (long long)slab * p.pps), q1 = min(NP, q0 + p.pps);
        float s = 0.f;
        for (long long q = q0 + lane; q < q1; q += 64)
            s += g[((q / (long long)gplane) * p.Cout + co) * (long long)gplane + q % (long long)gplane];
        s = wave_sum(s);
        if (lane == 0) (p.nslab == 1 ? dbdst : out + p.nW)[co] = s;
        return;
    }
    const int co0 = ((int)blockIdx.x % p.ncob) * COB, cb0 = ((int)blockIdx.x / p.ncob) * CIB;
    const int nco = min(COB, p.Cout - co0), nci = min(CIB, p.Cin - cb0);
    const int per_img = p.tilesY * p.tilesX;
    const long long t0 = (long long)slab * p.tps, t1 = min(p.T, t0 + p.tps);

    // position lane + 64 n of the gf piece: (row, column) in it, and where it goes in a channel's planes
    int gly[GN], glx[GN], goff[GN];
#pragma unroll
    for (int n = 0; n < GN; ++n) {
        const int k = min(lane + 64 * n, GPIX - 1);
        gly[n] = k / GW;
        glx[n] = k % GW;
        goff[n] = ((gly[n] & 1) * (TI + 1) + (gly[n] >> 1)) * GROW + (glx[n] & 1) * PX1 + (glx[n] >> 1);
    }
    const int xr = lane / TJ, xc = lane % TJ;            // the x pixel of the lane

    // lane -> channel within the wave's 16 and k-group kg = (tile row of the pair, pixel half)
    const int l15 = lane & 15, kg = lane >> 4, rr = kg >> 1, half = kg & 1;
    const int cg = wave & 1, xg = wave >> 1;
    const int ga_off = (16 * cg + l15) * GLD + rr * GROW + 8 * half;
    const int xb_off = (16 * xg + l15) * XLD + rr * TJ + 8 * half;
    const bool wave_on = 16 * cg < nco && 16 * xg < nci;                 // wave-uniform
    f32x4 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[t][r] = 0.f;

    unsigned go[GN], xo;
    bool gin[GN], xin;
    float gv[NG][GN], xv[NX];
    auto load = [&](long long t) __attribute__((always_inline)) {
        const int b = __builtin_amdgcn_readfirstlane((int)(t / per_img));
        const int rem = __builtin_amdgcn_readfirstlane((int)(t % per_img));
        const int ty = __builtin_amdgcn_readfirstlane(rem / p.tilesX);
        const int i0 = ty * TI, j0 = (rem - ty * p.tilesX) * TJ;
        const float* gb = g + ((size_t)b * p.Cout + co0) * gplane;
        const float* xb = x + ((size_t)b * p.Cin + cb0) * xplane;
#pragma unroll
        for (int n = 0; n < GN; ++n) {
            const int wy = 2 * i0 + gly[n] - p.oy0, wx = 2 * j0 + glx[n] - p.ox0;
            gin[n] = wy >= 0 && wy < p.OH && wx >= 0 && wx < p.OW;
            go[n] = (unsigned)(min(max(wy, 0), p.OH - 1) * p.OW + min(max(wx, 0), p.OW - 1));
        }
        xin = i0 + xr < p.H && j0 + xc < p.W;
        xo = (unsigned)(min(i0 + xr, p.H - 1) * p.W + min(j0 + xc, p.W - 1));
#pragma unroll
        for (int m = 0; m < NG; ++m) {
            const float* gc = gb + (size_t)min(NWAVE * m + wave, nco - 1) * gplane;
#pragma unroll
            for (int n = 0; n < GN; ++n) gv[m][n] = gc[go[n]];
        }
#pragma unroll
        for (int m = 0; m < NX; ++m) xv[m] = xb[(size_t)min(NWAVE * m + wave, nci - 1) * xplane + xo];
    };
    auto store = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int m = 0; m < NG; ++m) {
            const int c = NWAVE * m + wave;
#pragma unroll
            for (int n = 0; n < GN; ++n)
                if (lane + 64 * n < GPIX) gs[buf][c * GLD + goff[n]] = to_bf16(gin[n] && c < nco ? gv[m][n] : 0.f);
        }
#pragma unroll
        for (int m = 0; m < NX; ++m) {
            const int c = NWAVE * m + wave;
            xs[buf][c * XLD + lane] = to_bf16(xin && c < nci ? xv[m] : 0.f);
        }
    };
    // The products of one tile out of LDS image `buf`: step s is tile rows 2 s, 2 s + 1.
    auto multiply = [&](int buf) __attribute__((always_inline)) {
        const unsigned short* ga = gs[buf] + ga_off;
        const unsigned short* xb = xs[buf] + xb_off;
#pragma unroll
        for (int s = 0; s < TI / 2; ++s) {
            const bf16x8 b = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(xb + 2 * s * TJ));
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const unsigned short* r = ga + ((a & 1) * (TI + 1) + 2 * s + (a >> 1)) * GROW;
                const u32x4 e = *reinterpret_cast<const u32x4*>(r);
                const unsigned e4 = *reinterpret_cast<const unsigned*>(r + 8);
                const u32x4 o = *reinterpret_cast<const u32x4*>(r + PX1);
                const bf16x8 a0 = __builtin_bit_cast(bf16x8, e), a1 = __builtin_bit_cast(bf16x8, o);
                const bf16x8 a2 = frag_shift1(e.x, e.y, e.z, e.w, e4);
                acc[a * 3 + 0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b, acc[a * 3 + 0], 0, 0, 0);
                acc[a * 3 + 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b, acc[a * 3 + 1], 0, 0, 0);
                acc[a * 3 + 2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, b, acc[a * 3 + 2], 0, 0, 0);
            }
        }
    };

    load(t0);
    store(0);
    __syncthreads();
    int buf = 0;
    for (long long t = t0; t < t1; ++t, buf ^= 1) {
        const bool more = t + 1 < t1;                                    // block-uniform
        if (more) load(t + 1);
        if (wave_on) multiply(buf);
        if (more) store(buf ^ 1);
        __syncthreads();                                                 // image buf is read, image buf ^ 1 written
    }

    // C: row co = 4 kg + r, column ci = l15; tap (a, c) is W's [2 - a][2 - c]
    const int ci = cb0 + 16 * xg + l15;
    if (!wave_on || ci >= p.Cin) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int co = co0 + 16 * cg + 4 * kg + r;
        if (co >= p.Cout) continue;
        float* o = out + ((long long)ci * p.Cout + co) * 9;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c = 0; c < 3; ++c) o[(2 - a) * 3 + (2 - c)] = acc[a * 3 + c][r];
    }
}

__global__ __launch_bounds__(256) void deconv_wgrad_bf16_finalize_kernel(const float* __restrict__ ws, int nslab,
                                                                         long long S, long long nW,
                                                                         float* __restrict__ dW,
                                                                         float* __restrict__ db) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= S || (idx >= nW && !db)) return;
    float v = 0.f;
    for (int k = 0; k < nslab; ++k) v += ws[(long long)k * S + idx];
    if (idx < nW) dW[idx] = v;
    else db[idx - nW] = v;
}

// ---------------------------------------------------------------- data gradient
namespace dg {
constexpr int CB = 64;                                   // input channels of a workgroup
constexpr int CBP = CB + 1;                              // words per [tap][chunk] slice of W: the taps on other banks
constexpr int KT = 32, NCHUNK = KT / 8;                  // output channels of a k-tile, in chunks of 8
constexpr int PCOL = GW, PX1 = TJ + 1;                   // plane columns of a row: px = 0 at 0..16, px = 1 at 17..32
constexpr int GWORDS = GH * PCOL;                        // 16-byte words of a chunk's planes (297)
constexpr int GS_WORDS = NCHUNK * GWORDS, WS_WORDS = 9 * NCHUNK * CBP;
constexpr int GP = (GPIX + 127) / 128;                   // positions a staging lane holds: lane + 64 (2 n + pass0)
constexpr int WRUN = KT * 9;                             // floats of W per input channel and k-tile: [co][tap]
constexpr int WN = (WRUN + 63) / 64;                     // ... a lane loads: lane + 64 n
constexpr int NXW = CB / NWAVE;                          // input channels of W a wave stages: w, w + 8, ...
static_assert((GS_WORDS + WS_WORDS) * 16 <= 65536 && NCHUNK == 4, "LDS; a chunk per k-group");
}  // namespace dg

__global__ __launch_bounds__(512) void deconv_dgrad_bf16_kernel(db_params p, const float* __restrict__ g,
                                                                const float* __restrict__ w, float* __restrict__ gx) {
    using namespace dg;
    __shared__ __attribute__((aligned(16))) u32x4 gs[GS_WORDS];
    __shared__ __attribute__((aligned(16))) unsigned short wsm[WS_WORDS * 8];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cb0 = ((int)blockIdx.x % p.ncib) * CB, tile = (int)blockIdx.x / p.ncib;
    const int per_img = p.tilesY * p.tilesX;
    const int b = tile / per_img, rem = tile % per_img;
    const int i0 = (rem / p.tilesX) * TI, j0 = (rem % p.tilesX) * TJ;
    const size_t gplane = (size_t)p.OH * p.OW;
    const float* gimg = g + (size_t)b * p.Cout * gplane;

    // g: wave -> co chunk wave & 3 at the positions lane + 64 (2 n + (wave >> 2)) of the gf piece
    const int chunk = wave & 3, pass0 = wave >> 2;
    unsigned go[GP];
    int gdst[GP];
    bool gin[GP];
#pragma unroll
    for (int n = 0; n < GP; ++n) {
        const int k = min(lane + 64 * (2 * n + pass0), GPIX - 1), ly = k / GW, lx = k % GW;
        const int wy = 2 * i0 + ly - p.oy0, wx = 2 * j0 + lx - p.ox0;
        gin[n] = wy >= 0 && wy < p.OH && wx >= 0 && wx < p.OW;
        go[n] = (unsigned)(min(max(wy, 0), p.OH - 1) * p.OW + min(max(wx, 0), p.OW - 1));
        gdst[n] = chunk * GWORDS + ((ly & 1) * (TI + 1) + (ly >> 1)) * PCOL + (lx & 1) * PX1 + (lx >> 1);
    }
    // W: float lane + 64 n of an input channel's run [co][ky][kx] is (co = e / 9, tap (a, c) = 8 - e % 9)
    int wdst[WN];
#pragma unroll
    for (int n = 0; n < WN; ++n) {
        const int e = min(lane + 64 * n, WRUN - 1), col = e / 9, tap = 8 - e % 9;
        wdst[n] = ((tap * NCHUNK + (col >> 3)) * CBP) * 8 + (col & 7);
    }

    float gv[GP][8], wv[NXW][WN];
    auto load = [&](int kt) __attribute__((always_inline)) {
        const int c0 = kt * KT + chunk * 8;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float* gc = gimg + (size_t)min(c0 + i, p.Cout - 1) * gplane;
#pragma unroll
            for (int n = 0; n < GP; ++n) gv[n][i] = gc[go[n]];
        }
        const int last = (p.Cout - kt * KT) * 9 - 1;                     // of the run's real floats
#pragma unroll
        for (int m = 0; m < NXW; ++m) {
            const float* wc = w + ((size_t)min(cb0 + NWAVE * m + wave, p.Cin - 1) * p.Cout + (size_t)kt * KT) * 9;
#pragma unroll
            for (int n = 0; n < WN; ++n) wv[m][n] = wc[min(min(lane + 64 * n, WRUN - 1), last)];
        }
    };
    auto store = [&](int kt) __attribute__((always_inline)) {
        const int c0 = kt * KT + chunk * 8;
#pragma unroll
        for (int n = 0; n < GP; ++n) {
            float v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = gin[n] && c0 + i < p.Cout ? gv[n][i] : 0.f;
            u32x4 q;
            q.x = pack2(v[0], v[1]); q.y = pack2(v[2], v[3]); q.z = pack2(v[4], v[5]); q.w = pack2(v[6], v[7]);
            if (lane + 64 * (2 * n + pass0) < GPIX) gs[gdst[n]] = q;
        }
        const int last = (p.Cout - kt * KT) * 9 - 1;
#pragma unroll
        for (int m = 0; m < NXW; ++m) {
            const int c = NWAVE * m + wave;
#pragma unroll
            for (int n = 0; n < WN; ++n) {
                const int e = lane + 64 * n;
                if (e < WRUN) wsm[wdst[n] + c * 8] = to_bf16(e <= last && cb0 + c < p.Cin ? wv[m][n] : 0.f);
            }
        }
    };

    // wave -> tile row pr and the input-channel groups 2 cp, 2 cp + 1; lane -> (pixel / channel l15, co chunk kg)
    const int l15 = lane & 15, kg = lane >> 4, pr = wave & 3, cp = wave >> 2;
    const u32x4* wsw = reinterpret_cast<const u32x4*>(wsm);
    f32x4 acc[2];
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[n][r] = 0.f;
    const bool wave_on = cb0 + 32 * cp < p.Cin;                          // wave-uniform
    auto multiply = [&]() __attribute__((always_inline)) {
        const u32x4* gb = gs + kg * GWORDS + l15;
        const u32x4* wa = wsw + kg * CBP + 32 * cp + l15;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const bf16x8 bb = __builtin_bit_cast(
                    bf16x8, gb[((a & 1) * (TI + 1) + pr + (a >> 1)) * PCOL + (c & 1) * PX1 + (c >> 1)]);
                const bf16x8 a0 = __builtin_bit_cast(bf16x8, wa[(a * 3 + c) * NCHUNK * CBP]);
                const bf16x8 a1 = __builtin_bit_cast(bf16x8, wa[(a * 3 + c) * NCHUNK * CBP + 16]);
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, bb, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, bb, acc[1], 0, 0, 0);
            }
    };

    load(0);
    store(0);
    __syncthreads();
    for (int kt = 0; kt < p.nkt; ++kt) {
        const bool more = kt + 1 < p.nkt;                                // block-uniform
        if (more) load(kt + 1);
        if (wave_on) multiply();
        __syncthreads();                                                 // the image is read
        if (more) store(kt + 1);
        __syncthreads();                                                 // ... and written
    }

    // C: row ci = 4 kg + r of the group, column pixel j = l15 of tile row pr
    const int i = i0 + pr, j = j0 + l15;
    if (!wave_on || i >= p.H || j >= p.W) return;
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ci = cb0 + 16 * (2 * cp + n) + 4 * kg + r;
            if (ci < p.Cin) gx[(((size_t)b * p.Cin + ci) * p.H + i) * p.W + j] = acc[n][r];
        }
}

// ---- host side ----
int db_plan(const iiseg_deconv_desc* d, db_params& p) {
    if (!d) return IISEG_ERR_NULL;
    if (d->B <= 0 || d->Cin <= 0 || d->H <= 0 || d->W <= 0 || d->Cout <= 0 || d->K <= 0 || d->stride <= 0 ||
        d->OH <= 0 || d->OW <= 0 || d->oy0 < 0 || d->ox0 < 0)
        return IISEG_ERR_SHAPE;
    if (d->B > 65535 || d->Cin > 65535 || d->Cout > 65535 || d->K > 1024 || d->stride > 1024 ||
        (int64_t)d->H * d->W > (int64_t)1 << 28)
        return IISEG_ERR_SHAPE;
    const int64_t fullH = (int64_t)(d->H - 1) * d->stride + d->K, fullW = (int64_t)(d->W - 1) * d->stride + d->K;
    if ((int64_t)d->oy0 + d->OH > fullH || (int64_t)d->ox0 + d->OW > fullW) return IISEG_ERR_SHAPE;
    if ((int64_t)d->OH * d->OW > (int64_t)1 << 30) return IISEG_ERR_SHAPE;
    if (d->K != 3 || d->stride != 2) return IISEG_ERR_UNSUPPORTED;
    const int64_t nW = (int64_t)d->Cin * d->Cout * 9;
    if (nW > ((int64_t)1 << 31) - 1) return IISEG_ERR_SHAPE;
    p.B = d->B; p.Cin = d->Cin; p.Cout = d->Cout; p.H = d->H; p.W = d->W;
    p.oy0 = d->oy0; p.ox0 = d->ox0; p.OH = d->OH; p.OW = d->OW;
    p.tilesY = (d->H + TI - 1) / TI;
    p.tilesX = (d->W + TJ - 1) / TJ;
    p.T = (int64_t)d->B * p.tilesY * p.tilesX;
    p.nW = nW; p.S = nW + d->Cout;
    p.ncob = (d->Cout + wg::COB - 1) / wg::COB;
    p.ncib = (d->Cin + wg::CIB - 1) / wg::CIB;               // (dg::CB is the same 64)
    p.nkt = (d->Cout + dg::KT - 1) / dg::KT;
    if (p.T * p.ncib > ((int64_t)1 << 31) - 1) return IISEG_ERR_SHAPE;
    int64_t tps;
    split_slabs(p.T, (int64_t)p.ncob * p.ncib, wg::TARGET_WORKGROUPS, wg::MIN_TILES_PER_SLAB, &tps, &p.nslab);
    p.tps = tps;
    const int64_t NP = (int64_t)d->B * d->OH * d->OW;
    p.pps = (NP + p.nslab - 1) / p.nslab;
    return IISEG_OK;
}
static_assert(wg::CIB == dg::CB, "one count of input-channel blocks");

}  // namespace

extern "C" int iiseg_deconv_grad_bf16_check(const iiseg_deconv_desc* d) {
    db_params p;
    return db_plan(d, p);
}
extern "C" int iiseg_deconv_wgrad_bf16_slabs(const iiseg_deconv_desc* d) {
    db_params p;
    if (int st = db_plan(d, p)) return st;
    return p.nslab;
}
extern "C" int64_t iiseg_deconv_wgrad_bf16_workspace_elems(const iiseg_deconv_desc* d) {
    db_params p;
    if (int st = db_plan(d, p)) return st;
    return p.nslab == 1 ? 0 : (int64_t)p.nslab * p.S;
}
extern "C" int64_t iiseg_deconv_dgrad_bf16_workspace_elems(const iiseg_deconv_desc* d) {
    db_params p;
    if (int st = db_plan(d, p)) return st;
    return 0;                                                            // the reduction over co is not split
}
extern "C" int iiseg_deconv_wgrad_bf16(void* stream, const iiseg_deconv_desc* d, const float* x, const float* g,
                                       float* ws, float* dW, float* db) {
    db_params p;
    if (int st = db_plan(d, p)) return st;
    if (!x || !g || !dW || (p.nslab > 1 && !ws)) return IISEG_ERR_NULL;
    const int64_t xb = (int64_t)d->B * d->Cin * d->H * d->W * 4, gb = (int64_t)d->B * d->Cout * d->OH * d->OW * 4;
    const int64_t wsb = p.nslab > 1 ? p.nslab * p.S * 4 : 0;
    const void* outs[3] = {dW, db, p.nslab > 1 ? ws : nullptr};
    const int64_t outb[3] = {p.nW * 4, (int64_t)d->Cout * 4, wsb};
    for (int k = 0; k < 3; ++k)
        if (outs[k] && (ranges_overlap(outs[k], outb[k], x, xb) || ranges_overlap(outs[k], outb[k], g, gb)))
            return IISEG_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const unsigned nblk = (unsigned)(p.ncob * p.ncib), ndb = db ? (unsigned)((p.Cout + NWAVE - 1) / NWAVE) : 0u;
    IISEG_LAUNCH(deconv_wgrad_bf16_kernel, dim3(nblk + ndb, (unsigned)p.nslab), dim3(512), 0, s, p, x, g,
                 p.nslab == 1 ? dW : ws, db);
    if (p.nslab > 1)
        IISEG_LAUNCH(deconv_wgrad_bf16_finalize_kernel, dim3((unsigned)((p.S + 255) / 256)), dim3(256), 0, s,
                     (const float*)ws, p.nslab, p.S, p.nW, dW, db);
    return iiseg_check_launch();
}
extern "C" int iiseg_deconv_dgrad_bf16(void* stream, const iiseg_deconv_desc* d, const float* g, const float* w,
                                       float* ws, float* gx) {
    (void)ws;
    db_params p;
    if (int st = db_plan(d, p)) return st;
    if (!g || !w || !gx) return IISEG_ERR_NULL;
    const int64_t gxb = (int64_t)d->B * d->Cin * d->H * d->W * 4, gb = (int64_t)d->B * d->Cout * d->OH * d->OW * 4;
    // gx is written while other workgroups still read g and the parameter
    if (ranges_overlap(gx, gxb, g, gb) || ranges_overlap(gx, gxb, w, p.nW * 4)) return IISEG_ERR_UNSUPPORTED;
    IISEG_LAUNCH(deconv_dgrad_bf16_kernel, dim3((unsigned)(p.T * p.ncib)), dim3(512), 0, (hipStream_t)stream, p, g, w,
                 gx);
    return iiseg_check_launch();
}
