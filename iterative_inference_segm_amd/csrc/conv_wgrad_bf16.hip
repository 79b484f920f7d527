// Weight and bias gradient of a zero-padded 3x3 stride-1 layer with the products on the 16-bit matrix pipe
// (wgrad='bf16'; DESIGN.md sections 15 and 22) -- conv_wgrad.hip's sums for the same descriptor,
//
//   dW[co][ci0 + ci][ky][kx] = sum_{b,y,x} bf16(g_z[b][co][y][x]) * bf16(xpad[b][ci][y + ky][x + kx])
//   db[co]                   = sum_{b,y,x} g_z[b][co][y][x]                      (the unrounded fp32 values)
//
// in two forms: conv_wgrad_bf16_kernel for 64 output channels per workgroup and conv_wgrad_bf16_co16_kernel for 16
// (ops.conv_wgrad(mma='bf16', co_block=16): layers with few output channels, FC-DenseNet's growth = 16, where the 64
// x 64 block stages 64 g_z channels to use 16 and idles half its waves).
//
// What the forms share.  x and g_z arrive as fp32 NCHW; each element is rounded once, to nearest even, as it is
// staged into LDS.  A product of two bf16 values is exact in fp32, so dW is an fp32 sum of exact products in a fixed
// order.  A workgroup of eight waves owns a CO output x 64 input channels x 9 taps block of dW and a slab of 8 x 16
// pixel tiles.  LDS holds [channel][pixel] bf16 images, twice: g_z [CO][8][16] (68-dword channels) and the x patch
// with its halo [64][10][20] (18 columns used; 40-byte rows).  A lane stages pixels lane + 64 j of a channel's tile
// and patch, rows first, so that consecutive lanes read consecutive addresses; every load is at a clamped, always
// valid address, a wave-uniform plane address plus a 32-bit lane offset -- no branch in the staging; what lies
// outside the map or the active region is replaced by zero when it is stored.  An MFMA takes pixels as k (A = g_z:
// row co, B = x: column ci): a lane's k-group is 8 consecutive pixels of a tile row, 16 contiguous bytes for A; for
// B the lane reads the ten patch pixels 8 h .. 8 h + 9 of a patch row once (five dwords) and forms the operands of
// the three kx from them in registers (kx = 1: v_alignbyte); a patch row serves the three ky of three tile rows.
// Tile t is multiplied out of one LDS image while tile t + 1 is loaded, rounded and stored into the other: one
// barrier per tile.  Slabs, the finalize launch, the border share of db and the determinism contract are
// conv_wgrad.hip's: no atomics, fixed orders, the same inputs give the same bits.  db's active part is summed from
// the fp32 values as they are staged (per lane over the slab's tiles, then across the wave).
// In code the forms share the tile constants, tile_lane, the loads of a channel plane and of the patch rows, the
// tap row (the kx operand triple and its three MFMAs), the dW destination and the host side.  Three pieces are the
// same text in both kernels and stay spelled out in each: `locate`, the rounding stores of a staged channel and
// the db tail.  As shared inline functions each of them made hipcc order or allocate one of the two kernels
// otherwise (profiles/wgrad_bf16_shared_core.md); a change to one of them goes into both.
//
// The 64-channel form: v_mfma_f32_32x32x16_bf16 takes a tile row of 16 pixels as k, the lane of k half h pixels
// 8 h .. 8 h + 7.  A wave cannot hold the nine 32 x 32 accumulators and a tile's worth of staged fp32 values at
// once, and with staging and MFMAs in turn the global-load latency is exposed.  So there are two waves per SIMD:
// waves 0-3 multiply tile t (wave w the sub-block of co half w & 1, ci half w >> 1) while waves 4-7 load tile t + 1
// into registers (wave w channels w, w + 4, ... of g_z and of x), round it and store it.  A channel past nco / nci
// reads the block's last real one again; its products are finite and never stored.
//
// The 16-channel form: v_mfma_f32_16x16x32_bf16 takes TWO tile rows as k = 32 (A: row co = lane & 15; B: column
// ci = lane & 15; C: row 4 (lane >> 4) + reg, column lane & 15).  The k-group g = lane >> 4 of a lane is (tile row
// 2 s + (g & 1), pixels 8 (g >> 1) .. + 7) in step s = 0 .. 3, for A and B alike; a lane needs the nine patch rows
// (g & 1) .. (g & 1) + 8: row 2 s + ky of them serves step s, tap row ky.  The input block is the other form's on
// purpose: the slabs of a launch, and with them the cost of the finalize launch, which grows with their number and
// is a third of a 224 x 224 layer, are then its slabs; what the form saves is the 48 idle g_z channels per block
// (59 KiB of LDS).  The kernel is bound by the loads of x, not by its 36 MFMAs per 16 input channels and tile, so
// all eight waves load: wave w stages x channels w, w + 8, ... and g_z channels w, w + 8 of the block; waves 0-3
// multiply, wave w input channels 16 w .. 16 w + 15 (nine accumulators of four registers; a wave whose channels lie
// past Cin skips the products).  Per tile a wave issues the loads of tile t + 1 -- at most 28 --, multiplies tile t
// while they are in flight, then rounds and stores them.  A block with at most 16 or 32 input channels stages only
// that many (nothing reads the rest of the image); a channel past Cin below that is the last real one again.
#include "conv_wgrad_common.h"

namespace {

// ---------------------------------------------------------------- what the two forms share
constexpr int TH = 8, TW = 16;                           // output pixel tile
constexpr int PH = TH + 2, PW = TW + 2;                  // its x patch
constexpr int CIB = 64;                                  // input channels of a block
constexpr int NWAVE = 8;
constexpr int MIN_TILES_PER_SLAB = 2;
constexpr int TARGET_WORKGROUPS = 256;                   // one per CU: a workgroup takes a CU's waves and LDS
constexpr int GLD = TH * TW + 8;                         // bf16 per g_z channel: 68 dwords
constexpr int XROW = 20;                                 // bf16 per patch row: 8-byte aligned rows
constexpr int GPIX = TH * TW, XPIX = PH * PW;            // pixels of a channel's tile / patch
constexpr int GN = GPIX / 64, XN = (XPIX + 63) / 64;     // loads per lane and channel: pixel lane + 64 j

// What a lane stages of one tile: pixels lane + 64 j of the g_z tile and of the x patch -- the same for each of
// the wave's channels.  Offsets are clamped into the map; the flags say which of the loaded values are real.
struct tile_lane {
    const float* g;                // g_z plane of the block's first output channel, this tile's image
    const float* x;                // x plane of the block's first input channel
    unsigned go[GN], xo[XN];       // byte offsets in a plane (a plane is < 2^32 bytes)
    bool gin[GN], xin[XN];
};

// The lane's pixels of one channel plane, into registers.
template <int N>
__device__ __forceinline__ void load_plane(const float* plane, const unsigned (&off)[N], float (&v)[N]) {
    const char* c = reinterpret_cast<const char*>(plane);
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = *reinterpret_cast<const float*>(c + off[j]);
}

// The ten patch pixels 8 half .. 8 half + 9 of NR patch rows, from the lane's place `xb` in its channel.
template <int NR>
__device__ __forceinline__ void load_patch_rows(const unsigned short* xb, unsigned (&rows)[NR][5]) {
#pragma unroll
    for (int pr = 0; pr < NR; ++pr) {
        const u32x2 lo = *reinterpret_cast<const u32x2*>(xb + pr * XROW);
        const u32x2 hi = *reinterpret_cast<const u32x2*>(xb + pr * XROW + 4);
        rows[pr][0] = lo.x; rows[pr][1] = lo.y; rows[pr][2] = hi.x; rows[pr][3] = hi.y;
        rows[pr][4] = *reinterpret_cast<const unsigned*>(xb + pr * XROW + 8);
    }
}

// The MFMA of a form is the one of its accumulator ...
__device__ __forceinline__ f32x16 mfma(bf16x8 a, bf16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
// ... and one tap row is three of them: the operands of kx = 0, 1, 2 from the five dwords `d` of a patch row
template <typename ACC>
__device__ __forceinline__ void tap_row(bf16x8 a, const unsigned* d, ACC* acc) {
    const bf16x8 b0 = frag(d[0], d[1], d[2], d[3]);
    const bf16x8 b1 = frag_shift1(d[0], d[1], d[2], d[3], d[4]);
    const bf16x8 b2 = frag(d[1], d[2], d[3], d[4]);
    acc[0] = mfma(a, b0, acc[0]);
    acc[1] = mfma(a, b1, acc[1]);
    acc[2] = mfma(a, b2, acc[2]);
}

// Where the block of dW goes: into dW itself (one slab) or into this slab of the workspace.
struct dw_dest {
    float* out;
    long long so, sc;
};
__device__ __forceinline__ dw_dest dw_destination(const cw_params& p, float* dst, int slab) {
    if (p.nslab == 1) return {dst + (long long)p.ci0 * p.sc, p.so, p.sc};
    return {dst + (long long)slab * p.S, (long long)p.Cin * 9, 9};
}

// ---------------------------------------------------------------- the 64-channel form
namespace cb64 {
constexpr int CO = 64;
constexpr int NCH = CO / 4;                              // channels a staging wave stages: w, w + 4, ...
// bf16 per x channel: 102 dwords.  A lane reads 8 bytes at (channel l31) * 102 + 4 half dwords: 102 = 38 mod 64 keeps
// the 32 lanes of a half on distinct banks (as 68 does for g_z's 16-byte reads)
constexpr int XLD = PH * XROW + 4;
}  // namespace cb64

__global__ __launch_bounds__(512, 1) void conv_wgrad_bf16_kernel(cw_params p, const float* __restrict__ x,
                                                                 const float* __restrict__ gz, float* __restrict__ dst,
                                                                 float* __restrict__ dbdst) {
    using namespace cb64;
    __shared__ __attribute__((aligned(16))) unsigned short gs[2][CO * GLD];
    __shared__ __attribute__((aligned(16))) unsigned short xs[2][CIB * XLD];
    __shared__ float asum[CO], bsum[CO];
    const int tid = threadIdx.x, lane = tid & 63;
    // eight waves: 0-3 multiply tile t while 4-7 stage tile t + 1; `sw` is a wave's place among its four (in a
    // scalar register: what is indexed by it stays wave-uniform)
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), sw = wave & 3;
    const bool stager = wave >= 4;
    const int slab = blockIdx.x, co0 = blockIdx.y * CO, cb0 = blockIdx.z * CIB;
    const int nco = min(CO, p.Cout - co0), nci = min(CIB, p.Cin - cb0);
    const bool do_db = p.want_db && blockIdx.z == 0;

    const int yend = p.ay0 + p.AH, xend = p.ax0 + p.AW;
    const int per_img = p.tilesY * p.tilesX;
    const size_t gplane = (size_t)p.OH * p.OW, xplane = (size_t)p.H * p.W;
    const long long t0 = (long long)slab * p.tps, t1 = min(p.T, t0 + p.tps);

    // The two roles are two code paths with the same barriers, one before the first tile and one per tile, so
    // that neither holds the other's registers.
    if (stager) {
        auto locate = [&](long long t) {
            tile_lane q;
            // (the divisions run on the vector ALU: back into scalar registers, so that the plane addresses are)
            const int b = __builtin_amdgcn_readfirstlane((int)(t / per_img));
            const int rem = __builtin_amdgcn_readfirstlane((int)(t % per_img));
            const int ty = __builtin_amdgcn_readfirstlane(rem / p.tilesX);
            const int y0 = p.ay0 + ty * TH, x0 = p.ax0 + (rem - ty * p.tilesX) * TW;
            q.g = gz + ((size_t)b * p.Cout + co0) * gplane;
            q.x = x + ((size_t)b * p.Cin + cb0) * xplane;
#pragma unroll
            for (int j = 0; j < GN; ++j) {
                const int k = lane + 64 * j, y = y0 + k / TW, xx = x0 + k % TW;
                q.gin[j] = y < yend && xx < xend;
                q.go[j] = 4u * (unsigned)(min(y, yend - 1) * p.OW + min(xx, xend - 1));
            }
#pragma unroll
            for (int j = 0; j < XN; ++j) {
                const int k = lane + 64 * j, iy = y0 - p.pad + k / PW, ix = x0 - p.pad + k % PW;
                q.xin[j] = k < XPIX && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
                q.xo[j] = 4u * (unsigned)(min(max(iy, 0), p.H - 1) * p.W + min(max(ix, 0), p.W - 1));
            }
            return q;
        };
        float dbacc[NCH];                                                // db: channel 4 i + sw, this lane's pixels
#pragma unroll
        for (int i = 0; i < NCH; ++i) dbacc[i] = 0.f;
        // One tile: every load first, then the rounding and the LDS stores.  Pixel lane + 64 j of the patch sits at
        // row k / PW, column k % PW of a channel's XROW-wide rows; a lane without a pixel in the last pass stores
        // its first one again.
        auto stage = [&](long long t, int buf) {
            const tile_lane q = locate(t);
            float gv[NCH][GN], xv[NCH][XN];
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const int c = 4 * i + sw;
                load_plane(q.g + min(c, nco - 1) * gplane, q.go, gv[i]);
                load_plane(q.x + min(c, nci - 1) * xplane, q.xo, xv[i]);
            }
            int xoff[XN];
#pragma unroll
            for (int j = 0; j < XN; ++j) {
                const int k = lane + 64 * j < XPIX ? lane + 64 * j : lane;
                xoff[j] = (k / PW) * XROW + k % PW;
            }
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const int c = 4 * i + sw;
#pragma unroll
                for (int j = 0; j < GN; ++j) {
                    const float v = q.gin[j] ? gv[i][j] : 0.f;
                    dbacc[i] += v;
                    gs[buf][c * GLD + lane + 64 * j] = to_bf16(v);
                }
                const unsigned short first = to_bf16(q.xin[0] ? xv[i][0] : 0.f);
#pragma unroll
                for (int j = 0; j < XN; ++j)
                    xs[buf][c * XLD + xoff[j]] = lane + 64 * j < XPIX ? to_bf16(q.xin[j] ? xv[i][j] : 0.f) : first;
            }
        };
        if (t0 < t1) stage(t0, 0);
        __syncthreads();
        int buf = 0;
        for (long long t = t0; t < t1; ++t, buf ^= 1) {
            if (t + 1 < t1) stage(t + 1, buf ^ 1);
            __syncthreads();                                             // image buf is read, image buf ^ 1 written
        }
        if (do_db) {
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const float s = wave_sum(dbacc[i]);
                if (lane == 0) asum[4 * i + sw] = s;
            }
        }
    } else {
        // wave -> (co half, ci half), lane -> channel within the half and k half
        const int cw = sw & 1, ciw = sw >> 1, l31 = lane & 31, half = lane >> 5;
        const bool wave_on = cw * 32 < nco && ciw * 32 < nci;            // wave-uniform
        const int ga_off = (cw * 32 + l31) * GLD + 8 * half, xb_off = (ciw * 32 + l31) * XLD + 8 * half;
        f32x16 acc[9];
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
        __syncthreads();
        int buf = 0;
        for (long long t = t0; t < t1; ++t, buf ^= 1) {
            if (wave_on) {
                const unsigned short* ga = gs[buf] + ga_off;
                unsigned rows[PH][5];                                    // a patch row serves three tile rows
                load_patch_rows(xs[buf] + xb_off, rows);
#pragma unroll
                for (int r = 0; r < TH; ++r) {
                    const bf16x8 a = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(ga + r * TW));
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky) tap_row(a, rows[r + ky], acc + ky * 3);
                }
            }
            __syncthreads();
        }
        const dw_dest w = dw_destination(p, dst, slab);
        if (wave_on) {
            const int ci = ciw * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = cw * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (co < nco && ci < nci) {
                    float* o = w.out + (long long)(co0 + co) * w.so + (long long)(cb0 + ci) * w.sc;
#pragma unroll
                    for (int tap = 0; tap < 9; ++tap) o[tap] = acc[tap][r];
                }
            }
        }
    }

    // ---- db: active pixels (summed at staging) + this slab's share of the border pixels ----
    if (!do_db) return;                                                  // block-uniform
    const long long NB = (long long)p.B * p.nb;
    const long long q0 = min(NB, (long long)slab * p.bps), q1 = min(NB, q0 + p.bps);
    for (int c = wave; c < nco; c += NWAVE) {
        float s = 0;
        for (long long q = q0 + lane; q < q1; q += 64) {
            int y, xx;
            border_pixel(p, q % p.nb, y, xx);
            s += gz[(((size_t)(q / p.nb) * p.Cout + co0 + c) * p.OH + y) * p.OW + xx];
        }
        s = wave_sum(s);
        if (lane == 0) bsum[c] = s;
    }
    __syncthreads();
    float* dbo = p.nslab == 1 ? dbdst : dst + (long long)slab * p.S + p.nW;
    if (tid < nco) dbo[co0 + tid] = asum[tid] + bsum[tid];
}

// ---------------------------------------------------------------- the 16-channel form
namespace co16 {
constexpr int CO = 16;
constexpr int NG = CO / NWAVE, NX = CIB / NWAVE;         // channels a wave stages: w, w + 8, ...
// bf16 per x channel: 100 dwords.  With channels 100 dwords apart (36 mod 64) and the two tile rows of a 32-lane
// half 10 dwords apart, the 8-byte reads of a half fall on 64 distinct banks
constexpr int XLD = PH * XROW;
}  // namespace co16

__global__ __launch_bounds__(512, 1) void conv_wgrad_bf16_co16_kernel(cw_params p, const float* __restrict__ x,
                                                                      const float* __restrict__ gz,
                                                                      float* __restrict__ dst,
                                                                      float* __restrict__ dbdst) {
    using namespace co16;
    __shared__ __attribute__((aligned(16))) unsigned short gs[2][CO * GLD];
    __shared__ __attribute__((aligned(16))) unsigned short xs[2][CIB * XLD];
    __shared__ float asum[CO], bsum[CO];
    const int tid = threadIdx.x, lane = tid & 63;
    // (in a scalar register: what is indexed by it stays wave-uniform)
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int slab = blockIdx.x, co0 = blockIdx.y * CO, cb0 = blockIdx.z * CIB;
    const int nco = min(CO, p.Cout - co0), nci = min(CIB, p.Cin - cb0);
    const bool do_db = p.want_db && blockIdx.z == 0;

    const int yend = p.ay0 + p.AH, xend = p.ax0 + p.AW;
    const int per_img = p.tilesY * p.tilesX;
    const size_t gplane = (size_t)p.OH * p.OW, xplane = (size_t)p.H * p.W;
    const long long t0 = (long long)slab * p.tps, t1 = min(p.T, t0 + p.tps);

    auto locate = [&](long long t) __attribute__((always_inline)) {
        tile_lane q;
        // (the divisions run on the vector ALU: back into scalar registers, so that the plane addresses are)
        const int b = __builtin_amdgcn_readfirstlane((int)(t / per_img));
        const int rem = __builtin_amdgcn_readfirstlane((int)(t % per_img));
        const int ty = __builtin_amdgcn_readfirstlane(rem / p.tilesX);
        const int y0 = p.ay0 + ty * TH, x0 = p.ax0 + (rem - ty * p.tilesX) * TW;
        q.g = gz + ((size_t)b * p.Cout + co0) * gplane;
        q.x = x + ((size_t)b * p.Cin + cb0) * xplane;
#pragma unroll
        for (int j = 0; j < GN; ++j) {
            const int k = lane + 64 * j, y = y0 + k / TW, xx = x0 + k % TW;
            q.gin[j] = y < yend && xx < xend;
            q.go[j] = 4u * (unsigned)(min(y, yend - 1) * p.OW + min(xx, xend - 1));
        }
#pragma unroll
        for (int j = 0; j < XN; ++j) {
            const int k = lane + 64 * j, iy = y0 - p.pad + k / PW, ix = x0 - p.pad + k % PW;
            q.xin[j] = k < XPIX && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
            q.xo[j] = 4u * (unsigned)(min(max(iy, 0), p.H - 1) * p.W + min(max(ix, 0), p.W - 1));
        }
        return q;
    };

    // lane -> channel within the wave's 16 and k-group g = (tile row of the pair, pixel half)
    const int l15 = lane & 15, g = lane >> 4, rr = g & 1, half = g >> 1;
    const int ga_off = l15 * GLD + rr * TW + 8 * half;
    const int xb_off = (16 * (wave & 3) + l15) * XLD + rr * XROW + 8 * half;
    const bool wave_on = 16 * wave < nci;                                // wave-uniform; false on waves 4-7
    f32x4 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[t][r] = 0.f;
    float dbacc[NG];                                                     // db: channel 8 i + wave, this lane's pixels
#pragma unroll
    for (int i = 0; i < NG; ++i) dbacc[i] = 0.f;

    // The products of one tile out of LDS image `buf`.
    auto multiply = [&](int buf) __attribute__((always_inline)) {
        unsigned rows[PH - 1][5];
        load_patch_rows(xs[buf] + xb_off, rows);
        const unsigned short* ga = gs[buf] + ga_off;
#pragma unroll
        for (int s = 0; s < TH / 2; ++s) {
            const bf16x8 a = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(ga + 2 * s * TW));
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) tap_row(a, rows[2 * s + ky], acc + ky * 3);
        }
    };

    // The slab with NXA x channels per wave: the loads of a tile are issued in one piece and stored after the
    // products of the tile before it.
    auto run = [&](auto nxa) __attribute__((always_inline)) {
        constexpr int NXA = decltype(nxa)::value;
        tile_lane q;
        float gv[NG][GN], xv[NXA][XN];
        auto load = [&](long long t) __attribute__((always_inline)) {
            q = locate(t);
#pragma unroll
            for (int i = 0; i < NG; ++i) load_plane(q.g + min(NWAVE * i + wave, nco - 1) * gplane, q.go, gv[i]);
#pragma unroll
            for (int i = 0; i < NXA; ++i) load_plane(q.x + min(NWAVE * i + wave, nci - 1) * xplane, q.xo, xv[i]);
        };
        auto store = [&](int buf) __attribute__((always_inline)) {
            int xoff[XN];
#pragma unroll
            for (int j = 0; j < XN; ++j) {
                const int k = lane + 64 * j < XPIX ? lane + 64 * j : lane;
                xoff[j] = (k / PW) * XROW + k % PW;
            }
#pragma unroll
            for (int i = 0; i < NG; ++i) {
                const int c = NWAVE * i + wave;
#pragma unroll
                for (int j = 0; j < GN; ++j) {
                    const float v = q.gin[j] ? gv[i][j] : 0.f;
                    dbacc[i] += v;
                    gs[buf][c * GLD + lane + 64 * j] = to_bf16(v);
                }
            }
#pragma unroll
            for (int i = 0; i < NXA; ++i) {
                const int c = NWAVE * i + wave;
                const unsigned short first = to_bf16(q.xin[0] ? xv[i][0] : 0.f);
#pragma unroll
                for (int j = 0; j < XN; ++j)
                    xs[buf][c * XLD + xoff[j]] = lane + 64 * j < XPIX ? to_bf16(q.xin[j] ? xv[i][j] : 0.f) : first;
            }
        };
        if (t0 < t1) {
            load(t0);
            store(0);
        }
        __syncthreads();
        int buf = 0;
        for (long long t = t0; t < t1; ++t, buf ^= 1) {
            const bool more = t + 1 < t1;                                // block-uniform
            if (more) load(t + 1);
            if (wave_on) multiply(buf);
            if (more) store(buf ^ 1);
            __syncthreads();                                             // image buf is read, image buf ^ 1 written
        }
    };
    if (nci <= CIB / 4) run(std::integral_constant<int, NX / 4>());
    else if (nci <= CIB / 2) run(std::integral_constant<int, NX / 2>());
    else run(std::integral_constant<int, NX>());

    {
        const dw_dest w = dw_destination(p, dst, slab);
        const int ci = 16 * wave + l15;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = 4 * g + r;
            if (co < nco && ci < nci) {
                float* o = w.out + (long long)(co0 + co) * w.so + (long long)(cb0 + ci) * w.sc;
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) o[tap] = acc[tap][r];
            }
        }
    }

    // ---- db: active pixels (summed at staging) + this slab's share of the border pixels ----
    if (!do_db) return;                                                  // block-uniform
#pragma unroll
    for (int i = 0; i < NG; ++i) {
        const float s = wave_sum(dbacc[i]);
        if (lane == 0) asum[NWAVE * i + wave] = s;
    }
    const long long NB = (long long)p.B * p.nb;
    const long long q0 = min(NB, (long long)slab * p.bps), q1 = min(NB, q0 + p.bps);
    for (int c = wave; c < nco; c += NWAVE) {
        float s = 0;
        for (long long q = q0 + lane; q < q1; q += 64) {
            int y, xx;
            border_pixel(p, q % p.nb, y, xx);
            s += gz[(((size_t)(q / p.nb) * p.Cout + co0 + c) * p.OH + y) * p.OW + xx];
        }
        s = wave_sum(s);
        if (lane == 0) bsum[c] = s;
    }
    __syncthreads();
    float* dbo = p.nslab == 1 ? dbdst : dst + (long long)slab * p.S + p.nW;
    if (tid < nco) dbo[co0 + tid] = asum[tid] + bsum[tid];
}

// ---------------------------------------------------------------- host side, per form
struct form_cb64 {
    static constexpr int CO = cb64::CO;
    static constexpr auto kernel = conv_wgrad_bf16_kernel;
};
struct form_co16 {
    static constexpr int CO = co16::CO;
    static constexpr auto kernel = conv_wgrad_bf16_co16_kernel;
};

template <typename F>
int cwb_plan(const iiseg_conv_wgrad_desc* d, cw_params& p) {
    return cw_plan(d, p, TH, TW, F::CO, CIB, MIN_TILES_PER_SLAB, TARGET_WORKGROUPS);
}
template <typename F>
int cwb_slabs(const iiseg_conv_wgrad_desc* d) {
    cw_params p;
    if (int st = cwb_plan<F>(d, p)) return st;
    return p.nslab;
}
template <typename F>
int64_t cwb_workspace_elems(const iiseg_conv_wgrad_desc* d) {
    const int n = cwb_slabs<F>(d);
    if (n < 0) return n;
    return n == 1 ? 0 : (int64_t)n * ((int64_t)d->Cout * d->Cin * 9 + d->Cout);
}
template <typename F>
int cwb_launch(void* stream, const iiseg_conv_wgrad_desc* d, const float* x, const float* gz, float* ws, float* dW,
               float* db) {
    cw_params p;
    if (int st = cwb_plan<F>(d, p)) return st;
    if (!x || !gz || !dW || (p.nslab > 1 && !ws)) return IISEG_ERR_NULL;
    p.want_db = db != nullptr;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)p.nslab, (unsigned)((p.Cout + F::CO - 1) / F::CO), (unsigned)((p.Cin + CIB - 1) / CIB));
    IISEG_LAUNCH(F::kernel, grid, dim3(512), 0, s, p, x, gz, p.nslab == 1 ? dW : ws, db);
    if (p.nslab > 1)
        IISEG_LAUNCH(conv_wgrad_finalize_kernel<float>, dim3((unsigned)((p.S + 255) / 256)), dim3(256), 0, s,
                     (const float*)ws, p.nslab, p.S, p.nW, p.Cin, p.so, p.sc, p.ci0, dW, db);
    return iiseg_check_launch();
}

}  // namespace

extern "C" int iiseg_conv_wgrad_bf16_slabs(const iiseg_conv_wgrad_desc* d) { return cwb_slabs<form_cb64>(d); }
extern "C" int64_t iiseg_conv_wgrad_bf16_workspace_elems(const iiseg_conv_wgrad_desc* d) {
    return cwb_workspace_elems<form_cb64>(d);
}
extern "C" int iiseg_conv_wgrad_bf16(void* stream, const iiseg_conv_wgrad_desc* d, const float* x, const float* gz,
                                     float* ws, float* dW, float* db) {
    return cwb_launch<form_cb64>(stream, d, x, gz, ws, dW, db);
}
extern "C" int iiseg_conv_wgrad_bf16_co16_slabs(const iiseg_conv_wgrad_desc* d) { return cwb_slabs<form_co16>(d); }
extern "C" int64_t iiseg_conv_wgrad_bf16_co16_workspace_elems(const iiseg_conv_wgrad_desc* d) {
    return cwb_workspace_elems<form_co16>(d);
}
extern "C" int iiseg_conv_wgrad_bf16_co16(void* stream, const iiseg_conv_wgrad_desc* d, const float* x,
                                          const float* gz, float* ws, float* dW, float* db) {
    return cwb_launch<form_co16>(stream, d, x, gz, ws, dW, db);
}
