// The narrow-Cout form of conv_wgrad_bf16.hip (ops.conv_wgrad(mma='bf16', co_block=16)):
// the same sums for the same descriptor,
//
//   dW[co][ci0 + ci][ky][kx] = sum_{b,y,x} bf16(g_z[b][co][y][x]) * bf16(xpad[b][ci][y + ky][x + kx])
//   db[co]                   = sum_{b,y,x} g_z[b][co][y][x]                      (the unrounded fp32 values)
//
// with x and g_z fp32 NCHW, each element rounded once, to nearest even, as it is staged into LDS, and fp32
// accumulation in a fixed order.  It is for layers with few output channels (FC-DenseNet's growth = 16), where
// the 64 x 64 block of conv_wgrad_bf16_kernel stages 64 g_z channels to use 16 and idles half its waves.
//
// A workgroup owns 16 output x 64 input channels x 9 taps of dW and a slab of 8 x 16 pixel tiles.  LDS holds
// [channel][pixel] bf16 images as there: g_z [16][8][16] (68-dword channels) and the x patch with its halo
// [64][10][20] (18 columns used, 100-dword channels), twice: 59 KiB.  (The input block is that kernel's on
// purpose: the slabs of a launch, and with them the cost of the finalize launch, which grows with their number and
// is a third of a 224 x 224 layer, are then its slabs; what the form saves is the 48 idle g_z channels per block.)
// One v_mfma_f32_16x16x32_bf16 takes TWO tile rows as k = 32 (A = g_z: row co = lane & 15; B = x: column ci = lane & 15; C: row 4 (lane >> 4) + reg, column lane & 15).
// The k-group g = lane >> 4 of a lane is (tile row 2 s + (g & 1), pixels 8 (g >> 1) .. + 7) in step s = 0 .. 3, for
// A and B alike: A is one 16-byte read, and for B the lane reads the ten patch pixels 8 (g >> 1) .. + 9 of a patch
// row once (five dwords) and forms the three kx operands in registers (kx = 1: v_alignbyte).  A lane needs the
// nine patch rows (g & 1) .. (g & 1) + 8: row 2 s + ky of them serves step s, tap row ky.  With channels 100
// dwords apart (36 mod 64) and the two tile rows of a 32-lane half 10 dwords apart, the 8-byte reads of a half
// fall on 64 distinct banks.
//
// The kernel is bound by the loads of x, not by its 36 MFMAs per 16 input channels and tile, so all eight waves
// load: wave w stages x channels w, w + 8, ... and g_z channels w, w + 8 of the block; waves 0-3 multiply, wave w
// input channels 16 w .. 16 w + 15 (nine accumulators of four registers; a wave whose channels lie past Cin skips
// the products).  Per tile a wave issues the loads of tile t + 1 into registers -- at most 28, every one at a clamped,
// always valid address, no branch among them --, multiplies tile t out of one LDS image while they are in flight,
// then rounds them and stores them into the other image; what lies outside the map or the active region becomes
// zero when it is stored.  One barrier per tile.  A block with at most 16 or 32 input channels stages only that
// many (nothing reads the rest of the image); a channel past Cin below that is the last real one again, whose
// products are never stored.
// Slabs, the finalize launch, the border share of db and the determinism contract are conv_wgrad.hip's.
#include "conv_wgrad_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TH = 8, TW = 16;                           // output pixel tile
constexpr int PH = TH + 2, PW = TW + 2;                  // its x patch
constexpr int CO = 16, CIB = 64;                         // channel block: output, input
constexpr int NWAVE = 8;
constexpr int NG = CO / NWAVE, NX = CIB / NWAVE;         // channels a wave stages: w, w + 8, ...
constexpr int MIN_TILES_PER_SLAB = 2;
constexpr int TARGET_WORKGROUPS = 256;                   // one per CU (conv_wgrad_bf16_kernel's count, see above)
constexpr int GLD = TH * TW + 8;                         // bf16 per g_z channel: 68 dwords
constexpr int XROW = 20;                                 // bf16 per patch row: 8-byte aligned rows
constexpr int XLD = PH * XROW;                           // bf16 per x channel: 100 dwords
constexpr int GPIX = TH * TW, XPIX = PH * PW;            // pixels of a channel's tile / patch
constexpr int GN = GPIX / 64, XN = (XPIX + 63) / 64;     // loads per lane and channel: pixel lane + 64 j

__device__ __forceinline__ bf16x8 frag(unsigned a, unsigned b, unsigned c, unsigned d) {
    u32x4 v;
    v.x = a; v.y = b; v.z = c; v.w = d;
    return __builtin_bit_cast(bf16x8, v);
}

// What a lane stages of one tile (conv_wgrad_bf16.hip's): pixels lane + 64 j of the g_z tile and of the x patch.
struct tile_lane {
    const float* g;                // g_z plane of the block's first output channel, this tile's image
    const float* x;                // x plane of the block's first input channel
    unsigned go[GN], xo[XN];       // byte offsets in a plane (a plane is < 2^32 bytes)
    bool gin[GN], xin[XN];
};

__global__ __launch_bounds__(512, 1) void conv_wgrad_bf16_co16_kernel(cw_params p, const float* __restrict__ x,
                                                                      const float* __restrict__ gz,
                                                                      float* __restrict__ dst,
                                                                      float* __restrict__ dbdst) {
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
        const unsigned short* ga = gs[buf] + ga_off;
        const unsigned short* xb = xs[buf] + xb_off;
        unsigned rows[PH - 1][5];                                        // patch pixels 8 half .. 8 half + 9 per row
#pragma unroll
        for (int pr = 0; pr < PH - 1; ++pr) {
            const u32x2 lo = *reinterpret_cast<const u32x2*>(xb + pr * XROW);
            const u32x2 hi = *reinterpret_cast<const u32x2*>(xb + pr * XROW + 4);
            rows[pr][0] = lo.x; rows[pr][1] = lo.y; rows[pr][2] = hi.x; rows[pr][3] = hi.y;
            rows[pr][4] = *reinterpret_cast<const unsigned*>(xb + pr * XROW + 8);
        }
#pragma unroll
        for (int s = 0; s < TH / 2; ++s) {
            const bf16x8 a = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(ga + 2 * s * TW));
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const unsigned* d = rows[2 * s + ky];
                const bf16x8 b0 = frag(d[0], d[1], d[2], d[3]);
                const bf16x8 b1 = frag(__builtin_amdgcn_alignbyte(d[1], d[0], 2), __builtin_amdgcn_alignbyte(d[2], d[1], 2),
                                       __builtin_amdgcn_alignbyte(d[3], d[2], 2), __builtin_amdgcn_alignbyte(d[4], d[3], 2));
                const bf16x8 b2 = frag(d[1], d[2], d[3], d[4]);
                acc[ky * 3 + 0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b0, acc[ky * 3 + 0], 0, 0, 0);
                acc[ky * 3 + 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b1, acc[ky * 3 + 1], 0, 0, 0);
                acc[ky * 3 + 2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b2, acc[ky * 3 + 2], 0, 0, 0);
            }
        }
    };

    // The slab with NXA x channels per wave: the loads of a tile are issued in one piece, at a wave-uniform plane
    // address plus a 32-bit lane offset, and stored after the products of the tile before it.
    auto run = [&](auto nxa) __attribute__((always_inline)) {
        constexpr int NXA = decltype(nxa)::value;
        tile_lane q;
        float gv[NG][GN], xv[NXA][XN];
        auto load = [&](long long t) __attribute__((always_inline)) {
            q = locate(t);
#pragma unroll
            for (int i = 0; i < NG; ++i) {
                const char* gc = reinterpret_cast<const char*>(q.g + min(NWAVE * i + wave, nco - 1) * gplane);
#pragma unroll
                for (int j = 0; j < GN; ++j) gv[i][j] = *reinterpret_cast<const float*>(gc + q.go[j]);
            }
#pragma unroll
            for (int i = 0; i < NXA; ++i) {
                const char* xc = reinterpret_cast<const char*>(q.x + min(NWAVE * i + wave, nci - 1) * xplane);
#pragma unroll
                for (int j = 0; j < XN; ++j) xv[i][j] = *reinterpret_cast<const float*>(xc + q.xo[j]);
            }
        };
        auto store = [&](int buf) __attribute__((always_inline)) {
            // pixel lane + 64 j of the patch sits at row k / PW, column k % PW of a channel's XROW-wide rows; a lane
            // without a pixel in the last pass stores its first one again
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

    // the block of dW: into dW itself (one slab) or into this slab of the workspace
    {
        float* out;
        long long so, sc;
        if (p.nslab == 1) { out = dst + (long long)p.ci0 * p.sc; so = p.so; sc = p.sc; }
        else { out = dst + (long long)slab * p.S; so = (long long)p.Cin * 9; sc = 9; }
        const int ci = 16 * wave + l15;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = 4 * g + r;
            if (co < nco && ci < nci) {
                float* o = out + (long long)(co0 + co) * so + (long long)(cb0 + ci) * sc;
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

// ---- host side ----
int cwb16_plan(const iiseg_conv_wgrad_desc* d, cw_params& p) {
    return cw_plan(d, p, TH, TW, CO, CIB, MIN_TILES_PER_SLAB, TARGET_WORKGROUPS);
}

}  // namespace

extern "C" int iiseg_conv_wgrad_bf16_co16_slabs(const iiseg_conv_wgrad_desc* d) {
    cw_params p;
    if (int st = cwb16_plan(d, p)) return st;
    return p.nslab;
}
extern "C" int64_t iiseg_conv_wgrad_bf16_co16_workspace_elems(const iiseg_conv_wgrad_desc* d) {
    const int n = iiseg_conv_wgrad_bf16_co16_slabs(d);
    if (n < 0) return n;
    return n == 1 ? 0 : (int64_t)n * ((int64_t)d->Cout * d->Cin * 9 + d->Cout);
}
extern "C" int iiseg_conv_wgrad_bf16_co16(void* stream, const iiseg_conv_wgrad_desc* d, const float* x,
                                          const float* gz, float* ws, float* dW, float* db) {
    cw_params p;
    if (int st = cwb16_plan(d, p)) return st;
    if (!x || !gz || !dW || (p.nslab > 1 && !ws)) return IISEG_ERR_NULL;
    p.want_db = db != nullptr;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)p.nslab, (unsigned)((p.Cout + CO - 1) / CO), (unsigned)((p.Cin + CIB - 1) / CIB));
    IISEG_LAUNCH(conv_wgrad_bf16_co16_kernel, grid, dim3(512), 0, s, p, x, gz, p.nslab == 1 ? dW : ws, db);
    if (p.nslab > 1)
        IISEG_LAUNCH(conv_wgrad_finalize_kernel<float>, dim3((unsigned)((p.S + 255) / 256)), dim3(256), 0, s,
                     (const float*)ws, p.nslab, p.S, p.nW, p.Cin, p.so, p.sc, p.ci0, dW, db);
    return iiseg_check_launch();
}
