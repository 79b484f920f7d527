// Weight and bias gradient of a zero-padded 3x3 stride-1 layer with the products on the 16-bit matrix pipe
// (wgrad='bf16') -- conv_wgrad.hip's sums for the same descriptor,
//
//   dW[co][ci0 + ci][ky][kx] = sum_{b,y,x} bf16(g_z[b][co][y][x]) * bf16(xpad[b][ci][y + ky][x + kx])
//   db[co]                   = sum_{b,y,x} g_z[b][co][y][x]                      (the unrounded fp32 values)
//
// x and g_z arrive as fp32 NCHW; each element is rounded once, to nearest even, as it is staged into LDS.  A
// product of two bf16 values is exact in fp32, so dW is an fp32 sum of exact products in a fixed order.
//
// A workgroup owns a 64 output x 64 input channels x 9 taps block of dW and a slab of 8 x 16 pixel tiles; wave w
// owns the 32 x 32 sub-block (co half w & 1, ci half w >> 1) in nine accumulators.  LDS holds [channel][pixel]
// bf16 images: g_z [co][8][16] and the x patch with its halo [ci][10][20] (18 columns used; 40-byte rows).  One
// v_mfma_f32_32x32x16_bf16 takes a tile row of 16 pixels as k (A = g_z: row co, k = pixel; B = x: k = pixel,
// column ci): the lane of k half h reads pixels 8h .. 8h+7 of its channel's row, 16 contiguous bytes for A.  For
// B the lane reads the ten patch pixels 8h .. 8h+9 of a patch row once (five dwords) and forms the operands of
// the three kx from them in registers (kx = 1: v_alignbyte); a patch row serves the three ky of three tile rows.
// Channel strides of 68 (g_z) and 102 (x) dwords keep the 32 lanes of a half on distinct banks.
//
// A wave cannot hold the nine accumulators and a tile's worth of staged fp32 values at once, and with staging and
// MFMAs in turn the global-load latency is exposed.  So the workgroup has eight waves, two per SIMD: waves 0-3
// multiply tile t out of one LDS image while waves 4-7 load tile t + 1 into registers, round it and store it into
// the other image; one barrier per tile.  Every load is at a clamped, always valid address -- no branch in the
// staging; what lies outside the map or the active region is replaced by zero when it is stored.
// Slabs, the finalize launch, the border share of db and the determinism contract are conv_wgrad.hip's: no
// atomics, fixed orders, the same inputs give the same bits.  db's active part is summed from the fp32 values as
// they are staged (per lane over the slab's tiles, then across the wave).
#include "conv_wgrad_common.h"

namespace {

constexpr int TH = 8, TW = 16;                           // output pixel tile
constexpr int PH = TH + 2, PW = TW + 2;                  // its x patch
constexpr int CB = 64;                                   // channel block, both ways
constexpr int NCH = CB / 4;                              // channels a wave stages: w, w + 4, ...
constexpr int MIN_TILES_PER_SLAB = 2;
constexpr int TARGET_WORKGROUPS = 256;                   // one per CU: a workgroup takes a CU's waves and LDS
constexpr int GLD = TH * TW + 8;                         // bf16 per g_z channel: 68 dwords
constexpr int XROW = 20;                                 // bf16 per patch row: 8-byte aligned rows
constexpr int XLD = PH * XROW + 4;                       // bf16 per x channel: 102 dwords
constexpr int GPIX = TH * TW, XPIX = PH * PW;            // pixels of a channel's tile / patch
constexpr int GN = GPIX / 64, XN = (XPIX + 63) / 64;     // loads per lane and channel: pixel lane + 64 j

__device__ __forceinline__ bf16x8 frag(unsigned a, unsigned b, unsigned c, unsigned d) {
    u32x4 v;
    v.x = a; v.y = b; v.z = c; v.w = d;
    return __builtin_bit_cast(bf16x8, v);
}

// What a lane stages of one tile: pixels lane + 64 j of the g_z tile and of the x patch, rows first, so that
// consecutive lanes read consecutive addresses -- the same for each of the wave's channels.  Offsets are clamped
// into the map; the flags say which of the loaded values are real.
struct tile_lane {
    const float* g;                // g_z plane of the block's first output channel, this tile's image
    const float* x;                // x plane of the block's first input channel
    unsigned go[GN], xo[XN];       // byte offsets in a plane (a plane is < 2^32 bytes)
    bool gin[GN], xin[XN];
};

__global__ __launch_bounds__(512, 1) void conv_wgrad_bf16_kernel(cw_params p, const float* __restrict__ x,
                                                                 const float* __restrict__ gz, float* __restrict__ dst,
                                                                 float* __restrict__ dbdst) {
    __shared__ __attribute__((aligned(16))) unsigned short gs[2][CB * GLD];
    __shared__ __attribute__((aligned(16))) unsigned short xs[2][CB * XLD];
    __shared__ float asum[CB], bsum[CB];
    const int tid = threadIdx.x, lane = tid & 63;
    // eight waves: 0-3 multiply tile t while 4-7 stage tile t + 1; `sw` is a wave's place among its four (in a
    // scalar register: what is indexed by it stays wave-uniform)
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), sw = wave & 3;
    const bool stager = wave >= 4;
    const int slab = blockIdx.x, co0 = blockIdx.y * CB, cb0 = blockIdx.z * CB;
    const int nco = min(CB, p.Cout - co0), nci = min(CB, p.Cin - cb0);
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
        // One tile: every load first, at a wave-uniform plane address plus a 32-bit lane offset, then the rounding
        // and the LDS stores.  No branch: a channel past nco / nci reads the block's last real one again; its
        // products are finite and never stored.
        auto stage = [&](long long t, int buf) {
            const tile_lane q = locate(t);
            float gv[NCH][GN], xv[NCH][XN];
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const int c = 4 * i + sw;
                const char* g = reinterpret_cast<const char*>(q.g + min(c, nco - 1) * gplane);
#pragma unroll
                for (int j = 0; j < GN; ++j) gv[i][j] = *reinterpret_cast<const float*>(g + q.go[j]);
                const char* xc = reinterpret_cast<const char*>(q.x + min(c, nci - 1) * xplane);
#pragma unroll
                for (int j = 0; j < XN; ++j) xv[i][j] = *reinterpret_cast<const float*>(xc + q.xo[j]);
            }
            // pixel lane + 64 j of the patch sits at row k / PW, column k % PW of a channel's XROW-wide rows; a lane
            // without a pixel in the last pass stores its first one again
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
                const unsigned short* xb = xs[buf] + xb_off;
                unsigned rows[PH][5];                                    // patch pixels 8 half .. 8 half + 9 per row
#pragma unroll
                for (int pr = 0; pr < PH; ++pr) {
                    const u32x2 lo = *reinterpret_cast<const u32x2*>(xb + pr * XROW);
                    const u32x2 hi = *reinterpret_cast<const u32x2*>(xb + pr * XROW + 4);
                    rows[pr][0] = lo.x; rows[pr][1] = lo.y; rows[pr][2] = hi.x; rows[pr][3] = hi.y;
                    rows[pr][4] = *reinterpret_cast<const unsigned*>(xb + pr * XROW + 8);
                }
#pragma unroll
                for (int r = 0; r < TH; ++r) {
                    const bf16x8 a = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(ga + r * TW));
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky) {
                        const unsigned* d = rows[r + ky];
                        const bf16x8 b0 = frag(d[0], d[1], d[2], d[3]);
                        const bf16x8 b1 = frag(__builtin_amdgcn_alignbyte(d[1], d[0], 2), __builtin_amdgcn_alignbyte(d[2], d[1], 2),
                                               __builtin_amdgcn_alignbyte(d[3], d[2], 2), __builtin_amdgcn_alignbyte(d[4], d[3], 2));
                        const bf16x8 b2 = frag(d[1], d[2], d[3], d[4]);
                        acc[ky * 3 + 0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b0, acc[ky * 3 + 0], 0, 0, 0);
                        acc[ky * 3 + 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b1, acc[ky * 3 + 1], 0, 0, 0);
                        acc[ky * 3 + 2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b2, acc[ky * 3 + 2], 0, 0, 0);
                    }
                }
            }
            __syncthreads();
        }
        // the block of dW: into dW itself (one slab) or into this slab of the workspace
        float* out;
        long long so, sc;
        if (p.nslab == 1) { out = dst + (long long)p.ci0 * p.sc; so = p.so; sc = p.sc; }
        else { out = dst + (long long)slab * p.S; so = (long long)p.Cin * 9; sc = 9; }
        if (wave_on) {
            const int ci = ciw * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = cw * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (co < nco && ci < nci) {
                    float* o = out + (long long)(co0 + co) * so + (long long)(cb0 + ci) * sc;
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
    for (int c = wave; c < nco; c += 8) {
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
int cwb_plan(const iiseg_conv_wgrad_desc* d, cw_params& p) {
    return cw_plan(d, p, TH, TW, CB, MIN_TILES_PER_SLAB, TARGET_WORKGROUPS);
}

}  // namespace

extern "C" int iiseg_conv_wgrad_bf16_slabs(const iiseg_conv_wgrad_desc* d) {
    cw_params p;
    if (int st = cwb_plan(d, p)) return st;
    return p.nslab;
}
extern "C" int64_t iiseg_conv_wgrad_bf16_workspace_elems(const iiseg_conv_wgrad_desc* d) {
    const int n = iiseg_conv_wgrad_bf16_slabs(d);
    if (n < 0) return n;
    return n == 1 ? 0 : (int64_t)n * ((int64_t)d->Cout * d->Cin * 9 + d->Cout);
}
extern "C" int iiseg_conv_wgrad_bf16(void* stream, const iiseg_conv_wgrad_desc* d, const float* x, const float* gz,
                                     float* ws, float* dW, float* db) {
    cw_params p;
    if (int st = cwb_plan(d, p)) return st;
    if (!x || !gz || !dW || (p.nslab > 1 && !ws)) return IISEG_ERR_NULL;
    p.want_db = db != nullptr;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)p.nslab, (unsigned)((p.Cout + CB - 1) / CB), (unsigned)((p.Cin + CB - 1) / CB));
    IISEG_LAUNCH(conv_wgrad_bf16_kernel, grid, dim3(512), 0, s, p, x, gz, p.nslab == 1 ? dW : ws, db);
    if (p.nslab > 1)
        IISEG_LAUNCH(conv_wgrad_finalize_kernel<float>, dim3((unsigned)((p.S + 255) / 256)), dim3(256), 0, s,
                     (const float*)ws, p.nslab, p.S, p.nW, p.Cin, p.so, p.sc, p.ci0, dW, db);
    return iiseg_check_launch();
}
