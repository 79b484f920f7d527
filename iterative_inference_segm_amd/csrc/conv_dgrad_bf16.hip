// Data gradient of a zero-padded 3x3 stride-1 pad-1 layer with the products on the 16-bit matrix pipe
// (dgrad='bf16'):
//
//   gx[b][ci][y][x] = sum_{co,ky,kx} bf16(W[co][ci0 + ci][ky][kx]) * bf16(g_z[b][co][y + 1 - ky][x + 1 - kx])
//
// g_z is zero outside its plane.  g_z arrives as fp32 NCHW and each element is rounded once, to nearest even, as it
// is staged into LDS; the filter is rounded once by the pack kernel, which reads the fp32 parameter in place (either
// layout, a channel slice of a wider one) and writes the image the main kernel copies into LDS unchanged.  A
// product of two bf16 values is exact in fp32, so gx is an fp32 sum of exact products in a fixed order: k-tiles of
// KT = 16 output channels in turn (one k-step of v_mfma_f32_32x32x16_bf16), in a k-tile the nine taps (ky, kx) in
// turn.  No atomics: the same inputs give the same bits.
//
// The packed filter is [k-tile][tap = ky 3 + kx][co chunk of 8][ci, padded to a multiple of CB][8 co] bf16: the
// flip is the patch offset (2 - ky, 2 - kx) the multiplying waves read g_z at, the transpose is the order of the
// image -- indices, not copies.  Channels past Cout in the last k-tile and past Cin in the last block are ZERO in the
// image, and the g_z of a channel past Cout is replaced by zero when it is stored (its load re-reads the last real
// channel, which may hold anything): the tail of the reduction contributes exactly nothing.
//
// A workgroup owns CB = 64 input channels x a 16 x 16 pixel tile of one image.  LDS holds, per k-tile, the g_z
// patch with its halo as [co chunk][18 x 18 pixels][8 co] and the filter slice as [tap][co chunk][64 ci][8 co]: the
// lane of k half h of an MFMA reads its eight k values as one 16-byte word of either image (A = filter: row ci,
// B = g_z: column pixel).  Wave w of the four multiplying waves owns tile rows 4w .. 4w + 3 as two 32-pixel column
// blocks and both 32-channel row blocks: four accumulators, four fragment reads per four MFMAs.
// As in conv_wgrad_bf16.hip the workgroup has eight waves, two per SIMD: waves 0-3 multiply k-tile t out of one LDS
// image while waves 4-7 load k-tile t + 1 into registers (consecutive lanes load consecutive patch pixels of a
// channel plane; 16-byte loads of the packed filter), round it and store it into the other image; one barrier per
// k-tile.  Every load is at a clamped, always valid address; zeros are selected when the value is stored.
// The two images of a k-tile take 57.6 KB of LDS and a wave at most 128 registers, so two workgroups share a CU:
// one's staging latency and epilogue run under the other's MFMAs (with one 32-channel k-tile image per CU the
// 64-channel layers at 422 x 422, two k-tiles per workgroup, ran slower than their fp32 launch).
// The epilogue writes gx, adds what gx held (accumulate) and applies the gate (gx * [gate > 0], relu'(0) = 0), in
// that order.
#include "mma16_common.h"

namespace {

constexpr int TH = 16, TW = 16;                          // output pixel tile
constexpr int PH = TH + 2, PW = TW + 2, NPIX = PH * PW;  // its g_z patch
constexpr int CB = 64;                                   // input channels (rows of the product) of a workgroup
constexpr int KT = 16, NCHUNK = KT / 8;                  // output channels of a k-tile, in chunks of 8
constexpr int GN = (NPIX + 63) / 64;                     // patch pixels a staging lane holds: lane + 64 j
constexpr int GS_WORDS = NCHUNK * NPIX;                  // 16-byte words of a g_z image
constexpr int WS_WORDS = 9 * NCHUNK * CB;                // 16-byte words of a filter image
constexpr int WSLICES = 9 * NCHUNK;                      // [tap][chunk] slices of CB words (1 KiB) of a filter image
constexpr int WN = (WSLICES + 3) / 4;                    // ... a staging wave copies: slices sw, sw + 4, ...
static_assert(CB == 64 && NCHUNK == 2 && GN % 2 == 0 && KT % 16 == 0, "the staging waves' split of an image");

struct cd_params {
    int B, Cin, Cout, H, W;
    int cin_pad;                   // Cin rounded up to CB
    int nkt;                       // k-tiles
    int tilesX, tilesY;
    int ci0, accumulate;
    long long so, sc;
};

// The packed filter: element e of [k-tile][tap][chunk][cin_pad][8].
__global__ __launch_bounds__(256) void conv_dgrad_bf16_pack_kernel(cd_params p, const float* __restrict__ Wp,
                                                                   unsigned short* __restrict__ packed, long long n) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int j = (int)(e & 7);
    long long r = e >> 3;
    const int ci = (int)(r % p.cin_pad);
    r /= p.cin_pad;
    const int chunk = (int)(r % NCHUNK);
    r /= NCHUNK;
    const int tap = (int)(r % 9), kt = (int)(r / 9);
    const int co = kt * KT + chunk * 8 + j;
    float v = 0.f;
    if (co < p.Cout && ci < p.Cin) v = Wp[(long long)co * p.so + (long long)(p.ci0 + ci) * p.sc + tap];
    packed[e] = (unsigned short)to_bf16(v);
}

__global__ __launch_bounds__(512, 4) void conv_dgrad_bf16_kernel(cd_params p, const float* __restrict__ gz,
                                                                 const u32x4* __restrict__ packed,
                                                                 const float* __restrict__ gate, float* __restrict__ gx) {
    __shared__ __attribute__((aligned(16))) u32x4 lds[2][GS_WORDS + WS_WORDS];   // per image: g_z, then the filter
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), sw = wave & 3;
    const bool stager = wave >= 4;
    // Workgroup -> (pixel tile, channel block).  Workgroups are dealt to the eight XCDs in turn, each with an L2 of
    // its own: the remap hands every XCD one contiguous run of the sequence [tile][channel block], so that the
    // channel blocks of a tile (the same g_z patch) and neighbouring tiles (its halo, the other halves of its
    // 128-byte lines) meet in one L2.  A bijection of [0, gridDim.x) for any grid size; placement changes speed only.
    const unsigned nwg = gridDim.x, q = nwg >> 3, r = nwg & 7, xcd = blockIdx.x & 7;
    const unsigned wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (blockIdx.x >> 3);
    const int nblk = p.cin_pad / CB, tile = (int)(wg / (unsigned)nblk);
    const int per_img = p.tilesY * p.tilesX;
    const int b = tile / per_img, rem = tile % per_img;
    const int y0 = (rem / p.tilesX) * TH, x0 = (rem % p.tilesX) * TW;
    const int cb0 = (int)(wg % (unsigned)nblk) * CB;
    const size_t plane = (size_t)p.H * p.W;

    // The two roles are two code paths with the same barriers, one before the first k-tile and one per k-tile.
    if (stager) {
        // Wave sw stages co chunk sw & 1 of the patch (8 channels: one 16-byte word per pixel) for the patch pixels
        // lane + 64 (2 j + (sw >> 1)): plane offsets clamped into the map, and whether the pixel is real
        const int chunk = sw & 1, pass0 = sw >> 1;
        constexpr int GH = GN / 2;
        unsigned go[GH];
        bool gin[GH];
#pragma unroll
        for (int j = 0; j < GH; ++j) {
            const int k = min(lane + 64 * (2 * j + pass0), NPIX - 1), y = y0 - 1 + k / PW, x = x0 - 1 + k % PW;
            gin[j] = y >= 0 && y < p.H && x >= 0 && x < p.W;
            go[j] = 4u * (unsigned)(min(max(y, 0), p.H - 1) * p.W + min(max(x, 0), p.W - 1));
        }
        const float* gimg = gz + (size_t)b * p.Cout * plane;
        // One k-tile: every load first, then the rounding and the LDS stores.  Of the filter a wave copies every
        // fourth 1 KiB [tap][chunk] slice (the last pass of the waves without one loads the last slice again and
        // stores nothing).
        auto stage = [&](int kt, int buf) {
            float gv[8][GH];
            u32x4 wv[WN];
            const int c0 = kt * KT + chunk * 8;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const char* g = reinterpret_cast<const char*>(gimg + (size_t)min(c0 + i, p.Cout - 1) * plane);
#pragma unroll
                for (int j = 0; j < GH; ++j) gv[i][j] = *reinterpret_cast<const float*>(g + go[j]);
            }
            const u32x4* wsrc = packed + (size_t)kt * 9 * NCHUNK * p.cin_pad + cb0 + lane;
#pragma unroll
            for (int i = 0; i < WN; ++i) wv[i] = wsrc[(size_t)min(4 * i + sw, WSLICES - 1) * p.cin_pad];
            u32x4* gs = lds[buf];
            u32x4* ws = lds[buf] + GS_WORDS;
#pragma unroll
            for (int j = 0; j < GH; ++j) {
                float v[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = gin[j] && c0 + i < p.Cout ? gv[i][j] : 0.f;
                u32x4 w;                                                 // (not pack8(v): the call allocates registers differently)
                w.x = pack2(v[0], v[1]); w.y = pack2(v[2], v[3]); w.z = pack2(v[4], v[5]); w.w = pack2(v[6], v[7]);
                const int k = lane + 64 * (2 * j + pass0);
                if (k < NPIX) gs[chunk * NPIX + k] = w;
            }
#pragma unroll
            for (int i = 0; i < WN; ++i)
                if (4 * i + sw < WSLICES) ws[(4 * i + sw) * CB + lane] = wv[i];
        };
        stage(0, 0);
        __syncthreads();
        int buf = 0;
        for (int kt = 0; kt < p.nkt; ++kt, buf ^= 1) {
            if (kt + 1 < p.nkt) stage(kt + 1, buf ^ 1);
            __syncthreads();                                             // image buf is read, image buf ^ 1 written
        }
        return;
    }

    // wave sw -> tile rows 4 sw .. 4 sw + 3; lane -> (row / pixel within a 32 block, k half)
    const int l31 = lane & 31, half = lane >> 5;
    // B: pixel (row 4 sw + 2 n + (l31 >> 4), column l31 & 15) of column block n, before the tap's offset
    const int gb_off = half * NPIX + (4 * sw + (l31 >> 4)) * PW + (l31 & 15);
    const int wa_off = half * CB + l31;                                  // A: channel l31 of row block 0
    f32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;
    __syncthreads();
    int buf = 0;
    for (int kt = 0; kt < p.nkt; ++kt, buf ^= 1) {
        const u32x4* gs = lds[buf] + gb_off;
        const u32x4* ws = lds[buf] + GS_WORDS + wa_off;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int dy = 2 - tap / 3, dx = 2 - tap % 3;                // the flip
#pragma unroll
            for (int s = 0; s < KT / 16; ++s) {                          // k-step: chunks 2 s, 2 s + 1
                const bf16x8 a0 = __builtin_bit_cast(bf16x8, ws[(tap * NCHUNK + 2 * s) * CB]);
                const bf16x8 a1 = __builtin_bit_cast(bf16x8, ws[(tap * NCHUNK + 2 * s) * CB + 32]);
                const bf16x8 b0 = __builtin_bit_cast(bf16x8, gs[2 * s * NPIX + dy * PW + dx]);
                const bf16x8 b1 = __builtin_bit_cast(bf16x8, gs[2 * s * NPIX + (dy + 2) * PW + dx]);
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0][0], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc[1][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // ---- epilogue: gx (+ what it held) (gated) ----
    const int x = x0 + (l31 & 15);
    if (x >= p.W) return;
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int y = y0 + 4 * sw + 2 * n + (l31 >> 4);
        if (y >= p.H) continue;
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ci = cb0 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (ci >= p.Cin) continue;
                const size_t o = (((size_t)b * p.Cin + ci) * p.H + y) * p.W + x;
                float v = acc[m][n][r];
                if (p.accumulate) v += gx[o];
                if (gate) v = gate[o] > 0.f ? v : 0.f;
                gx[o] = v;
            }
    }
}

// ---- host side ----
int cd_plan(const iiseg_conv_dgrad_desc* d, cd_params& p) {
    if (!d) return IISEG_ERR_NULL;
    if (d->K != 3 || d->pad != 1) return IISEG_ERR_SHAPE;
    if (d->B < 1 || d->B > 65535 || d->Cin < 1 || d->Cin > 65535 || d->Cout < 1 || d->Cout > 65535 || d->H < 1 ||
        d->W < 1 || (int64_t)d->H * d->W > (int64_t)1 << 28)
        return IISEG_ERR_SHAPE;
    if (!param_layout_ok(d->so, d->sc, d->ci0, d->Cin, d->Cin_tot, d->Cout, 9)) return IISEG_ERR_SHAPE;
    if (d->accumulate != 0 && d->accumulate != 1) return IISEG_ERR_SHAPE;
    p.B = d->B; p.Cin = d->Cin; p.Cout = d->Cout; p.H = d->H; p.W = d->W;
    p.cin_pad = (d->Cin + CB - 1) / CB * CB;
    p.nkt = (d->Cout + KT - 1) / KT;
    p.tilesY = (d->H + TH - 1) / TH;
    p.tilesX = (d->W + TW - 1) / TW;
    if ((int64_t)d->B * p.tilesY * p.tilesX * (p.cin_pad / CB) > ((int64_t)1 << 31) - 1) return IISEG_ERR_SHAPE;
    p.ci0 = d->ci0; p.accumulate = d->accumulate;
    p.so = d->so; p.sc = d->sc;
    return IISEG_OK;
}

int64_t cd_pack_elems(const cd_params& p) { return (int64_t)p.nkt * 9 * KT * p.cin_pad; }

}  // namespace

extern "C" int iiseg_conv_dgrad_bf16_check(const iiseg_conv_dgrad_desc* d) {
    cd_params p;
    return cd_plan(d, p);
}
extern "C" int64_t iiseg_conv_dgrad_bf16_pack_elems(const iiseg_conv_dgrad_desc* d) {
    cd_params p;
    if (int st = cd_plan(d, p)) return st;
    return cd_pack_elems(p);
}
extern "C" int iiseg_conv_dgrad_bf16_pack(void* stream, const iiseg_conv_dgrad_desc* d, const float* W, void* packed) {
    cd_params p;
    if (int st = cd_plan(d, p)) return st;
    if (!W || !packed) return IISEG_ERR_NULL;
    if ((uintptr_t)W % 4 || (uintptr_t)packed % 16) return IISEG_ERR_ALIGN;
    const int64_t n = cd_pack_elems(p);
    if (ranges_overlap(W, (int64_t)d->Cout * d->Cin_tot * 9 * 4, packed, n * 2)) return IISEG_ERR_UNSUPPORTED;
    IISEG_LAUNCH(conv_dgrad_bf16_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p,
                 W, (unsigned short*)packed, (long long)n);
    return iiseg_check_launch();
}
extern "C" int iiseg_conv_dgrad_bf16(void* stream, const iiseg_conv_dgrad_desc* d, const float* gz, const void* packed,
                                     const float* gate, float* gx) {
    cd_params p;
    if (int st = cd_plan(d, p)) return st;
    if (!gz || !packed || !gx) return IISEG_ERR_NULL;
    if ((uintptr_t)gz % 4 || (uintptr_t)gx % 4 || (uintptr_t)gate % 4 || (uintptr_t)packed % 16) return IISEG_ERR_ALIGN;
    const int64_t plane = (int64_t)d->H * d->W, gzb = (int64_t)d->B * d->Cout * plane * 4,
                  gxb = (int64_t)d->B * d->Cin * plane * 4;
    // gx is written while other workgroups still read g_z and the filter image
    if (ranges_overlap(gx, gxb, gz, gzb) || ranges_overlap(gx, gxb, packed, cd_pack_elems(p) * 2)) return IISEG_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)(p.B * p.tilesY * p.tilesX * (p.cin_pad / CB)));
    IISEG_LAUNCH(conv_dgrad_bf16_kernel, grid, dim3(512), 0, (hipStream_t)stream, p, gz,
                 reinterpret_cast<const u32x4*>(packed), gate, gx);
    return iiseg_check_launch();
}
