// The training forward of FC-DenseNet's dense-block layer as ONE launch on the 16-bit matrix pipe
// (ops.bnrelu_conv_fwd, FCDenseNet(fwd='bf16')).  For a stack x (B, cap, H, W) fp32 of which
// channels [0, n) are read and the layer's own fp32 parameter W[Cout][n][3][3] ('oihw', read as it is: no packed
// copy that could go stale):
//
//   y = (x - mean[c]) * (gamma[c] * inv_std[c]) + beta[c]          (bn_relu_kernel's expression, fp32)
//   t = max(y, 0) inside the map, exactly 0 on the padding ring     (zeros of t, not BN(0))
//   z[b][co][i][j] = (sum_{c<n,ky,kx} bf16(W[co][c][ky][kx]) * bf16(tpad[b][c][i + ky][j + kx]) + bias[co])
//                    * keep[b][co][i][j] * s,      s = 1 / (1 - p) in fp32  (scale_mask_kernel's expression)
//
// into channels [out_c0, out_c0 + Cout) of a (B, out_cap, H, W) tensor -- which may be the stack itself, behind the
// channels that are read.  Every operand is rounded once, to nearest even, as it is staged; fp32 accumulation in a
// fixed order by v_mfma_f32_16x16x32_bf16; no atomics.
//
// A workgroup of four waves owns an 8 x 32 pixel tile of one image, 16 output channels and a slab of 32-channel
// k-tiles.  LDS holds t channel-innermost: [8-channel chunk (4)][patch row (10)][patch column (34)][8 bf16], so the B
// operand of one MFMA (k = 8 channels x 4 chunks at one tap, column = 16 pixels of a tile row) is ONE 16-byte read
// per lane at the tap's offset; and W as [tap (9)][chunk (4)][co (16)][8 bf16], the A operand one 16-byte read.
// C: row co = 4 (lane >> 4) + reg, column pixel = lane & 15.  Wave w multiplies tile rows 2 w and 2 w + 1 (four
// 16-pixel segments, four accumulators; a segment outside the map is skipped) and stages chunk w of the next
// k-tile: a lane gathers the 8 channel planes at one patch pixel -- 48 loads, coalesced along pixels, every one at
// a clamped, always valid address -- with the BatchNorm vectors of its 8 channels wave-uniform.  The kernel is bound
// by those loads, not by its 36 MFMAs per wave and k-tile: they are issued in one piece before the products of the
// k-tile before them, and normalised, rectified, rounded and stored afterwards.  There is ONE LDS image (NBUF = 1,
// 30 KiB, two barriers per k-tile: read, then written) and the kernel keeps to 128 registers, so that four
// workgroups share a CU and the loads of one cover the products of another: measured against two images and one
// barrier (NBUF = 2, 61 KiB, two workgroups per CU) the 224 x 224 layers of a DenseNet103 step take 0.53 instead of
// 0.70 ms at batch 3 and 1.34 instead of 1.65 ms at batch 10, and no resolution is slower.
//
// Small maps split the reduction over input channels: slab s of k-tiles goes to slab s of a workspace
// [slab][B][Cout][H][W]; a second launch adds the slabs in slab order, then bias, mask and scale.  The slab rule
// depends on (n, Cout, H, W) only, never on B, so an element's bits do not depend on the batch it is in.
#include "mma16_common.h"

namespace {

constexpr int TH = 8, TW = 32;                     // output pixel tile
constexpr int PH = TH + 2, PW = TW + 2;            // its patch of t
constexpr int PPIX = PH * PW;                      // 340 patch pixels
constexpr int CO = 16;                             // output channels per workgroup
constexpr int KC = 32, NCHUNK = KC / 8;            // channels per k-tile: four chunks of 8
constexpr int NT = 256, NWAVE = NT / 64;
constexpr int XN = (PPIX + 63) / 64;               // patch pixels per lane and chunk: lane + 64 j
constexpr int WROW = KC * 9;                       // parameter elements per output channel and k-tile
constexpr int WQ = CO * KC / NT;                   // (co, c) pairs per thread: nine taps each
constexpr int NBUF = 1;                            // LDS images of a k-tile (see above)
constexpr int TARGET_WORKGROUPS = 128;             // per image (the rule must not see B)
constexpr int MIN_KT_PER_SLAB = 2;
static_assert(NWAVE == NCHUNK && TH == 2 * NWAVE && TW == 32 && CO * KC % NT == 0 && NT % KC == 0, "the lane maps below");

struct bc_params {
    int B, n, cap, Cout, H, W, out_cap, out_c0;
    int tilesX, per_img, KT, kps, nslab;
    int has_keep;
    float scale;
};

__global__ __launch_bounds__(NT, NBUF == 1 ? 4 : 2) void bnrelu_conv_bf16_kernel(bc_params p, const float* __restrict__ x,
                                                                 const float* __restrict__ beta,
                                                                 const float* __restrict__ gamma,
                                                                 const float* __restrict__ mean,
                                                                 const float* __restrict__ inv_std,
                                                                 const float* __restrict__ Wp,
                                                                 const float* __restrict__ bias,
                                                                 const float* __restrict__ keep, float* dst) {
    __shared__ __attribute__((aligned(16))) unsigned short ts[NBUF][NCHUNK * PPIX * 8];
    __shared__ __attribute__((aligned(16))) unsigned short wsm[NBUF][9 * NCHUNK * CO * 8];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x / p.per_img, rem = blockIdx.x % p.per_img;
    const int y0 = (rem / p.tilesX) * TH, x0 = (rem % p.tilesX) * TW;
    const int co0 = blockIdx.y * CO, slab = blockIdx.z;
    const int kt0 = slab * p.kps, kt1 = min(p.KT, kt0 + p.kps);
    const size_t HW = (size_t)p.H * p.W;
    const float* xim = x + (size_t)b * p.cap * HW;

    // what a lane stages of a k-tile: patch pixels lane + 64 j of its wave's chunk ...
    unsigned xo[XN];                               // byte offset in a plane (a plane is < 2^30 bytes)
    bool xin[XN];
#pragma unroll
    for (int j = 0; j < XN; ++j) {
        const int k = min(lane + 64 * j, PPIX - 1);
        const int iy = y0 - 1 + k / PW, ix = x0 - 1 + k % PW;
        xin[j] = iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
        xo[j] = 4u * (unsigned)(min(max(iy, 0), p.H - 1) * p.W + min(max(ix, 0), p.W - 1));
    }
    // ... and the nine taps of the (co, c) pairs tid + 256 q of the [16 co][32 c] block of the parameter
    const int wc = tid & (KC - 1);
    // (formed again where they are used, not held in registers: the kernel runs four waves per SIMD at 128)
    auto wco = [&](int q) __attribute__((always_inline)) { return (tid >> 5) + (NT / KC) * q; };
    auto wok = [&](int kt, int q) __attribute__((always_inline)) {
        return co0 + wco(q) < p.Cout && kt * KC + wc < p.n;
    };
    float xv[8][XN], wv[WQ][9];
    auto load = [&](int kt) __attribute__((always_inline)) {
        const int c0 = kt * KC + 8 * wave;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const char* pl = reinterpret_cast<const char*>(xim + (size_t)min(c0 + i, p.n - 1) * HW);
#pragma unroll
            for (int j = 0; j < XN; ++j) xv[i][j] = *reinterpret_cast<const float*>(pl + xo[j]);
        }
#pragma unroll
        for (int q = 0; q < WQ; ++q) {
            // (element offset of the pair: Cout n 9 < 2^31)
            const float* wp = Wp + (wok(kt, q) ? (unsigned)((co0 + wco(q)) * p.n + kt * KC + wc) * 9u : 0u);
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) wv[q][tap] = wp[wok(kt, q) ? tap : 0];
        }
    };
    auto store = [&](int buf, int kt) __attribute__((always_inline)) {
        const int c0 = kt * KC + 8 * wave;
        float m[8], g[8], be[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c = min(c0 + i, p.n - 1);    // wave-uniform: scalar loads
            m[i] = mean[c];
            g[i] = gamma[c] * inv_std[c];
            be[i] = beta[c];
        }
#pragma unroll
        for (int j = 0; j < XN; ++j) {
            float t[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float v = (xv[i][j] - m[i]) * g[i] + be[i];      // (input - mean) * (gamma * inv_std) + beta
                const float r = v > 0.f ? v : 0.f;
                t[i] = xin[j] && c0 + i < p.n ? r : 0.f;               // the ring and the ragged k-tile: zeros of t
            }
            const int k = lane + 64 * j;
            if (k < PPIX) *reinterpret_cast<u32x4*>(&ts[buf][(wave * PPIX + k) * 8]) = pack8(t);
        }
#pragma unroll
        for (int q = 0; q < WQ; ++q) {
            const bool ok = wok(kt, q);
#pragma unroll
            for (int tap = 0; tap < 9; ++tap)
                wsm[buf][((wc >> 3) * CO + wco(q)) * 8 + (wc & 7) + tap * NCHUNK * CO * 8] = to_bf16(ok ? wv[q][tap] : 0.f);
        }
    };

    const int l15 = lane & 15, g4 = lane >> 4;
    bool seg_on[4];                                // wave-uniform
#pragma unroll
    for (int s = 0; s < 4; ++s) seg_on[s] = y0 + 2 * wave + (s >> 1) < p.H && x0 + 16 * (s & 1) < p.W;
    f32x4 acc[4];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[s][r] = 0.f;
    auto multiply = [&](int buf) __attribute__((always_inline)) {
        const unsigned short* wa = wsm[buf] + (g4 * CO + l15) * 8;
        const unsigned short* tb = ts[buf] + (g4 * PPIX + 2 * wave * PW + l15) * 8;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const bf16x8 a =
                __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(wa + tap * NCHUNK * CO * 8));
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if (!seg_on[s]) continue;
                const int off = ((s >> 1) + tap / 3) * PW + 16 * (s & 1) + tap % 3;
                const bf16x8 bv = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(tb + off * 8));
                acc[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bv, acc[s], 0, 0, 0);
            }
        }
    };

    if (kt0 < kt1) {
        load(kt0);
        store(0, kt0);
    }
    __syncthreads();
    int buf = 0;
    for (int kt = kt0; kt < kt1; ++kt) {
        const bool more = kt + 1 < kt1;            // block-uniform
        if (more) load(kt + 1);
        multiply(buf);
        if (NBUF == 1) __syncthreads();            // the one image is read ...
        else buf ^= 1;
        if (more) store(buf, kt + 1);
        __syncthreads();                           // ... and written (two images: one read, the other written)
    }

    // the tile: bias, mask and scale into z (one slab), or the bare sums into this slab of the workspace
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int y = y0 + 2 * wave + (s >> 1), xx = x0 + 16 * (s & 1) + l15;
        if (y >= p.H || xx >= p.W) continue;
        const size_t pix = (size_t)y * p.W + xx;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = co0 + 4 * g4 + r;
            if (co >= p.Cout) continue;
            if (p.nslab == 1) {
                float v = acc[s][r] + bias[co];
                if (p.has_keep) v = v * keep[((size_t)b * p.Cout + co) * HW + pix] * p.scale;
                dst[((size_t)b * p.out_cap + p.out_c0 + co) * HW + pix] = v;
            } else {
                dst[(((size_t)slab * p.B + b) * p.Cout + co) * HW + pix] = acc[s][r];
            }
        }
    }
}

// z = (slab 0 + slab 1 + ... + bias) * keep * s
__global__ __launch_bounds__(256) void bnrelu_conv_bf16_finalize_kernel(bc_params p, const float* __restrict__ ws,
                                                                        const float* __restrict__ bias,
                                                                        const float* __restrict__ keep,
                                                                        float* __restrict__ z) {
    const size_t HW = (size_t)p.H * p.W, per = (size_t)p.Cout * HW, total = (size_t)p.B * per;
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        float v = ws[i];
        for (int s = 1; s < p.nslab; ++s) v += ws[(size_t)s * total + i];
        const size_t b = i / per, r = i - b * per;
        v += bias[r / HW];
        if (p.has_keep) v = v * keep[i] * p.scale;
        z[(b * p.out_cap + p.out_c0) * HW + r] = v;
    }
}

// ---- host side ----
int bc_plan(const iiseg_bnrelu_conv_desc* d, bc_params& p) {
    if (!d) return IISEG_ERR_NULL;
    if (d->B < 1 || d->n < 1 || d->Cout < 1 || d->H < 1 || d->W < 1 || d->cap < d->n || d->out_c0 < 0 ||
        (int64_t)d->out_c0 + d->Cout > d->out_cap || d->B > 65535 || d->cap > 65535 || d->out_cap > 65535 ||
        (int64_t)d->H * d->W > ((int64_t)1 << 28) || (int64_t)d->Cout * d->n * 9 > ((int64_t)1 << 31) - 1)
        return IISEG_ERR_SHAPE;
    p.B = d->B; p.n = d->n; p.cap = d->cap; p.Cout = d->Cout; p.H = d->H; p.W = d->W;
    p.out_cap = d->out_cap; p.out_c0 = d->out_c0;
    p.tilesX = (d->W + TW - 1) / TW;
    p.per_img = p.tilesX * ((d->H + TH - 1) / TH);
    p.KT = (d->n + KC - 1) / KC;
    if ((int64_t)p.per_img * d->B > ((int64_t)1 << 31) - 1) return IISEG_ERR_SHAPE;
    int64_t kps;
    int nslab;
    split_slabs(p.KT, (int64_t)p.per_img * ((d->Cout + CO - 1) / CO), TARGET_WORKGROUPS, MIN_KT_PER_SLAB, &kps,
                &nslab);
    p.kps = (int)kps;
    p.nslab = nslab;
    p.has_keep = 0;
    p.scale = 1.f;
    return IISEG_OK;
}

}  // namespace

extern "C" int iiseg_bnrelu_conv_fwd_bf16_check(const iiseg_bnrelu_conv_desc* d) {
    bc_params p;
    return bc_plan(d, p);
}
extern "C" int iiseg_bnrelu_conv_fwd_bf16_slabs(const iiseg_bnrelu_conv_desc* d) {
    bc_params p;
    if (int st = bc_plan(d, p)) return st;
    return p.nslab;
}
extern "C" int64_t iiseg_bnrelu_conv_fwd_bf16_workspace_elems(const iiseg_bnrelu_conv_desc* d) {
    bc_params p;
    if (int st = bc_plan(d, p)) return st;
    return p.nslab == 1 ? 0 : (int64_t)p.nslab * d->B * d->Cout * d->H * d->W;
}
extern "C" int iiseg_bnrelu_conv_fwd_bf16(void* stream, const iiseg_bnrelu_conv_desc* d, const float* x,
                                          const float* beta, const float* gamma, const float* mean,
                                          const float* inv_std, const float* W, const float* bias, const float* keep,
                                          float p_drop, float* ws, float* z) {
    bc_params p;
    if (int st = bc_plan(d, p)) return st;
    if (!x || !beta || !gamma || !mean || !inv_std || !W || !bias || !z || (p.nslab > 1 && !ws))
        return IISEG_ERR_NULL;
    if (!(p_drop >= 0.f) || !(p_drop < 1.f)) return IISEG_ERR_SHAPE;
    const int64_t HW = (int64_t)p.H * p.W;
    const int64_t xbytes = 4 * ((int64_t)(p.B - 1) * p.cap + p.n) * HW;
    const int64_t zbytes = 4 * ((int64_t)(p.B - 1) * p.out_cap + p.out_c0 + p.Cout) * HW;
    const int64_t wsbytes = 4 * (int64_t)p.nslab * p.B * p.Cout * HW;
    // z inside the stack it reads: only the stack's own channels behind the n that are read
    if (ranges_overlap(x, xbytes, z, zbytes) && !(x == z && p.cap == p.out_cap && p.out_c0 >= p.n))
        return IISEG_ERR_UNSUPPORTED;
    if (ranges_overlap(W, 4 * (int64_t)p.Cout * p.n * 9, z, zbytes) ||
        (keep && ranges_overlap(keep, 4 * (int64_t)p.B * p.Cout * HW, z, zbytes)) ||
        (p.nslab > 1 && (ranges_overlap(ws, wsbytes, z, zbytes) || ranges_overlap(ws, wsbytes, x, xbytes))))
        return IISEG_ERR_UNSUPPORTED;
    p.has_keep = keep != nullptr;
    p.scale = 1.f / (1.f - p_drop);                // scale_mask_kernel's factor
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(p.per_img * p.B), (unsigned)((p.Cout + CO - 1) / CO), (unsigned)p.nslab);
    IISEG_LAUNCH(bnrelu_conv_bf16_kernel, grid, dim3(NT), 0, s, p, x, beta, gamma, mean, inv_std, W, bias, keep,
                 p.nslab == 1 ? z : ws);
    if (p.nslab > 1) {
        const int64_t total = (int64_t)p.B * p.Cout * HW;
        const int64_t g = (total + 255) / 256;
        IISEG_LAUNCH(bnrelu_conv_bf16_finalize_kernel, dim3((unsigned)(g > 16384 ? 16384 : g)), dim3(256), 0, s, p,
                     (const float*)ws, bias, keep, z);
    }
    return iiseg_check_launch();
}
