// 'valid' K x K convolution (K = 1 or 3) with a DILATION d in {1, 2, 4, 8, 16} between at most 16 channels on
// bf16 C8 activations (gfx950, v_mfma_f32_16x16x32_bf16, fp32 accumulate): the 16-bit leg of the context-module
// DAE (models/contextmod_dae.py:74-105: conv 3x3, PadLayer(32), six dilated 3x3 layers, a 1x1 score layer, 11
// channels throughout).  conv_c8_m16.hip stages halo-1 LDS patches and cannot be stretched
// to d = 16 (a 16-row tile would stage a 48-row patch); here there is NO LDS:
//   * M = 16 output channels, N = 16 pixels along a row, K = 32 = two taps x 16 input channels per MFMA: tap
//     pairs (0,1) (2,3) (4,5) (6,7), then tap 8 with a zero second half -- 5 MFMAs per 16-pixel group (K = 1: one
//     MFMA with a zero second half);
//   * the B operand straight from global memory: in C8 the 8 consecutive k-values of a lane ARE one 16-byte
//     chunk entry.  Lane group lane / 16 selects (tap of the pair, chunk), lane % 16 the pixel: one
//     buffer_load_dwordx4 per lane and MFMA at the tap's dilated offset, sixteen lanes reading 256 contiguous
//     bytes of a row.  A tap is re-read by the eight other taps' loads from L1 / L2 (as conv_small.hip reads its
//     taps), never amplified by a halo;
//   * 'valid': no tap of an output pixel is out of range.  A row's last, partly filled 16-pixel group and a
//     block's rows past the map CLAMP their pixel / row for the loads (in range by construction) and switch
//     their stores off through the buffer descriptor (an out-of-range offset), not per element;
//   * the A operand: 5 x (16 x 32) bf16 images packed once by the host side (c8dil_pack_elem below, round to
//     nearest-even), loaded once per wave -- 5 x 4 registers for the kernel's life;
//   * a wave owns one 16-pixel column group and RB rows of it, RT rows per round: the RT x 5 loads (and the
//     addend's) are issued together, then the RT MFMA chains and epilogues run;
//   * epilogue, in this order, in fp32: + bias, + addend (an fp32 NCHW map: the cached image half of conv1),
//     ReLU, store -- bf16 C8 (round to nearest-even; lane group g holds channels 4 g .. 4 g + 3 of its pixel = 8
//     bytes of chunk g / 2; channels >= Cout come out as exact zeros: zero weight rows, no bias, no addend),
//     placed at an offset inside a larger buffer whose border is never touched, or fp32 NCHW.
// Every output is one fixed-order sum (the MFMA chain from zero in tap-pair order): results do not depend on
// the batch size, the block a pixel falls into, or the launch.  No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "iiseg.h"
#include "common.h"
#include "conv_common.h"

using namespace iiseg;

namespace {

constexpr unsigned OOB = 0x80000000u;   // beyond every descriptor here (one image of a tensor is < 2^31 bytes)
constexpr int RT = 4;                   // rows per round of a wave
constexpr int RB = 8;                   // rows per workgroup
constexpr int CGW = 4;                  // 16-pixel column groups per workgroup (one per wave)

// fp32 -> bf16, round to nearest-even (finite input; the layer objects refuse non-finite parameters)
__host__ __device__ inline uint16_t bf16_rne(float f) {
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// element idx of the packed A operand: [m][g][co][j] (see include/iiseg.h)
__host__ __device__ inline uint16_t c8dil_pack_elem(const float* W, int64_t so, int64_t sc, int Cin, int Cout,
                                                    int K, int idx) {
    const int j = idx & 7, co = (idx >> 3) & 15, g = (idx >> 7) & 3, m = idx >> 9;
    const int tap = 2 * m + (g >> 1), ci = 8 * (g & 1) + j;
    if (tap >= K * K || co >= Cout || ci >= Cin) return 0;
    return bf16_rne(W[co * so + ci * sc + tap]);
}

__global__ __launch_bounds__(256) void c8dil_pack_kernel(const float* __restrict__ W, int64_t so, int64_t sc,
                                                         int Cin, int Cout, int K, int n,
                                                         uint16_t* __restrict__ wpack) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < n) wpack[idx] = c8dil_pack_elem(W, so, sc, Cin, Cout, K, idx);
}

struct DilParams {
    const char* x;
    const uint4* wp;
    const float* bias;
    const float* add;
    char* out;
    int H, W, OH, OW, Cout, d;
    int out_H, out_W, out_y0, out_x0;
    int relu, ncb;
};

template <int K, bool OUTF32>
__global__ __launch_bounds__(256) void conv_c8_dil_kernel(const DilParams p) {
    constexpr int NM = K == 3 ? 5 : 1;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const int rb = (int)blockIdx.x / p.ncb, cb = (int)blockIdx.x - rb * p.ncb, b = blockIdx.y;
    const int ox0 = (cb * CGW + wave) * 16, oy0 = rb * RB;
    if (ox0 >= p.OW) return;            // (wave-uniform; the kernel has no barrier)

    // A: the packed images, one 16-byte entry per lane and tap pair, for the kernel's life
    bf16x8 a[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) a[m] = __builtin_bit_cast(bf16x8, p.wp[m * 64 + lane]);

    const int HW = p.H * p.W, OHW = p.OH * p.OW, OPL = p.out_H * p.out_W;
    const __amdgpu_buffer_rsrc_t r_x = mk_rsrc(p.x + (size_t)b * 2 * HW * 16, (unsigned)(2 * HW) * 16u);
    const __amdgpu_buffer_rsrc_t r_b = mk_rsrc(p.bias, p.bias ? (unsigned)p.Cout * 4u : 0u);
    const __amdgpu_buffer_rsrc_t r_a =
        mk_rsrc(p.add ? p.add + (size_t)b * p.Cout * OHW : nullptr, p.add ? (unsigned)(p.Cout * OHW) * 4u : 0u);
    const unsigned obytes = OUTF32 ? (unsigned)(p.Cout * OPL) * 4u : (unsigned)(2 * OPL) * 16u;
    const __amdgpu_buffer_rsrc_t r_o = mk_rsrc(p.out + (size_t)b * obytes, obytes);

    // this lane's pixel of the group (clamped for the loads) and its tap of every pair
    const bool pok = ox0 + l15 < p.OW;
    const int px = pok ? ox0 + l15 : p.OW - 1;
    unsigned voff[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) {
        const int tap = 2 * m + (g >> 1);
        const int ky = tap / 3, kx = tap - 3 * ky;      // (K = 1: tap 0 only)
        voff[m] = tap < K * K ? (unsigned)((g & 1) * HW + ky * p.d * p.W + kx * p.d + px) * 16u : OOB;
    }
    // bias of channels 4 g .. 4 g + 3 (beyond Cout: out of the descriptor's range, zeros)
    const f32x4 bv = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r_b, (int)(16u * (unsigned)g), 0, 0));

#pragma unroll 1
    for (int r0 = oy0; r0 < oy0 + RB && r0 < p.OH; r0 += RT) {
        u32x4 xb[RT][NM];
        f32x4 av[RT];
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const int row = min(r0 + r, p.OH - 1);
            const int so = (int)((unsigned)(row * p.W) * 16u);
#pragma unroll
            for (int m = 0; m < NM; ++m)
                xb[r][m] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r_x, (int)voff[m], so, 0));
            if (p.add) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int co = 4 * g + q;
                    av[r][q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                        r_a, (int)(co < p.Cout ? (unsigned)(co * OHW + row * p.OW + px) * 4u : OOB), 0, 0));
                }
            }
        }
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int m = 0; m < NM; ++m)
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[m], __builtin_bit_cast(bf16x8, xb[r][m]), acc, 0, 0, 0);
            // (the epilogue on four scalars, the ReLU as a select: with the vector's elements rectified in place
            // under a branch, hipcc stored element 0 four times in the fp32 form)
            float v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                v[q] = acc[q] + bv[q];
                if (p.add) v[q] += av[r][q];
                v[q] = p.relu ? fmaxf(v[q], 0.f) : v[q];
            }
            const bool ok = pok && r0 + r < p.OH;
            const unsigned opix = (unsigned)((p.out_y0 + r0 + r) * p.out_W + p.out_x0 + px);
            if constexpr (OUTF32) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int co = 4 * g + q;
                    __builtin_amdgcn_raw_buffer_store_b32(
                        __builtin_bit_cast(int, v[q]), r_o,
                        (int)((ok && co < p.Cout) ? 4u * ((unsigned)(co * OPL) + opix) : OOB), 0, 0);
                }
            } else {
                u32x2 w2;
                w2[0] = pack_bf16(v[0], v[1]);
                w2[1] = pack_bf16(v[2], v[3]);
                __builtin_amdgcn_raw_buffer_store_b64(
                    w2, r_o, (int)(ok ? ((unsigned)((g >> 1) * OPL) + opix) * 16u + 8u * (unsigned)(g & 1) : OOB), 0, 0);
            }
        }
    }
}

int c8dil_check(const iiseg_c8dil_desc* d) {
    if (!d) return IISEG_ERR_NULL;
    if (d->K != 1 && d->K != 3) return IISEG_ERR_UNSUPPORTED;
    if (d->dil != 1 && d->dil != 2 && d->dil != 4 && d->dil != 8 && d->dil != 16) return IISEG_ERR_UNSUPPORTED;
    if (d->Cin > 16 || d->Cout > 16) return IISEG_ERR_UNSUPPORTED;
    if (d->flags & ~(IISEG_CONV_RELU | IISEG_C8DIL_OUT_NCHW)) return IISEG_ERR_UNSUPPORTED;
    if (d->B <= 0 || d->Cin <= 0 || d->Cout <= 0 || d->H <= 0 || d->W <= 0) return IISEG_ERR_SHAPE;
    const int64_t halo = (int64_t)d->dil * (d->K - 1);
    if (d->H <= halo || d->W <= halo) return IISEG_ERR_SHAPE;
    const int OH = d->H - (int)halo, OW = d->W - (int)halo;
    if (d->out_H == 0) {
        if (d->out_W != 0 || d->out_y0 != 0 || d->out_x0 != 0) return IISEG_ERR_SHAPE;
    } else if (d->out_H < 0 || d->out_W <= 0 || d->out_y0 < 0 || d->out_x0 < 0 ||
               (int64_t)d->out_y0 + OH > d->out_H || (int64_t)d->out_x0 + OW > d->out_W) {
        return IISEG_ERR_SHAPE;         // the placement window does not fit
    }
    // one image of every tensor is addressed with 32-bit byte offsets; the batch is the grid's y dimension
    const int64_t opl = d->out_H ? (int64_t)d->out_H * d->out_W : (int64_t)OH * OW;
    if ((int64_t)d->H * d->W * 64 >= (1ll << 31) || opl * 64 >= (1ll << 31) || d->B > 65535)
        return IISEG_ERR_UNSUPPORTED;
    return IISEG_OK;
}

}  // namespace

extern "C" int iiseg_conv_c8_dil_check(const iiseg_c8dil_desc* d) { return c8dil_check(d); }

extern "C" int64_t iiseg_conv_c8_dil_pack_bytes(int32_t K) {
    if (K != 1 && K != 3) return IISEG_ERR_UNSUPPORTED;
    return (int64_t)(K == 3 ? 5 : 1) * 64 * 8 * 2;
}

extern "C" int iiseg_conv_c8_dil_pack_host(const iiseg_c8dil_desc* d, const float* W, int64_t so, int64_t sc,
                                           void* wpack) {
    const int st = c8dil_check(d);
    if (st) return st;
    if (!W || !wpack) return IISEG_ERR_NULL;
    if (so <= 0 || sc <= 0) return IISEG_ERR_SHAPE;
    const int n = (int)(iiseg_conv_c8_dil_pack_bytes(d->K) / 2);
    for (int i = 0; i < n; ++i) ((uint16_t*)wpack)[i] = c8dil_pack_elem(W, so, sc, d->Cin, d->Cout, d->K, i);
    return IISEG_OK;
}

extern "C" int iiseg_conv_c8_dil_pack(void* stream, const iiseg_c8dil_desc* d, const float* W, int64_t so,
                                      int64_t sc, void* wpack) {
    const int st = c8dil_check(d);
    if (st) return st;
    if (!W || !wpack) return IISEG_ERR_NULL;
    if (so <= 0 || sc <= 0) return IISEG_ERR_SHAPE;
    if ((uintptr_t)wpack & 15) return IISEG_ERR_ALIGN;
    const int n = (int)(iiseg_conv_c8_dil_pack_bytes(d->K) / 2);
    IISEG_LAUNCH(c8dil_pack_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, W, so, sc, d->Cin,
                 d->Cout, d->K, n, (uint16_t*)wpack);
    return iiseg_check_launch();
}

extern "C" int iiseg_conv_c8_dil(void* stream, const iiseg_c8dil_desc* d, const void* x8, const void* wpack,
                                 const float* bias, const float* addend, void* out) {
    const int st = c8dil_check(d);
    if (st) return st;
    if (!x8 || !wpack || !out) return IISEG_ERR_NULL;
    const bool f32 = (d->flags & IISEG_C8DIL_OUT_NCHW) != 0;
    if (((uintptr_t)x8 & 15) || ((uintptr_t)wpack & 15) || ((uintptr_t)out & (f32 ? 3 : 15)) ||
        ((uintptr_t)bias & 3) || ((uintptr_t)addend & 3))
        return IISEG_ERR_ALIGN;
    const int halo = d->dil * (d->K - 1);
    DilParams p = {};
    p.x = (const char*)x8; p.wp = (const uint4*)wpack; p.bias = bias; p.add = addend; p.out = (char*)out;
    p.H = d->H; p.W = d->W; p.OH = d->H - halo; p.OW = d->W - halo; p.Cout = d->Cout; p.d = d->dil;
    p.out_H = d->out_H ? d->out_H : p.OH;
    p.out_W = d->out_H ? d->out_W : p.OW;
    p.out_y0 = d->out_y0; p.out_x0 = d->out_x0;
    p.relu = (d->flags & IISEG_CONV_RELU) ? 1 : 0;
    p.ncb = (p.OW + 16 * CGW - 1) / (16 * CGW);
    const dim3 grid((unsigned)(p.ncb * ((p.OH + RB - 1) / RB)), (unsigned)d->B), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (d->K == 3) {
        if (f32) IISEG_LAUNCH((conv_c8_dil_kernel<3, true>), grid, block, 0, s, p);
        else IISEG_LAUNCH((conv_c8_dil_kernel<3, false>), grid, block, 0, s, p);
    } else {
        if (f32) IISEG_LAUNCH((conv_c8_dil_kernel<1, true>), grid, block, 0, s, p);
        else IISEG_LAUNCH((conv_c8_dil_kernel<1, false>), grid, block, 0, s, p);
    }
    return iiseg_check_launch();
}
