// True-gradient refinement on the standard DAE's bf16 C8 leg: the two element-wise adjoint
// kernels of the backward walk on C8 tensors (B, C/8, H, W, 8).  The convolutions of that walk are the forward's
// kernels (conv_c8_kernel / conv_c8_m16_kernel) on the flipped filters.
//
//   depool_bwd_c8_kernel   adjoint of DePool2D (layers/mylayers.py:88-115) under the level's mask bytes
//   relu_gate_c8_kernel    the ReLU half of max-pool + ReLU backward, at pooled resolution
//
// Both are grid-stride, one thread = one pooled element of one chunk (the shape of unpool_c8_kernel): 16-byte
// loads and stores, the 8 mask bytes of the element as one uint2.  No LDS, no atomics: every output is one
// fixed-order fp32 sum, rounded once (RNE) at its store.  The entry points (abi.hip) check every argument.
#include <stdint.h>
#include "common.h"
#include "conv_common.h"
#include "c8_common.h"

using iiseg::pack_bf16;

namespace {

__device__ __forceinline__ float bf_lo(uint32_t u) { return __builtin_bit_cast(float, u << 16); }
__device__ __forceinline__ float bf_hi(uint32_t u) { return __builtin_bit_cast(float, u & 0xffff0000u); }

// 0xffff in the halves of a bf16 pair whose value is > 0 (+0, -0, negative and NaN: 0)
__device__ __forceinline__ uint32_t positive_halves(uint32_t p) {
    return (bf_lo(p) > 0.f ? 0x0000ffffu : 0u) | (bf_hi(p) > 0.f ? 0xffff0000u : 0u);
}

// g_f[q] = sum over k = 0..3 with bit k of mask[q] set of g_u[2 qy + (k >> 1)][2 qx + (k & 1)], for the pooled
// window (y0, x0, wh, ww) of the (h2, w2) planes; g_u planes are (PH, PW) with PH >= 2 h2, PW >= 2 w2 (the unpaired
// last row / column of an odd map is never read).  The sum runs in fp32 from +0 in the order k = 0, 1, 2, 3: a
// position the mask leaves out contributes nothing (it is not multiplied by zero -- whatever it holds stays
// out).  GATE: the result of a channel is +0 where gate[q] <= 0 (-0 included): the ReLU mask of the stage that
// follows at the deepest level.
template <bool GATE>
__global__ __launch_bounds__(256) void depool_bwd_c8_kernel(const uint4* __restrict__ gu,
                                                            const uint2* __restrict__ mask,
                                                            const uint4* __restrict__ gate, uint4* __restrict__ out,
                                                            int PH, int PW, int h2, int w2, int y0, int x0, int wh,
                                                            int ww, int64_t total) {
    for (int64_t t = blockIdx.x * (int64_t)256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int qx = x0 + (int)(t % ww);
        int64_t r = t / ww;
        const int qy = y0 + (int)(r % wh);
        r /= wh;                                    // b * C8n + c8
        const int64_t pi = (r * h2 + qy) * w2 + qx;
        const uint2 m = mask[pi];
        const uint4* s = gu + (r * PH + 2 * qy) * PW + 2 * qx;
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint4 u = s[(int64_t)(k >> 1) * PW + (k & 1)];
            const float v[8] = {bf_lo(u.x), bf_hi(u.x), bf_lo(u.y), bf_hi(u.y),
                                bf_lo(u.z), bf_hi(u.z), bf_lo(u.w), bf_hi(u.w)};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const unsigned byte = ((j < 4 ? m.x : m.y) >> (8 * (j & 3))) & 0xffu;
                if ((byte >> k) & 1u) acc[j] += v[j];
            }
        }
        uint4 o = make_uint4(pack_bf16(acc[0], acc[1]), pack_bf16(acc[2], acc[3]), pack_bf16(acc[4], acc[5]),
                             pack_bf16(acc[6], acc[7]));
        if constexpr (GATE) {
            const uint4 p = gate[pi];
            o.x &= positive_halves(p.x); o.y &= positive_halves(p.y);
            o.z &= positive_halves(p.z); o.w &= positive_halves(p.w);
        }
        out[pi] = o;
    }
}

// out = g where pooled > 0, else +0 (relu'(0) = 0), element-wise on the pooled window; g's bits pass unchanged.
// `out` may be `g` itself (no __restrict__ on the two: a thread reads its element before it writes it).
__global__ __launch_bounds__(256) void relu_gate_c8_kernel(const uint4* g, const uint4* __restrict__ pooled,
                                                           uint4* out, int h2, int w2, int y0, int x0, int wh,
                                                           int ww, int64_t total) {
    for (int64_t t = blockIdx.x * (int64_t)256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int qx = x0 + (int)(t % ww);
        int64_t r = t / ww;
        const int qy = y0 + (int)(r % wh);
        r /= wh;
        const int64_t pi = (r * h2 + qy) * w2 + qx;
        uint4 o = g[pi];
        const uint4 p = pooled[pi];
        o.x &= positive_halves(p.x); o.y &= positive_halves(p.y);
        o.z &= positive_halves(p.z); o.w &= positive_halves(p.w);
        out[pi] = o;
    }
}

inline int grid_for(int64_t total) {
    const int64_t blocks = (total + 255) / 256;
    return (int)(blocks < 65536 ? blocks : 65536);
}

}  // namespace

namespace iiseg {

int depool_bwd_c8_launch(void* stream, const void* gu, const uint8_t* mask, const void* gate, void* out,
                         int64_t BC8, int PH, int PW, int h2, int w2, int y0, int x0, int wh, int ww) {
    const int64_t total = BC8 * wh * ww;
    if (gate)
        IISEG_LAUNCH(depool_bwd_c8_kernel<true>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream,
                     (const uint4*)gu, (const uint2*)mask, (const uint4*)gate, (uint4*)out, PH, PW, h2, w2, y0, x0,
                     wh, ww, total);
    else
        IISEG_LAUNCH(depool_bwd_c8_kernel<false>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream,
                     (const uint4*)gu, (const uint2*)mask, (const uint4*)nullptr, (uint4*)out, PH, PW, h2, w2, y0,
                     x0, wh, ww, total);
    return iiseg_check_launch();
}

int relu_gate_c8_launch(void* stream, const void* g, const void* pooled, void* out, int64_t BC8, int h2, int w2,
                        int y0, int x0, int wh, int ww) {
    const int64_t total = BC8 * wh * ww;
    IISEG_LAUNCH(relu_gate_c8_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const uint4*)g,
                 (const uint4*)pooled, (uint4*)out, h2, w2, y0, x0, wh, ww, total);
    return iiseg_check_launch();
}

}  // namespace iiseg
