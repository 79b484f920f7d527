// What the kernels of the 16-bit matrix pipe share (conv_wgrad_bf16.hip, conv_dgrad_bf16.hip, conv_kxk_bf16.hip,
// deconv_grad_bf16.hip, bnrelu_conv_bf16.hip) and, on the host side, the plans of every split reduction (those five,
// and conv_wgrad.hip -- through conv_wgrad_common.h, as conv_wgrad_bf16.hip -- and conv_wgrad_kxk.hip): the MFMA
// operand types, the fp32 -> bf16 packing, the operand of "the same pixels, one further", the parameter-layout check,
// the slab split, the overlap test and the K = 1 .. 7 launch ladder.
#pragma once
#include <type_traits>
#include "common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// fp32 -> bf16 (round to nearest even)
__device__ __forceinline__ unsigned to_bf16(float a) {
    return __builtin_bit_cast(unsigned short, static_cast<__bf16>(a));
}
__device__ __forceinline__ unsigned pack2(float lo, float hi) { return to_bf16(lo) | (to_bf16(hi) << 16); }
__device__ __forceinline__ u32x4 pack8(const float* v) {
    u32x4 w;
    w.x = pack2(v[0], v[1]); w.y = pack2(v[2], v[3]); w.z = pack2(v[4], v[5]); w.w = pack2(v[6], v[7]);
    return w;
}

// An MFMA operand of 8 bf16 from four dwords ...
__device__ __forceinline__ bf16x8 frag(unsigned a, unsigned b, unsigned c, unsigned d) {
    u32x4 v;
    v.x = a; v.y = b; v.z = c; v.w = d;
    return __builtin_bit_cast(bf16x8, v);
}
// ... and the one of pixels 1 .. 8 of the ten in five dwords: the run shifted by one element (v_alignbyte)
__device__ __forceinline__ bf16x8 frag_shift1(unsigned d0, unsigned d1, unsigned d2, unsigned d3, unsigned d4) {
    return frag(__builtin_amdgcn_alignbyte(d1, d0, 2), __builtin_amdgcn_alignbyte(d2, d1, 2),
                __builtin_amdgcn_alignbyte(d3, d2, 2), __builtin_amdgcn_alignbyte(d4, d3, 2));
}

// ---- host side ----
inline bool ranges_overlap(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)bbytes && b0 < a0 + (uintptr_t)abytes;
}

// The parameter array of a layer with KK taps: Cin_tot input channels, this call's at [ci0, ci0 + Cin); 'oihw' or
// 'iohw' strides; fewer than 2^31 elements.
inline bool param_layout_ok(int64_t so, int64_t sc, int ci0, int Cin, int Cin_tot, int Cout, int KK) {
    if (ci0 < 0 || Cin_tot < 1 || Cin_tot > 65535 || (int64_t)ci0 + Cin > Cin_tot) return false;
    if (!((so == (int64_t)Cin_tot * KK && sc == KK) || (so == KK && sc == (int64_t)Cout * KK))) return false;
    return (int64_t)Cout * Cin_tot * KK <= ((int64_t)1 << 31) - 1;
}

// Cut a reduction of `units` steps into slabs: as many as bring a launch of `base_workgroups` (without a split) to
// `target_workgroups`, of at least `min_per_slab` units each.
inline void split_slabs(int64_t units, int64_t base_workgroups, int64_t target_workgroups, int64_t min_per_slab,
                        int64_t* per_slab, int* nslab) {
    const int64_t target =
        base_workgroups >= target_workgroups ? 1 : (target_workgroups + base_workgroups - 1) / base_workgroups;
    int64_t n = (units + target - 1) / target;
    if (n < min_per_slab) n = min_per_slab;
    *per_slab = n;
    *nslab = (int)((units + n - 1) / n);
}

// f(std::integral_constant<int, K>) for the K of a 'valid' K x K layer, 1 <= K <= 7 (checked by the plans)
template <typename F>
inline void dispatch_k(int K, F&& f) {
    switch (K) {
        case 1: f(std::integral_constant<int, 1>()); break;
        case 2: f(std::integral_constant<int, 2>()); break;
        case 3: f(std::integral_constant<int, 3>()); break;
        case 4: f(std::integral_constant<int, 4>()); break;
        case 5: f(std::integral_constant<int, 5>()); break;
        case 6: f(std::integral_constant<int, 6>()); break;
        default: f(std::integral_constant<int, 7>()); break;
    }
}

}  // namespace
