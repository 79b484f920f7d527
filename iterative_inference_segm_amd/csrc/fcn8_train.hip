// The two element-wise kernels of an FCN-8 training step:
//   relu_gate : dst = g * [out > 0]  (relu'(0) = 0) on NCHW maps, in place or not
//   l2_term   : the weight-decay term of lasagne's regularize_network_params(l2) over the weight arrays of the
//               flat parameter buffer (never the biases): g += 2 wd W, penalty = sum W^2 in double.  One launch
//               over the buffer -- L2_BLOCKS workgroups per weight range, the ranges in the kernel's arguments --
//               and a one-workgroup finalize that adds the partials in a fixed order.  No atomics.
#include "common.h"

namespace {

constexpr int L2_BLOCKS = 512;                           // two per CU: the largest range (fc6: 1e8) sets the pace
constexpr int L2_MAX_RANGES = IISEG_L2_MAX_RANGES;

struct l2_ranges {
    long long lo[L2_MAX_RANGES], hi[L2_MAX_RANGES];
};

template <typename T>
__global__ __launch_bounds__(256) void relu_gate_kernel(const T* __restrict__ g, const T* __restrict__ out, T* dst,
                                                        long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        dst[i] = out[i] > (T)0 ? g[i] : (T)0;
}

template <typename T>
__global__ __launch_bounds__(256) void l2_term_kernel(l2_ranges r, const T* __restrict__ p, T* __restrict__ g, T two_wd,
                                                      double* __restrict__ partial) {
    __shared__ double red[4];
    const long long lo = r.lo[blockIdx.y], hi = r.hi[blockIdx.y];
    double s = 0.0;
    for (long long i = lo + (long long)blockIdx.x * 256 + threadIdx.x; i < hi; i += (long long)L2_BLOCKS * 256) {
        const T w = p[i];
        g[i] = fma(two_wd, w, g[i]);
        s = fma((double)w, (double)w, s);
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.y * L2_BLOCKS + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void l2_term_finalize_kernel(const double* __restrict__ partial, int n,
                                                              double* __restrict__ penalty) {
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += partial[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) *penalty = ((red[0] + red[1]) + red[2]) + red[3];
}

template <typename T>
int relu_gate(void* stream, const T* g, const T* out, T* dst, int64_t n) {
    if (!g || !out || !dst) return IISEG_ERR_NULL;
    if (n <= 0) return IISEG_ERR_SHAPE;
    if (dst == out) return IISEG_ERR_UNSUPPORTED;                        // (dst == g is fine: element-wise)
    int64_t blocks = (n + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    IISEG_LAUNCH(relu_gate_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, g, out, dst,
                 (long long)n);
    return iiseg_check_launch();
}

template <typename T>
int l2_term(void* stream, const T* p, T* g, int64_t n, const int64_t* ranges, int32_t nranges, double weight_decay,
            double* partial, double* penalty) {
    if (!p || !g || !ranges || !partial || !penalty) return IISEG_ERR_NULL;
    if (n <= 0 || nranges < 1) return IISEG_ERR_SHAPE;
    if (nranges > L2_MAX_RANGES) return IISEG_ERR_UNSUPPORTED;
    l2_ranges r;
    int64_t prev = 0;
    for (int k = 0; k < nranges; ++k) {                                  // ascending, disjoint, inside the buffer
        const int64_t lo = ranges[2 * k], hi = ranges[2 * k + 1];
        if (lo < prev || hi <= lo || hi > n) return IISEG_ERR_SHAPE;
        r.lo[k] = lo; r.hi[k] = hi;
        prev = hi;
    }
    hipStream_t s = (hipStream_t)stream;
    IISEG_LAUNCH(l2_term_kernel<T>, dim3(L2_BLOCKS, (unsigned)nranges), dim3(256), 0, s, r, p, g,
                 (T)(2.0 * weight_decay), partial);
    IISEG_LAUNCH(l2_term_finalize_kernel, dim3(1), dim3(256), 0, s, (const double*)partial, nranges * L2_BLOCKS, penalty);
    return iiseg_check_launch();
}

}  // namespace

extern "C" int iiseg_l2_term_partials(int32_t nranges) {
    if (nranges < 1) return IISEG_ERR_SHAPE;
    if (nranges > L2_MAX_RANGES) return IISEG_ERR_UNSUPPORTED;
    return nranges * L2_BLOCKS;
}
extern "C" int iiseg_relu_gate_f32(void* stream, const float* g, const float* out, float* dst, int64_t n) {
    return relu_gate<float>(stream, g, out, dst, n);
}
extern "C" int iiseg_relu_gate_f64(void* stream, const double* g, const double* out, double* dst, int64_t n) {
    return relu_gate<double>(stream, g, out, dst, n);
}
extern "C" int iiseg_l2_term_f32(void* stream, const float* p, float* g, int64_t n, const int64_t* ranges,
                                 int32_t nranges, double weight_decay, double* partial, double* penalty) {
    return l2_term<float>(stream, p, g, n, ranges, nranges, weight_decay, partial, penalty);
}
extern "C" int iiseg_l2_term_f64(void* stream, const double* p, double* g, int64_t n, const int64_t* ranges,
                                 int32_t nranges, double weight_decay, double* partial, double* penalty) {
    return l2_term<double>(stream, p, g, n, ranges, nranges, weight_decay, partial, penalty);
}
