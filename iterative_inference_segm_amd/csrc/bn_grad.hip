// The two adjoints peculiar to an FC-DenseNet training step (float32 / float64):
//   bn_relu_bwd    : backward of relu(BatchNorm(x)) with BATCH statistics for ONE consumer of a growing stack --
//                    its own (beta, gamma), the stack's (mean, inv_std) -- in two launches:
//                      reduce : dbeta[c] = sum g_y, dgamma[c] = sum g_y xhat, with y recomputed from x (no saved
//                               t): y = (x - mean) (gamma inv_std) + beta as bn_relu forms it, g_y = g_t [y > 0]
//                               (relu'(0) = 0), xhat = (x - mean) inv_std.  BNB chunks per channel, each a segment
//                               of the plane over every image, summed in double in a fixed order; a finalize
//                               launch adds the chunks in chunk order.  No atomics: two runs give the same bits.
//                      apply  : gstack[:, c] += gamma inv_std (g_y - dbeta / N - xhat dgamma / N).  The mean and
//                               variance terms are there because inference and training both run on batch
//                               statistics (batch_norm_use_averages=False).
//                    x and gstack are the first n channels of (B, cap, H, W) buffers (`bstride` elements between
//                    images), g_t is dense (B, n, H, W).  Both launches stream: 2n planes read, then 3n read and n
//                    written; 16-byte accesses when a plane is a whole number of them (and the bases are aligned),
//                    scalar ones otherwise.
//   maxpool2x2_bwd : adjoint of the 2x2 max-pool alone (TransitionDown pools a LINEAR map: no ReLU gate, unlike
//                    pool_relu_bwd): every position equal to the window maximum receives the gradient (the equality
//                    mask the project uses everywhere), zero on a trailing odd row / column.  Ties do occur -- at 0,
//                    between elements dropout has zeroed -- and are harmless: the dropout mask that follows in the
//                    walk multiplies exactly those gradients away.
#include "common.h"

namespace {

constexpr int BNB_MAX_CHUNKS = 64;       // per channel
constexpr int BNB_TARGET_BLOCKS = 2048;  // eight workgroups per CU of 256: n = 16 fills the chip as n = 1000 does
constexpr int BNB_MIN_CHUNK = 1024;      // plane positions per chunk at least (a chunk reads them in every image)

template <typename T> struct vec_of;
template <> struct vec_of<float> { typedef float4 type; static constexpr int N = 4; };
template <> struct vec_of<double> { typedef double2 type; static constexpr int N = 2; };

inline int bnb_chunks(int n, int HW) {
    int k = (BNB_TARGET_BLOCKS + n - 1) / n;
    const int by_size = (HW + BNB_MIN_CHUNK - 1) / BNB_MIN_CHUNK;
    if (k > by_size) k = by_size;
    if (k > BNB_MAX_CHUNKS) k = BNB_MAX_CHUNKS;
    return k < 1 ? 1 : k;
}

// plane positions per chunk: a multiple of 4 (whole 16-byte groups of either type)
inline int bnb_per(int HW, int chunks) {
    const int per = (HW + chunks - 1) / chunks;
    return (per + 3) & ~3;
}

template <typename T>
__device__ inline void bnb_term(T x, T gt, T m, T r, T g, T be, double& s1, double& s2) {
    const T d = x - m;
    const T y = d * g + be;                  // as bn_relu_kernel forms it
    const T gy = y > (T)0 ? gt : (T)0;
    s1 += (double)gy;
    s2 += (double)gy * (double)(d * r);
}

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void bn_relu_bwd_reduce_kernel(const T* __restrict__ x, long long bstride,
                                                                 const T* __restrict__ gt, int B, int C, int HW,
                                                                 int per, const T* __restrict__ beta,
                                                                 const T* __restrict__ gamma,
                                                                 const T* __restrict__ mean,
                                                                 const T* __restrict__ inv_std,
                                                                 double* __restrict__ partial) {
    __shared__ double red[2][4];
    typedef typename vec_of<T>::type V;
    constexpr int N = vec_of<T>::N;
    const int c = blockIdx.y, chunk = blockIdx.x, chunks = gridDim.x;
    const T m = mean[c], r = inv_std[c], g = gamma[c] * r, be = beta[c];
    const int lo = chunk * per, hi = lo + per < HW ? lo + per : HW;
    double s1 = 0.0, s2 = 0.0;
    for (int b = 0; b < B; ++b) {
        const T* xp = x + (size_t)b * bstride + (size_t)c * HW;
        const T* gp = gt + ((size_t)b * C + c) * HW;
        if (VEC) {
            for (int i = lo + (int)threadIdx.x * N; i < hi; i += 256 * N) {
                const V xv = *reinterpret_cast<const V*>(xp + i);
                const V gv = *reinterpret_cast<const V*>(gp + i);
                const T* xs = reinterpret_cast<const T*>(&xv);
                const T* gs = reinterpret_cast<const T*>(&gv);
#pragma unroll
                for (int k = 0; k < N; ++k) bnb_term(xs[k], gs[k], m, r, g, be, s1, s2);
            }
        } else {
            for (int i = lo + (int)threadIdx.x; i < hi; i += 256) bnb_term(xp[i], gp[i], m, r, g, be, s1, s2);
        }
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = s1;
        red[1][threadIdx.x >> 6] = s2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[((size_t)c * chunks + chunk) * 2 + 0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        partial[((size_t)c * chunks + chunk) * 2 + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}

template <typename T>
__global__ void bn_relu_bwd_finalize_kernel(const double* __restrict__ partial, int C, int chunks,
                                            T* __restrict__ dbeta, T* __restrict__ dgamma) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < chunks; ++k) {
        s1 += partial[((size_t)c * chunks + k) * 2 + 0];
        s2 += partial[((size_t)c * chunks + k) * 2 + 1];
    }
    dbeta[c] = (T)s1;
    dgamma[c] = (T)s2;
}

template <typename T>
__device__ inline T bnb_gx(T x, T gt, T gs, T m, T r, T g, T be, T k, T db, T dg) {
    const T d = x - m;
    const T y = d * g + be;
    const T gy = y > (T)0 ? gt : (T)0;
    return gs + k * (gy - db - (d * r) * dg);
}

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void bn_relu_bwd_apply_kernel(const T* __restrict__ x, long long bstride,
                                                                const T* __restrict__ gt, T* __restrict__ gstack,
                                                                int C, int HW, T count, const T* __restrict__ beta,
                                                                const T* __restrict__ gamma,
                                                                const T* __restrict__ mean,
                                                                const T* __restrict__ inv_std,
                                                                const T* __restrict__ dbeta,
                                                                const T* __restrict__ dgamma) {
    typedef typename vec_of<T>::type V;
    constexpr int N = vec_of<T>::N;
    const int c = blockIdx.y, b = blockIdx.z;
    const T m = mean[c], r = inv_std[c], g = gamma[c] * r, be = beta[c];
    const T k = gamma[c] * r, db = dbeta[c] / count, dg = dgamma[c] / count;
    const T* xp = x + (size_t)b * bstride + (size_t)c * HW;
    const T* gp = gt + ((size_t)b * C + c) * HW;
    T* sp = gstack + (size_t)b * bstride + (size_t)c * HW;
    if (VEC) {
        for (int i = (blockIdx.x * 256 + (int)threadIdx.x) * N; i < HW; i += gridDim.x * 256 * N) {
            const V xv = *reinterpret_cast<const V*>(xp + i);
            const V gv = *reinterpret_cast<const V*>(gp + i);
            V sv = *reinterpret_cast<const V*>(sp + i);
            const T* xs = reinterpret_cast<const T*>(&xv);
            const T* gs = reinterpret_cast<const T*>(&gv);
            T* ss = reinterpret_cast<T*>(&sv);
#pragma unroll
            for (int j = 0; j < N; ++j) ss[j] = bnb_gx(xs[j], gs[j], ss[j], m, r, g, be, k, db, dg);
            *reinterpret_cast<V*>(sp + i) = sv;
        }
    } else {
        for (int i = blockIdx.x * 256 + (int)threadIdx.x; i < HW; i += gridDim.x * 256)
            sp[i] = bnb_gx(xp[i], gp[i], sp[i], m, r, g, be, k, db, dg);
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <typename T>
int bn_relu_bwd(void* stream, const T* x, int64_t bstride, const T* gt, T* gstack, int32_t B, int32_t C, int32_t HW,
                const T* beta, const T* gamma, const T* mean, const T* inv_std, T* dbeta, T* dgamma,
                double* workspace, int32_t stages) {
    if (!x || !gt || !gstack || !beta || !gamma || !mean || !inv_std || !dbeta || !dgamma || !workspace)
        return IISEG_ERR_NULL;
    if (B <= 0 || C <= 0 || HW <= 0 || bstride < (int64_t)C * HW) return IISEG_ERR_SHAPE;
    if (C > 65535 || B > 65535 || !(stages & 3) || (stages & ~3)) return IISEG_ERR_UNSUPPORTED;
    constexpr int N = vec_of<T>::N;
    const bool vec = HW % N == 0 && bstride % N == 0 && aligned16(x) && aligned16(gt) && aligned16(gstack);
    const int chunks = bnb_chunks(C, HW), per = bnb_per(HW, chunks);
    hipStream_t s = (hipStream_t)stream;
    if (stages & IISEG_BN_BWD_REDUCE) {
        if (vec)
            IISEG_LAUNCH((bn_relu_bwd_reduce_kernel<T, true>), dim3(chunks, C), dim3(256), 0, s, x, (long long)bstride,
                         gt, B, C, HW, per, beta, gamma, mean, inv_std, workspace);
        else
            IISEG_LAUNCH((bn_relu_bwd_reduce_kernel<T, false>), dim3(chunks, C), dim3(256), 0, s, x, (long long)bstride,
                         gt, B, C, HW, per, beta, gamma, mean, inv_std, workspace);
        IISEG_LAUNCH(bn_relu_bwd_finalize_kernel<T>, dim3((C + 63) / 64), dim3(64), 0, s, (const double*)workspace, C,
                     chunks, dbeta, dgamma);
    }
    if (!(stages & IISEG_BN_BWD_APPLY)) return iiseg_check_launch();
    int gx = (HW + 256 * N - 1) / (256 * N);
    if (gx > 64) gx = 64;
    const T count = (T)((double)B * HW);
    if (vec)
        IISEG_LAUNCH((bn_relu_bwd_apply_kernel<T, true>), dim3(gx, C, B), dim3(256), 0, s, x, (long long)bstride, gt,
                     gstack, C, HW, count, beta, gamma, mean, inv_std, (const T*)dbeta, (const T*)dgamma);
    else
        IISEG_LAUNCH((bn_relu_bwd_apply_kernel<T, false>), dim3(gx, C, B), dim3(256), 0, s, x, (long long)bstride, gt,
                     gstack, C, HW, count, beta, gamma, mean, inv_std, (const T*)dbeta, (const T*)dgamma);
    return iiseg_check_launch();
}

template <typename T>
__global__ __launch_bounds__(256) void maxpool2x2_bwd_kernel(const T* __restrict__ gpool, const T* __restrict__ pre,
                                                             const T* __restrict__ pooled, T* __restrict__ gz,
                                                             int BC, int H, int W, int h, int w) {
    const size_t n = (size_t)BC * H * W;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % W);
        const size_t t = i / W;
        const int y = (int)(t % H);
        const size_t bc = t / H;
        T v = 0;
        if (y < 2 * h && x < 2 * w) {
            const size_t j = (bc * h + (y >> 1)) * (size_t)w + (x >> 1);
            v = pre[i] == pooled[j] ? gpool[j] : (T)0;
        }
        gz[i] = v;
    }
}

template <typename T>
int maxpool2x2_bwd(void* stream, const T* gpool, const T* pre, const T* pooled, T* gz, int32_t BC, int32_t H,
                   int32_t W) {
    if (!gpool || !pre || !pooled || !gz) return IISEG_ERR_NULL;
    if (BC <= 0 || H < 2 || W < 2) return IISEG_ERR_SHAPE;
    size_t g = ((size_t)BC * H * W + 255) / 256;
    if (g > 8192) g = 8192;
    IISEG_LAUNCH(maxpool2x2_bwd_kernel<T>, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, gpool, pre, pooled,
                 gz, BC, H, W, H / 2, W / 2);
    return iiseg_check_launch();
}

}  // namespace

extern "C" int64_t iiseg_bn_relu_bwd_workspace_elems(int32_t C, int32_t HW) {
    if (C <= 0 || HW <= 0) return IISEG_ERR_SHAPE;
    return (int64_t)C * bnb_chunks(C, HW) * 2;
}
extern "C" int iiseg_bn_relu_bwd_f32(void* stream, const float* x, int64_t bstride, const float* g_t, float* gstack,
                                     int32_t B, int32_t C, int32_t HW, const float* beta, const float* gamma,
                                     const float* mean, const float* inv_std, float* dbeta, float* dgamma,
                                     double* workspace, int32_t stages) {
    return bn_relu_bwd<float>(stream, x, bstride, g_t, gstack, B, C, HW, beta, gamma, mean, inv_std, dbeta, dgamma,
                              workspace, stages);
}
extern "C" int iiseg_bn_relu_bwd_f64(void* stream, const double* x, int64_t bstride, const double* g_t,
                                     double* gstack, int32_t B, int32_t C, int32_t HW, const double* beta,
                                     const double* gamma, const double* mean, const double* inv_std, double* dbeta,
                                     double* dgamma, double* workspace, int32_t stages) {
    return bn_relu_bwd<double>(stream, x, bstride, g_t, gstack, B, C, HW, beta, gamma, mean, inv_std, dbeta, dgamma,
                               workspace, stages);
}
extern "C" int iiseg_maxpool2x2_bwd_f32(void* stream, const float* gpool, const float* pre, const float* pooled,
                                        float* gz, int32_t BC, int32_t H, int32_t W) {
    return maxpool2x2_bwd<float>(stream, gpool, pre, pooled, gz, BC, H, W);
}
extern "C" int iiseg_maxpool2x2_bwd_f64(void* stream, const double* gpool, const double* pre, const double* pooled,
                                        double* gz, int32_t BC, int32_t H, int32_t W) {
    return maxpool2x2_bwd<double>(stream, gpool, pre, pooled, gz, BC, H, W);
}
