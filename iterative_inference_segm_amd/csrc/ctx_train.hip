// Training the context-module DAE (reference train_dae.py with dae kind 'contextmod'): the three kernels
// its backward pass needs beyond the forward layers.  Definition and measurements: DESIGN.md section 9.
//
//   ctx_loss          : r = softmax(score), the reference's crossentropy / squared_error (metrics.py:68-91,
//                       144-156) and g_score = dL/dscore in one pass; the batch divisors 1 / sum(mask) come
//                       from ctx_loss_count (a launch of its own on the target), so g_score is normalised.
//   conv_small_wgrad  : dW / db of a 'valid' 1x1 / (dilated) 3x3 layer between at most 16 channels; applies
//                       the ReLU mask while reading g_out and stores g_z = g_out [out > 0] once (optionally
//                       inside a zero-bordered buffer: the data-gradient layer then runs 'valid' on it).
//   opt_step          : Lasagne's rmsprop / adam on one flat parameter buffer, lr read from device memory.
//
// Every sum has a fixed order (lane -> wave -> slab per workgroup -> slabs in slab order, in double): the same
// inputs give the same bits on every run.  No floating-point atomics.
#include "common.h"
#include "tail_math.h"

#include <math.h>

namespace {

constexpr int LOSS_BLOCK = 256;

__device__ inline float log_t(float x) { return logf(x); }
__device__ inline double log_t(double x) { return log(x); }

// sum of v over the 256 threads of the block in a fixed order (lanes by butterfly, then waves 0..3)
__device__ inline double block_sum_256(double v, double* s4) {
    v = wave_sum(v);
    __syncthreads();          // s4 of a previous call has been read
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((s4[0] + s4[1]) + s4[2]) + s4[3];
}

// ---- mask counts of the batch: N_ce = #{pixels whose arg-max channel is not the void channel},
//      N_se = sum_px sum_{c < C} t[c]  (metrics.py:76-78, 148) ----
template <typename T>
__global__ __launch_bounds__(LOSS_BLOCK) void ctx_loss_count_kernel(const T* __restrict__ t, double* __restrict__ partial,
                                                                    int C, int HW) {
    __shared__ double s4[4];
    const int pix = blockIdx.x * LOSS_BLOCK + threadIdx.x;
    const int b = blockIdx.y;
    double mce = 0.0, mse = 0.0;
    if (pix < HW) {
        const T* tp = t + (size_t)b * (C + 1) * HW + pix;
        T best = tp[0];
        int label = 0;
        T s = 0;
        for (int c = 0; c <= C; ++c) {
            const T v = tp[(size_t)c * HW];
            if (v > best) { best = v; label = c; }        // first maximum, as T.argmax
            if (c < C) s += v;
        }
        mce = label != C ? 1.0 : 0.0;
        mse = (double)s;
    }
    const double a = block_sum_256(mce, s4);
    const double q = block_sum_256(mse, s4);
    if (threadIdx.x == 0) {
        const size_t blk = (size_t)b * gridDim.x + blockIdx.x;
        partial[2 * blk] = a;
        partial[2 * blk + 1] = q;
    }
}

// one block: column sums of partial[n][2] in a fixed order (thread-strided, then the block tree)
__device__ inline void columns2(const double* partial, int n, double* s4, double& a, double& q) {
    double va = 0.0, vq = 0.0;
    for (int k = threadIdx.x; k < n; k += LOSS_BLOCK) {
        va += partial[2 * k];
        vq += partial[2 * k + 1];
    }
    a = block_sum_256(va, s4);
    q = block_sum_256(vq, s4);
}

// cnt = {N_ce, N_se, 1 / N_ce, 1 / N_se}; an empty mask gives the reciprocal 0 (loss and gradient 0, no NaN)
__global__ __launch_bounds__(LOSS_BLOCK) void ctx_loss_count_finalize_kernel(const double* __restrict__ partial, int n,
                                                                             double* __restrict__ cnt) {
    __shared__ double s4[4];
    double a, q;
    columns2(partial, n, s4, a, q);
    if (threadIdx.x == 0) {
        cnt[0] = a;
        cnt[1] = q;
        cnt[2] = a > 0.0 ? 1.0 / a : 0.0;
        cnt[3] = q > 0.0 ? 1.0 / q : 0.0;
    }
}

template <typename T>
__global__ __launch_bounds__(LOSS_BLOCK) void ctx_loss_kernel(const T* __restrict__ score, const T* __restrict__ t,
                                                              const double* __restrict__ cnt, T* __restrict__ g,
                                                              double* __restrict__ partial, int C, int HW,
                                                              unsigned flags, double lmb) {
    __shared__ double s4[4];
    const int pix = blockIdx.x * LOSS_BLOCK + threadIdx.x;
    const int b = blockIdx.y;
    double lce = 0.0, lse = 0.0;
    if (pix < HW) {
        const T* sp = score + (size_t)b * C * HW + pix;
        const T* tp = t + (size_t)b * (C + 1) * HW + pix;
        T r[16], tv[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            r[c] = c < C ? sp[(size_t)c * HW] : (T)0;
            tv[c] = c < C ? tp[(size_t)c * HW] : (T)0;
        }
        softmax_column<16, T>(C, r);
        T best = tv[0];
        int label = 0;
        T msum = 0;
#pragma unroll
        for (int c = 0; c < 16; ++c)
            if (c < C) {
                if (tv[c] > best) { best = tv[c]; label = c; }
                msum += tv[c];
            }
        const bool isvoid = tp[(size_t)C * HW] > best;
        // weights of the two terms in dL/dr: flag / N_ce and lmb / N_se
        const T wce = (flags & IISEG_LOSS_CROSSENTROPY) && !isvoid ? (T)cnt[2] : (T)0;
        const T wse = (flags & IISEG_LOSS_SQUARED_ERROR) ? (T)(lmb * cnt[3]) * msum : (T)0;
        const T eps = (T)1e-7, one_eps = (T)1 - (T)1e-7;          // _EPSILON = 10e-8
        T gr[16];
        T dot = 0, se = 0, rl = 0;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            gr[c] = 0;
            if (c < C) {
                const T d = r[c] - tv[c];
                se += d * d;
                gr[c] = wse * ((T)2 * d / (T)C);
                if (c == label) {
                    rl = r[c];
                    // T.clip passes the gradient only where the value is inside the interval
                    if (r[c] >= eps && r[c] <= one_eps) gr[c] -= wce / r[c];
                }
                dot += r[c] * gr[c];
            }
        }
        if (!isvoid) {
            const T p = rl < eps ? eps : (rl > one_eps ? one_eps : rl);
            lce = -(double)log_t(p);
        }
        lse = (double)msum * ((double)se / (double)C);
        if (g) {
            T* gp = g + (size_t)b * C * HW + pix;
#pragma unroll
            for (int c = 0; c < 16; ++c)
                if (c < C) gp[(size_t)c * HW] = r[c] * (gr[c] - dot);     // softmax backward
        }
    }
    const double a = block_sum_256(lce, s4);
    const double q = block_sum_256(lse, s4);
    if (threadIdx.x == 0) {
        const size_t blk = (size_t)b * gridDim.x + blockIdx.x;
        partial[2 * blk] = a;
        partial[2 * blk + 1] = q;
    }
}

// res = {loss, crossentropy, squared_error}: the two masked means and their flagged, weighted sum
__global__ __launch_bounds__(LOSS_BLOCK) void ctx_loss_finalize_kernel(const double* __restrict__ partial, int n,
                                                                       const double* __restrict__ cnt,
                                                                       double* __restrict__ res, unsigned flags,
                                                                       double lmb) {
    __shared__ double s4[4];
    double a, q;
    columns2(partial, n, s4, a, q);
    if (threadIdx.x == 0) {
        const double ce = a * cnt[2], se = q * cnt[3];
        res[0] = ((flags & IISEG_LOSS_CROSSENTROPY) ? ce : 0.0) + ((flags & IISEG_LOSS_SQUARED_ERROR) ? lmb * se : 0.0);
        res[1] = ce;
        res[2] = se;
    }
}

// ---- weight gradient ----
constexpr int WG_TW = 64;                                                 // tile width: one lane per column
template <typename T> constexpr int wg_rows() { return sizeof(T) == 4 ? 16 : 8; }   // tile rows (LDS: 48 KB)
constexpr int FIN_IDX = 16, FIN_SEG = 16;                                 // finalize: 16 sums x 16 slab segments

struct wgrad_params {
    int B, Cin, Cout, H, W, OH, OW, dil;
    int gzH, gzW, gzy0, gzx0;
    long long so, sc;       // strides of the output / input channel in dW (the layer's own parameter layout)
    int nW;                 // Cin * Cout * K * K; a slab is nW + Cout sums
};

// Workgroup = 4 waves over a 64 x TR tile of output pixels of one image.  Phase 0: g_z = g_out [out > 0] of the
// tile, to LDS (all CP planes; the padding planes are zeros) and to global memory.  Phase 1: wave w takes the
// input channels w, w + 4, ...; lane = column; per row the K*K taps of x come straight from L1 / L2 (coalesced
// row segments whatever the dilation), the g_z column from LDS, K*K x CP FMAs into registers; after the rows
// the wave's sums are reduced across the lanes and written to the workgroup's slab.
template <typename T, int K, int CP>
__global__ __launch_bounds__(256) void conv_small_wgrad_kernel(wgrad_params p, const T* __restrict__ x,
                                                               const T* __restrict__ gout, const T* __restrict__ out,
                                                               T* __restrict__ gz, T* __restrict__ slab) {
    constexpr int TR = wg_rows<T>();
    constexpr int TAPS = K * K;
    __shared__ T sg[CP][TR][WG_TW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.z, x0 = blockIdx.x * WG_TW, y0 = blockIdx.y * TR;
    const size_t blk = ((size_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    T* my = slab + blk * (size_t)(p.nW + p.Cout);

    for (int idx = threadIdx.x; idx < CP * TR * WG_TW; idx += 256) {
        const int c = idx / (TR * WG_TW), r = (idx / WG_TW) % TR, col = idx % WG_TW;
        const int oy = y0 + r, ox = x0 + col;
        T v = 0;
        if (c < p.Cout && oy < p.OH && ox < p.OW) {
            const size_t o = (((size_t)b * p.Cout + c) * p.OH + oy) * p.OW + ox;
            v = gout[o];
            if (out && !(out[o] > (T)0)) v = 0;                          // relu'(0) = 0
            if (gz) gz[(((size_t)b * p.Cout + c) * p.gzH + p.gzy0 + oy) * p.gzW + p.gzx0 + ox] = v;
        }
        sg[c][r][col] = v;
    }
    __syncthreads();

    for (int c = wave; c < p.Cout; c += 4) {                             // db: rows in order, then the lanes
        T s = 0;
#pragma unroll
        for (int r = 0; r < TR; ++r) s += sg[c][r][lane];
        s = wave_sum(s);
        if (lane == 0) my[p.nW + c] = s;
    }

    const bool colok = x0 + lane < p.OW;
    for (int ci = wave; ci < p.Cin; ci += 4) {
        T acc[TAPS][CP];
#pragma unroll
        for (int t = 0; t < TAPS; ++t)
#pragma unroll
            for (int c = 0; c < CP; ++c) acc[t][c] = 0;
        const T* xp = x + (((size_t)b * p.Cin + ci) * p.H + y0) * p.W + x0 + lane;
#pragma unroll 2
        for (int r = 0; r < TR; ++r) {
            if (y0 + r >= p.OH) break;                                   // wave-uniform
            T xv[TAPS];
#pragma unroll
            for (int t = 0; t < TAPS; ++t)
                xv[t] = colok ? xp[(size_t)(r + (t / K) * p.dil) * p.W + (t % K) * p.dil] : (T)0;
#pragma unroll
            for (int c = 0; c < CP; ++c) {
                const T gv = sg[c][r][lane];
#pragma unroll
                for (int t = 0; t < TAPS; ++t) acc[t][c] = fma(xv[t], gv, acc[t][c]);
            }
        }
#pragma unroll
        for (int t = 0; t < TAPS; ++t)
#pragma unroll
            for (int c = 0; c < CP; ++c) {
                const T v = wave_sum(acc[t][c]);
                if (c < p.Cout && lane == ((t * CP + c) & 63)) my[(size_t)c * p.so + (size_t)ci * p.sc + t] = v;
            }
    }
}

// dW / db = the slabs added in slab order, in double: thread (i, s) adds segment s of the slabs for sum i,
// the 16 segments are then added in order
template <typename T>
__global__ __launch_bounds__(FIN_IDX * FIN_SEG) void conv_small_wgrad_finalize_kernel(const T* __restrict__ slab, int nslab,
                                                                                      int nW, int S, T* __restrict__ dW,
                                                                                      T* __restrict__ db) {
    __shared__ double part[FIN_SEG][FIN_IDX];
    const int i = threadIdx.x % FIN_IDX, s = threadIdx.x / FIN_IDX;
    const int idx = blockIdx.x * FIN_IDX + i;
    const int per = (nslab + FIN_SEG - 1) / FIN_SEG;
    const int k0 = s * per, k1 = min(nslab, k0 + per);
    double v = 0.0;
    if (idx < S)
        for (int k = k0; k < k1; ++k) v += (double)slab[(size_t)k * S + idx];
    part[s][i] = v;
    __syncthreads();
    if (s == 0 && idx < S) {
        double tot = 0.0;
#pragma unroll
        for (int q = 0; q < FIN_SEG; ++q) tot += part[q][i];
        if (idx < nW) dW[idx] = (T)tot;
        else db[idx - nW] = (T)tot;
    }
}

// ---- optimizer step: ONE workgroup walks the flat buffer (8129 scalars for the context module), so the step
//      counter state can be read by every thread before thread 0 advances it.  Element-wise formulas in T, each
//      operation rounded on its own (no FMA contraction): the float32 step equals numpy's float32 arithmetic. ----
template <typename T>
__global__ __launch_bounds__(1024) void opt_step_kernel(int kind, T* __restrict__ p, const T* __restrict__ g,
                                                        T* __restrict__ s1, T* __restrict__ s2, const T* __restrict__ lr_p,
                                                        T* __restrict__ state, long long n) {
#pragma clang fp contract(off)
    const T lr = lr_p[0];
    const T one = (T)1;
    if (kind == IISEG_OPT_RMSPROP) {
        const T rho = (T)0.9, eps = (T)1e-6;
        const T omr = one - rho;
        for (long long i = threadIdx.x; i < n; i += 1024) {
            const T gi = g[i];
            const T a = rho * s1[i] + omr * (gi * gi);
            s1[i] = a;
            p[i] = p[i] - (lr * gi) / sqrt_t(a + eps);
        }
        return;
    }
    const T b1 = (T)0.9, b2 = (T)0.999, eps = (T)1e-8;
    // state = {t, b1^t, b2^t}: the powers as running products
    const T t1 = state[0] + one, p1 = state[1] * b1, p2 = state[2] * b2;
    __syncthreads();
    if (threadIdx.x == 0) {
        state[0] = t1;
        state[1] = p1;
        state[2] = p2;
    }
    const T alpha = (lr * sqrt_t(one - p2)) / (one - p1);
    const T omb1 = one - b1, omb2 = one - b2;
    for (long long i = threadIdx.x; i < n; i += 1024) {
        const T gi = g[i];
        const T m = b1 * s1[i] + omb1 * gi;
        const T v = b2 * s2[i] + omb2 * (gi * gi);
        s1[i] = m;
        s2[i] = v;
        p[i] = p[i] - (alpha * m) / (sqrt_t(v) + eps);
    }
}

// ---- grid form of the optimizer step (the standard DAE: tens of millions of scalars).  The per-element
//      arithmetic of opt_step_kernel, so the same bits; every workgroup reads adam's state as the previous step
//      left it and forms the advanced values locally; opt_state_advance_kernel stores them afterwards. ----
constexpr int OPT_GRID_BLOCK = 256;

template <typename T>
__global__ __launch_bounds__(OPT_GRID_BLOCK) void opt_step_grid_kernel(int kind, T* __restrict__ p, const T* __restrict__ g,
                                                                       T* __restrict__ s1, T* __restrict__ s2,
                                                                       const T* __restrict__ lr_p,
                                                                       const T* __restrict__ state, long long n) {
#pragma clang fp contract(off)
    const T lr = lr_p[0];
    const T one = (T)1;
    const long long stride = (long long)gridDim.x * OPT_GRID_BLOCK;
    const long long i0 = (long long)blockIdx.x * OPT_GRID_BLOCK + threadIdx.x;
    if (kind == IISEG_OPT_RMSPROP) {
        const T rho = (T)0.9, eps = (T)1e-6;
        const T omr = one - rho;
        for (long long i = i0; i < n; i += stride) {
            const T gi = g[i];
            const T a = rho * s1[i] + omr * (gi * gi);
            s1[i] = a;
            p[i] = p[i] - (lr * gi) / sqrt_t(a + eps);
        }
        return;
    }
    const T b1 = (T)0.9, b2 = (T)0.999, eps = (T)1e-8;
    const T p1 = state[1] * b1, p2 = state[2] * b2;
    const T alpha = (lr * sqrt_t(one - p2)) / (one - p1);
    const T omb1 = one - b1, omb2 = one - b2;
    for (long long i = i0; i < n; i += stride) {
        const T gi = g[i];
        const T m = b1 * s1[i] + omb1 * gi;
        const T v = b2 * s2[i] + omb2 * (gi * gi);
        s1[i] = m;
        s2[i] = v;
        p[i] = p[i] - (alpha * m) / (sqrt_t(v) + eps);
    }
}

template <typename T>
__global__ void opt_state_advance_kernel(T* __restrict__ state) {
#pragma clang fp contract(off)
    const T t1 = state[0] + (T)1, p1 = state[1] * (T)0.9, p2 = state[2] * (T)0.999;
    state[0] = t1;
    state[1] = p1;
    state[2] = p2;
}

// ---- host side ----
int loss_check(int B, int C, int H, int W) {
    if (B < 1 || B > 65535 || C < 2 || C > 16 || H < 1 || W < 1 || (int64_t)H * W > (int64_t)1 << 30) return IISEG_ERR_SHAPE;
    return IISEG_OK;
}

template <typename T>
int ctx_loss_count(void* stream, const T* target, double* partial, double* cnt, int B, int C, int H, int W) {
    if (!target || !partial || !cnt) return IISEG_ERR_NULL;
    if (int st = loss_check(B, C, H, W)) return st;
    const int HW = H * W, nb = (HW + LOSS_BLOCK - 1) / LOSS_BLOCK;
    hipStream_t s = (hipStream_t)stream;
    IISEG_LAUNCH(ctx_loss_count_kernel<T>, dim3(nb, B), dim3(LOSS_BLOCK), 0, s, target, partial, C, HW);
    IISEG_LAUNCH(ctx_loss_count_finalize_kernel, dim3(1), dim3(LOSS_BLOCK), 0, s, (const double*)partial, nb * B, cnt);
    return iiseg_check_launch();
}

template <typename T>
int ctx_loss(void* stream, const T* score, const T* target, const double* cnt, T* g, double* partial, double* res,
             int B, int C, int H, int W, uint32_t flags, double lmb) {
    if (!score || !target || !cnt || !partial || !res) return IISEG_ERR_NULL;
    if (int st = loss_check(B, C, H, W)) return st;
    if (flags == 0 || (flags & ~(uint32_t)(IISEG_LOSS_CROSSENTROPY | IISEG_LOSS_SQUARED_ERROR)) || !isfinite(lmb))
        return IISEG_ERR_SHAPE;
    const int HW = H * W, nb = (HW + LOSS_BLOCK - 1) / LOSS_BLOCK;
    hipStream_t s = (hipStream_t)stream;
    IISEG_LAUNCH(ctx_loss_kernel<T>, dim3(nb, B), dim3(LOSS_BLOCK), 0, s, score, target, cnt, g, partial, C, HW,
                 (unsigned)flags, lmb);
    IISEG_LAUNCH(ctx_loss_finalize_kernel, dim3(1), dim3(LOSS_BLOCK), 0, s, (const double*)partial, nb * B, cnt, res,
                 (unsigned)flags, lmb);
    return iiseg_check_launch();
}

int wgrad_check(const iiseg_wgrad_desc* d, int& OH, int& OW) {
    if (d->K != 1 && d->K != 3) return IISEG_ERR_SHAPE;
    if (d->B < 1 || d->B > 65535 || d->Cin < 1 || d->Cin > 16 || d->Cout < 1 || d->Cout > 16 || d->dil < 1 ||
        d->H < 1 || d->W < 1 || (int64_t)d->H * d->W > (int64_t)1 << 30)
        return IISEG_ERR_SHAPE;
    OH = d->H - d->dil * (d->K - 1);
    OW = d->W - d->dil * (d->K - 1);
    if (OH < 1 || OW < 1) return IISEG_ERR_SHAPE;
    // g_z placement: the (OH, OW) map inside (gz_H, gz_W) planes at (gz_y0, gz_x0)
    if (d->gz_y0 < 0 || d->gz_x0 < 0 || d->gz_H < d->gz_y0 + OH || d->gz_W < d->gz_x0 + OW) return IISEG_ERR_SHAPE;
    // the parameter layout: 'oihw' (so = Cin K K, sc = K K) or 'iohw' (so = K K, sc = Cout K K)
    const int64_t kk = d->K * d->K;
    if (!((d->so == d->Cin * kk && d->sc == kk) || (d->so == kk && d->sc == d->Cout * kk))) return IISEG_ERR_SHAPE;
    return IISEG_OK;
}

template <typename T>
int wgrad_partials(const iiseg_wgrad_desc* d) {
    int OH, OW;
    if (!d) return IISEG_ERR_NULL;
    if (int st = wgrad_check(d, OH, OW)) return st;
    const int64_t n = (int64_t)((OW + WG_TW - 1) / WG_TW) * ((OH + wg_rows<T>() - 1) / wg_rows<T>()) * d->B;
    return n > (int64_t)1 << 24 ? IISEG_ERR_SHAPE : (int)n;
}

template <typename T, int K>
void wgrad_launch(hipStream_t s, dim3 grid, int cp, const wgrad_params& p, const T* x, const T* gout, const T* out, T* gz,
                  T* slab) {
    switch (cp) {
        case 4: IISEG_LAUNCH((conv_small_wgrad_kernel<T, K, 4>), grid, dim3(256), 0, s, p, x, gout, out, gz, slab); break;
        case 8: IISEG_LAUNCH((conv_small_wgrad_kernel<T, K, 8>), grid, dim3(256), 0, s, p, x, gout, out, gz, slab); break;
        case 12: IISEG_LAUNCH((conv_small_wgrad_kernel<T, K, 12>), grid, dim3(256), 0, s, p, x, gout, out, gz, slab); break;
        default: IISEG_LAUNCH((conv_small_wgrad_kernel<T, K, 16>), grid, dim3(256), 0, s, p, x, gout, out, gz, slab); break;
    }
}

template <typename T>
int wgrad(void* stream, const iiseg_wgrad_desc* d, const T* x, const T* gout, const T* out, T* gz, T* slab, T* dW, T* db) {
    if (!d || !x || !gout || !slab || !dW || !db) return IISEG_ERR_NULL;
    int OH, OW;
    if (int st = wgrad_check(d, OH, OW)) return st;
    const int nslab = wgrad_partials<T>(d);
    if (nslab < 0) return nslab;
    wgrad_params p;
    p.B = d->B; p.Cin = d->Cin; p.Cout = d->Cout; p.H = d->H; p.W = d->W; p.OH = OH; p.OW = OW; p.dil = d->dil;
    p.gzH = d->gz_H; p.gzW = d->gz_W; p.gzy0 = d->gz_y0; p.gzx0 = d->gz_x0;
    p.so = d->so; p.sc = d->sc;
    p.nW = d->Cin * d->Cout * d->K * d->K;
    const dim3 grid((unsigned)((OW + WG_TW - 1) / WG_TW), (unsigned)((OH + wg_rows<T>() - 1) / wg_rows<T>()), (unsigned)d->B);
    hipStream_t s = (hipStream_t)stream;
    const int cp = (d->Cout + 3) / 4 * 4;
    if (d->K == 1) wgrad_launch<T, 1>(s, grid, cp, p, x, gout, out, gz, slab);
    else wgrad_launch<T, 3>(s, grid, cp, p, x, gout, out, gz, slab);
    const int S = p.nW + p.Cout;
    IISEG_LAUNCH(conv_small_wgrad_finalize_kernel<T>, dim3((unsigned)((S + FIN_IDX - 1) / FIN_IDX)), dim3(FIN_IDX * FIN_SEG), 0,
                 s, (const T*)slab, nslab, p.nW, S, dW, db);
    return iiseg_check_launch();
}

template <typename T>
int opt_step(void* stream, int kind, T* p, const T* g, T* s1, T* s2, const T* lr, T* state, int64_t n) {
    if (kind != IISEG_OPT_RMSPROP && kind != IISEG_OPT_ADAM) return IISEG_ERR_SHAPE;
    if (!p || !g || !s1 || !lr) return IISEG_ERR_NULL;
    if (kind == IISEG_OPT_ADAM && (!s2 || !state)) return IISEG_ERR_NULL;
    if (n < 1 || n > (int64_t)1 << 30) return IISEG_ERR_SHAPE;
    IISEG_LAUNCH(opt_step_kernel<T>, dim3(1), dim3(1024), 0, (hipStream_t)stream, kind, p, g, s1, s2, lr, state, (long long)n);
    return iiseg_check_launch();
}

template <typename T>
int opt_step_grid(void* stream, int kind, T* p, const T* g, T* s1, T* s2, const T* lr, T* state, int64_t n) {
    if (kind != IISEG_OPT_RMSPROP && kind != IISEG_OPT_ADAM) return IISEG_ERR_SHAPE;
    if (!p || !g || !s1 || !lr) return IISEG_ERR_NULL;
    if (kind == IISEG_OPT_ADAM && (!s2 || !state)) return IISEG_ERR_NULL;
    if (n < 1 || n > (int64_t)1 << 30) return IISEG_ERR_SHAPE;
    int64_t blocks = (n + OPT_GRID_BLOCK - 1) / OPT_GRID_BLOCK;
    if (blocks > 2048) blocks = 2048;                       // 8 workgroups per CU, grid-stride beyond
    hipStream_t s = (hipStream_t)stream;
    IISEG_LAUNCH(opt_step_grid_kernel<T>, dim3((unsigned)blocks), dim3(OPT_GRID_BLOCK), 0, s, kind, p, g, s1, s2, lr,
                 (const T*)state, (long long)n);
    if (kind == IISEG_OPT_ADAM) IISEG_LAUNCH(opt_state_advance_kernel<T>, dim3(1), dim3(1), 0, s, state);
    return iiseg_check_launch();
}

}  // namespace

extern "C" int iiseg_ctx_loss_partials(int32_t B, int32_t H, int32_t W) {
    if (int st = loss_check(B, 2, H, W)) return st;
    return B * ((H * W + LOSS_BLOCK - 1) / LOSS_BLOCK);
}
extern "C" int iiseg_ctx_loss_count_f32(void* stream, const float* target, double* partial, double* cnt, int32_t B,
                                        int32_t C, int32_t H, int32_t W) {
    return ctx_loss_count<float>(stream, target, partial, cnt, B, C, H, W);
}
extern "C" int iiseg_ctx_loss_count_f64(void* stream, const double* target, double* partial, double* cnt, int32_t B,
                                        int32_t C, int32_t H, int32_t W) {
    return ctx_loss_count<double>(stream, target, partial, cnt, B, C, H, W);
}
extern "C" int iiseg_ctx_loss_f32(void* stream, const float* score, const float* target, const double* cnt, float* g,
                                  double* partial, double* res, int32_t B, int32_t C, int32_t H, int32_t W,
                                  uint32_t flags, double lmb) {
    return ctx_loss<float>(stream, score, target, cnt, g, partial, res, B, C, H, W, flags, lmb);
}
extern "C" int iiseg_ctx_loss_f64(void* stream, const double* score, const double* target, const double* cnt, double* g,
                                  double* partial, double* res, int32_t B, int32_t C, int32_t H, int32_t W,
                                  uint32_t flags, double lmb) {
    return ctx_loss<double>(stream, score, target, cnt, g, partial, res, B, C, H, W, flags, lmb);
}
extern "C" int iiseg_conv_small_wgrad_partials(const iiseg_wgrad_desc* d, int32_t elem_bytes) {
    if (elem_bytes == 4) return wgrad_partials<float>(d);
    if (elem_bytes == 8) return wgrad_partials<double>(d);
    return IISEG_ERR_SHAPE;
}
extern "C" int iiseg_conv_small_wgrad_f32(void* stream, const iiseg_wgrad_desc* d, const float* x, const float* gout,
                                          const float* out, float* gz, float* slab, float* dW, float* db) {
    return wgrad<float>(stream, d, x, gout, out, gz, slab, dW, db);
}
extern "C" int iiseg_conv_small_wgrad_f64(void* stream, const iiseg_wgrad_desc* d, const double* x, const double* gout,
                                          const double* out, double* gz, double* slab, double* dW, double* db) {
    return wgrad<double>(stream, d, x, gout, out, gz, slab, dW, db);
}
extern "C" int iiseg_opt_step_f32(void* stream, int32_t kind, float* p, const float* g, float* s1, float* s2,
                                  const float* lr, float* state, int64_t n) {
    return opt_step<float>(stream, kind, p, g, s1, s2, lr, state, n);
}
extern "C" int iiseg_opt_step_f64(void* stream, int32_t kind, double* p, const double* g, double* s1, double* s2,
                                  const double* lr, double* state, int64_t n) {
    return opt_step<double>(stream, kind, p, g, s1, s2, lr, state, n);
}
extern "C" int iiseg_opt_step_grid_f32(void* stream, int32_t kind, float* p, const float* g, float* s1, float* s2,
                                       const float* lr, float* state, int64_t n) {
    return opt_step_grid<float>(stream, kind, p, g, s1, s2, lr, state, n);
}
extern "C" int iiseg_opt_step_grid_f64(void* stream, int32_t kind, double* p, const double* g, double* s1, double* s2,
                                       const double* lr, double* state, int64_t n) {
    return opt_step_grid<double>(stream, kind, p, g, s1, s2, lr, state, n);
}
