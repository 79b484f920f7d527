// Dense-CRF mean field (Kraehenbuehl & Koltun, the model pydensecrf's DenseCRF2D defines) with the
// pairwise sums computed exactly inside a (2R+1) x (2R+1) window instead of on a permutohedral lattice.
// Replaces the per-image pydensecrf calls of the reference's crf_inference.py:143-177.  Definition and
// layout: DESIGN.md section "Dense-CRF baseline".
//
//   crf_prepare : U = -log(clamp(P, clip, 1)), Q0 = softmax(-U), colour features I = uint8(255 x)
//                 (clamped), smoothness normaliser n^g = 1/sqrt(Sx(x) Sy(y)) (product of two 1-D border
//                 sums) and appearance normaliser n^b = 1/sqrt(sum_j k_b(i, j)); one pixel per thread,
//                 arithmetic in float64 for both instantiations (it runs once per batch).
//   crf_step    : Q_out = softmax(-U + w_g n^g_i sum_j k_g n^g_j Q_j + w_b n^b_i sum_j k_b n^b_j Q_j),
//                 one launch per iteration, the whole batch in one grid, tiles never cross images.
#include "common.h"

#include <math.h>

namespace {

constexpr int CRF_TW = 64;        // tile width: one lane per output column
constexpr int CRF_WAVES = 4;      // waves per workgroup, one group of PY output rows each
constexpr double LOG2E = 1.4426950408889634;
constexpr float NEG_BIG = -1.0e30f;   // exp2 of it is 0: rows outside the window

template <typename T> struct vec4;
template <> struct vec4<float> { using type = float4; };
template <> struct vec4<double> { using type = double4; };

__device__ inline float crf_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ inline double crf_exp2(double x) { return exp2(x); }

// colour feature of one channel value: floor of the float32 product 255 * x (numpy's
// (255 * img).astype('uint8') on a float32 image), clamped to [0, 255]; with `in255` the value is
// taken as already on 0..255
__device__ inline double crf_colour(double x, bool in255) {
    const float v = in255 ? (float)x : 255.0f * (float)x;
    const double f = floor((double)v);
    return f < 0.0 ? 0.0 : (f > 255.0 ? 255.0 : f);
}

__device__ inline double crf_border_sum(int p, int n, int R, double c) {
    double s = 0.0;
    for (int d = -R; d <= R; ++d)
        if (p + d >= 0 && p + d < n) s += exp(-(double)(d * d) * c);
    return s;
}

template <typename T>
__global__ __launch_bounds__(256) void crf_prepare_kernel(iiseg_crf_desc d, const T* __restrict__ P,
                                                          const T* __restrict__ X, T* __restrict__ U,
                                                          T* __restrict__ Q0, T* __restrict__ I,
                                                          T* __restrict__ ng, T* __restrict__ nb) {
    const int HW = d.H * d.W;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (pix >= HW) return;
    const int y = pix / d.W, x = pix - y * d.W;
    const bool in255 = (d.flags & IISEG_CRF_INPUT_0_255) != 0;
    const size_t pc = (size_t)b * d.C * HW + pix;
    // unary and start
    double u[16];
    double mx = -INFINITY;
    for (int l = 0; l < d.C; ++l) {
        double p = (double)P[pc + (size_t)l * HW];
        p = p < d.clip ? d.clip : (p > 1.0 ? 1.0 : p);
        u[l] = -log(p);
        mx = fmax(mx, -u[l]);
        U[pc + (size_t)l * HW] = (T)u[l];
    }
    double s = 0.0;
    for (int l = 0; l < d.C; ++l) s += exp(-u[l] - mx);
    for (int l = 0; l < d.C; ++l) Q0[pc + (size_t)l * HW] = (T)(exp(-u[l] - mx) / s);
    // colour features
    const T* xb = X + (size_t)b * 3 * HW;
    double ci[3];
    for (int k = 0; k < 3; ++k) {
        ci[k] = crf_colour((double)xb[(size_t)k * HW + pix], in255);
        I[(size_t)b * 3 * HW + (size_t)k * HW + pix] = (T)ci[k];
    }
    // smoothness normaliser: the window sum of a separable Gaussian is a product of border sums
    const double cg = 1.0 / (2.0 * d.sxy_g * d.sxy_g);
    const double sg = crf_border_sum(x, d.W, d.R, cg) * crf_border_sum(y, d.H, d.R, cg);
    ng[(size_t)b * HW + pix] = (T)(1.0 / sqrt(sg));
    // appearance normaliser
    const double cb = 1.0 / (2.0 * d.sxy_b * d.sxy_b), cc = 1.0 / (2.0 * d.srgb * d.srgb);
    double sb = 0.0;
    for (int yy = max(0, y - d.R); yy <= min(d.H - 1, y + d.R); ++yy)
        for (int xx = max(0, x - d.R); xx <= min(d.W - 1, x + d.R); ++xx) {
            const int j = yy * d.W + xx;
            double c2 = 0.0;
            for (int k = 0; k < 3; ++k) {
                const double dc = ci[k] - crf_colour((double)xb[(size_t)k * HW + j], in255);
                c2 += dc * dc;
            }
            const int dy = yy - y, dx = xx - x;
            sb += exp(-(double)(dx * dx + dy * dy) * cb - c2 * cc);
        }
    nb[(size_t)b * HW + pix] = (T)(1.0 / sqrt(sb));
}

// One mean-field iteration.  Workgroup = 4 waves over a CRF_TW x (4 PY) output tile of one image; lane =
// output column, each lane holds PY vertically adjacent output pixels (register blocking: a neighbour
// read from LDS once serves PY outputs, and lanes of a wave read consecutive pixels -- conflict-free
// 16-byte reads).  The (TH + 2R) halo rows pass through LDS in bands of KB rows; per staged pixel:
// Q n^b (CP/4 vec4 planes), {I0, I1, I2, n^g / n^b} (one vec4).
//   appearance : m^b_p(l) += exp2(sx + sy_p - cc |I_i - I_j|^2) * (Q n^b)_j(l)   one exp per (i, j)
//   smoothness : separable -- a row sum h(l) = sum_dx g(dx) (Q n^g)_j(l) per lane and staged row,
//                then m^g_p(l) += g(dy_p) h(l): C FMAs per neighbour instead of per (i, j) pair.
// CP: C rounded up to a multiple of 4 (padding planes are staged as zeros).
template <typename T, int CP, int PY, int KB, bool BIL>
__global__ __launch_bounds__(256) void crf_step_kernel(iiseg_crf_desc d, const T* __restrict__ U,
                                                       const T* __restrict__ Qin, const T* __restrict__ I,
                                                       const T* __restrict__ ng, const T* __restrict__ nb,
                                                       T* __restrict__ Qout) {
    using V = typename vec4<T>::type;
    constexpr int G = CP / 4;
    constexpr int TH = CRF_WAVES * PY;
    extern __shared__ __align__(16) unsigned char crf_smem[];
    const int R = d.R, H = d.H, W = d.W, C = d.C;
    const int SW = CRF_TW + 2 * R;                    // staged row width
    V* sQ = reinterpret_cast<V*>(crf_smem);            // [G][KB][SW]
    V* sF = sQ + G * KB * SW;                          // [KB][SW]

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.z;
    const int x0 = blockIdx.x * CRF_TW, y0 = blockIdx.y * TH;
    const int x = x0 + lane, yw = y0 + wave * PY;      // this lane's outputs: (x, yw + p), p < PY
    const size_t HW = (size_t)H * W;
    const T* Ib = I + (size_t)b * 3 * HW;

    // spatial / colour coefficients in exp2 units
    const T cgl = (T)(LOG2E / (2.0 * d.sxy_g * d.sxy_g));
    const T cbl = (T)(LOG2E / (2.0 * d.sxy_b * d.sxy_b));
    const T ccl = (T)(LOG2E / (2.0 * d.srgb * d.srgb));

    T fi[PY][3];
#pragma unroll
    for (int p = 0; p < PY; ++p) {
        const bool in = x < W && yw + p < H;
        const size_t o = in ? (size_t)(yw + p) * W + x : 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) fi[p][k] = in ? Ib[(size_t)k * HW + o] : (T)0;
    }
    T mb[PY][CP], mg[PY][CP];
#pragma unroll
    for (int p = 0; p < PY; ++p)
#pragma unroll
        for (int l = 0; l < CP; ++l) mb[p][l] = mg[p][l] = (T)0;

    const int ylo = max(0, y0 - R), yhi = min(H - 1, y0 + TH - 1 + R);
    for (int ys0 = ylo; ys0 <= yhi; ys0 += KB) {
        __syncthreads();   // the previous band has been read
        for (int idx = threadIdx.x; idx < KB * SW; idx += 256) {
            const int r = idx / SW, c = idx - r * SW;
            const int ys = ys0 + r, xs = x0 - R + c;
            const bool in = ys <= yhi && xs >= 0 && xs < W;
            const size_t o = in ? (size_t)ys * W + xs : 0;
            T vb = (T)0, rho = (T)0;
            V f;
            f.x = f.y = f.z = f.w = (T)0;
            if (in) {
                vb = nb[(size_t)b * HW + o];
                rho = ng[(size_t)b * HW + o] / vb;
                f.x = Ib[o];
                f.y = Ib[HW + o];
                f.z = Ib[2 * HW + o];
                f.w = rho;
            }
            sF[r * SW + c] = f;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                V q;
                q.x = (in && 4 * g + 0 < C) ? Qin[((size_t)b * C + 4 * g + 0) * HW + o] * vb : (T)0;
                q.y = (in && 4 * g + 1 < C) ? Qin[((size_t)b * C + 4 * g + 1) * HW + o] * vb : (T)0;
                q.z = (in && 4 * g + 2 < C) ? Qin[((size_t)b * C + 4 * g + 2) * HW + o] * vb : (T)0;
                q.w = (in && 4 * g + 3 < C) ? Qin[((size_t)b * C + 4 * g + 3) * HW + o] * vb : (T)0;
                sQ[(g * KB + r) * SW + c] = q;
            }
        }
        __syncthreads();
        const int nr = min(KB, yhi - ys0 + 1);
        for (int r = 0; r < nr; ++r) {
            const int ys = ys0 + r;
            // rows outside every window of this wave's PY outputs: wave-uniform skip
            if (ys < yw - R || ys > yw + PY - 1 + R) continue;
            T sy[PY], gy[PY];
#pragma unroll
            for (int p = 0; p < PY; ++p) {
                const int dy = ys - (yw + p);
                const bool inw = dy >= -R && dy <= R;
                const T e = -(T)(dy * dy);
                sy[p] = inw ? e * cbl : (T)NEG_BIG;
                gy[p] = inw ? crf_exp2(e * cgl) : (T)0;
            }
            T h[CP];
#pragma unroll
            for (int l = 0; l < CP; ++l) h[l] = (T)0;
            const V* rowF = sF + r * SW + lane + R;
            const V* rowQ = sQ + r * SW + lane + R;
            for (int dx = -R; dx <= R; ++dx) {
                const V f = rowF[dx];
                const T e = -(T)(dx * dx);
                const T gx = crf_exp2(e * cgl) * f.w;      // g(dx) n^g_j / n^b_j
                const T sx = e * cbl;
                T wb[PY];
#pragma unroll
                for (int p = 0; p < PY && BIL; ++p) {
                    const T d0 = fi[p][0] - f.x, d1 = fi[p][1] - f.y, d2 = fi[p][2] - f.z;
                    const T c2 = d0 * d0 + d1 * d1 + d2 * d2;
                    wb[p] = crf_exp2(sx + sy[p] - ccl * c2);
                }
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const V q = rowQ[g * KB * SW + dx];
                    const T qv[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        h[4 * g + k] += gx * qv[k];
#pragma unroll
                        for (int p = 0; p < PY && BIL; ++p) mb[p][4 * g + k] += wb[p] * qv[k];
                    }
                }
            }
#pragma unroll
            for (int p = 0; p < PY; ++p)
#pragma unroll
                for (int l = 0; l < CP; ++l) mg[p][l] += gy[p] * h[l];
        }
    }

    // -U + w_g n^g_i m^g + w_b n^b_i m^b, softmax over the C labels (maximum subtracted first)
    if (x >= W) return;
    const T wg = (T)d.w_g, wbb = (T)d.w_b;
#pragma unroll
    for (int p = 0; p < PY; ++p) {
        const int y = yw + p;
        if (y >= H) break;
        const size_t o = (size_t)y * W + x;
        const T gi = wg * ng[(size_t)b * HW + o], bi = BIL ? wbb * nb[(size_t)b * HW + o] : (T)0;
        T e[CP];
        T mx = (T)NEG_BIG;
#pragma unroll
        for (int l = 0; l < CP; ++l)
            if (l < C) {
                e[l] = -U[((size_t)b * C + l) * HW + o] + gi * mg[p][l] + bi * mb[p][l];
                mx = e[l] > mx ? e[l] : mx;
            }
        T s = (T)0;
#pragma unroll
        for (int l = 0; l < CP; ++l)
            if (l < C) {
                e[l] = exp(e[l] - mx);
                s += e[l];
            }
        const T inv = (T)1 / s;
#pragma unroll
        for (int l = 0; l < CP; ++l)
            if (l < C) Qout[((size_t)b * C + l) * HW + o] = e[l] * inv;
    }
}

int crf_check(const iiseg_crf_desc* d) {
    if (!iiseg_crf_supported(d)) return IISEG_ERR_SHAPE;
    return IISEG_OK;
}

template <typename T> constexpr int crf_py() { return sizeof(T) == 4 ? 4 : 2; }
template <typename T> constexpr int crf_kb() { return sizeof(T) == 4 ? 8 : 4; }

template <typename T>
size_t crf_lds_bytes(const iiseg_crf_desc* d) {
    const int CP = (d->C + 3) / 4 * 4;
    return (size_t)(CP / 4 + 1) * crf_kb<T>() * (CRF_TW + 2 * d->R) * 4 * sizeof(T);
}

template <typename T>
int crf_prepare(void* stream, const iiseg_crf_desc* d, const T* P, const T* X, T* U, T* Q0, T* I, T* ng,
                T* nb) {
    if (!d || !P || !X || !U || !Q0 || !I || !ng || !nb) return IISEG_ERR_NULL;
    if (int st = crf_check(d)) return st;
    const dim3 grid((unsigned)((d->H * d->W + 255) / 256), (unsigned)d->B);
    IISEG_LAUNCH(crf_prepare_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, *d, P, X, U, Q0, I, ng, nb);
    return iiseg_check_launch();
}

template <typename T, int CP>
int crf_step_cp(hipStream_t s, const iiseg_crf_desc* d, const T* U, const T* Qin, const T* I, const T* ng,
                const T* nb, T* Qout) {
    constexpr int PY = crf_py<T>(), KB = crf_kb<T>();
    const dim3 grid((unsigned)((d->W + CRF_TW - 1) / CRF_TW), (unsigned)((d->H + CRF_WAVES * PY - 1) / (CRF_WAVES * PY)),
                    (unsigned)d->B);
    const size_t lds = crf_lds_bytes<T>(d);
    if (d->flags & IISEG_CRF_BILATERAL)
        IISEG_LAUNCH((crf_step_kernel<T, CP, PY, KB, true>), grid, dim3(256), lds, s, *d, U, Qin, I, ng, nb, Qout);
    else
        IISEG_LAUNCH((crf_step_kernel<T, CP, PY, KB, false>), grid, dim3(256), lds, s, *d, U, Qin, I, ng, nb, Qout);
    return iiseg_check_launch();
}

template <typename T>
int crf_step(void* stream, const iiseg_crf_desc* d, const T* U, const T* Qin, const T* I, const T* ng,
             const T* nb, T* Qout) {
    if (!d || !U || !Qin || !I || !ng || !nb || !Qout) return IISEG_ERR_NULL;
    if (int st = crf_check(d)) return st;
    if (Qin == Qout) return IISEG_ERR_SHAPE;     // ping-pong: never in place
    hipStream_t s = (hipStream_t)stream;
    switch ((d->C + 3) / 4) {
        case 1: return crf_step_cp<T, 4>(s, d, U, Qin, I, ng, nb, Qout);
        case 2: return crf_step_cp<T, 8>(s, d, U, Qin, I, ng, nb, Qout);
        case 3: return crf_step_cp<T, 12>(s, d, U, Qin, I, ng, nb, Qout);
        default: return crf_step_cp<T, 16>(s, d, U, Qin, I, ng, nb, Qout);
    }
}

}  // namespace

extern "C" int iiseg_crf_supported(const iiseg_crf_desc* d) {
    if (!d) return 0;
    if (d->B < 1 || d->B > 65535 || d->C < 2 || d->C > 16 || d->R < 1 || d->R > 16) return 0;
    if (d->H < 1 || d->W < 1 || (int64_t)d->H * d->W > (int64_t)1 << 30) return 0;
    if ((d->flags & ~(uint32_t)(IISEG_CRF_BILATERAL | IISEG_CRF_INPUT_0_255)) != 0) return 0;
    if (!(d->sxy_g > 0) || !(d->sxy_b > 0) || !(d->srgb > 0) || !(d->clip > 0) || !(d->clip <= 1)) return 0;
    if (!isfinite(d->w_g) || !isfinite(d->w_b)) return 0;
    return 1;
}

extern "C" int iiseg_crf_prepare_f32(void* stream, const iiseg_crf_desc* d, const float* P, const float* X,
                                     float* U, float* Q0, float* I, float* ng, float* nb) {
    return crf_prepare<float>(stream, d, P, X, U, Q0, I, ng, nb);
}
extern "C" int iiseg_crf_prepare_f64(void* stream, const iiseg_crf_desc* d, const double* P, const double* X,
                                     double* U, double* Q0, double* I, double* ng, double* nb) {
    return crf_prepare<double>(stream, d, P, X, U, Q0, I, ng, nb);
}
extern "C" int iiseg_crf_step_f32(void* stream, const iiseg_crf_desc* d, const float* U, const float* Qin,
                                  const float* I, const float* ng, const float* nb, float* Qout) {
    return crf_step<float>(stream, d, U, Qin, I, ng, nb, Qout);
}
extern "C" int iiseg_crf_step_f64(void* stream, const iiseg_crf_desc* d, const double* U, const double* Qin,
                                  const double* I, const double* ng, const double* nb, double* Qout) {
    return crf_step<double>(stream, d, U, Qin, I, ng, nb, Qout);
}
