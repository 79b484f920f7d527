// True-gradient refinement through the context-module DAE: the two kernels the
// backward pass w.r.t. y needs beyond what training brought (ctx_train.hip), in fp32 and float64.
//
//   conv_small_dgrad : g_x of a 'valid' 1x1 / (dilated) 3x3 layer between at most 16 channels from
//                      g_z = g_out [out > 0], the mask applied WHILE g_out is read (predicated taps: a tap
//                      outside g_out is a zero), for a window of g_x and a range of input channels.
//   ctx_grad_head    : (score, y, out6) -> g_z of dilconv6: softmax, the squared-error gradient through it,
//                      the adjoint of the 1x1 layer and dilconv6's mask, per pixel in registers -- the mirror
//                      of ctx_tail_kernel (conv_small.hip).
//
// Both run on the vector ALU like conv_small_f32_kernel (11 channels fill 11 of 16 MFMA columns):
// a thread owns four consecutive pixels of a row and all its input channels in registers.  Sum order: from 0,
// output-channel-major / tap-minor sequential FMAs.  No atomics.
#include "common.h"
#include "tail_math.h"

#include <string.h>

namespace {

constexpr int DG_TW = 64, DG_TH = 16;          // tile of g_x: 16 rows x 16 groups of four columns

struct dgrad_params {
    int B, Cout, dil, OH, OW;
    int oH, oW, oy0, ox0;                      // the planes `out` lives in and where its (OH, OW) map starts
    int wy0, wx0, WH, WW;                      // window of g_x
    int ci0, nci;
    int gxC, gxH, gxW, gxc0, gxy0, gxx0;       // destination planes and the window's corner in them
    long long so, sc;                          // parameter element (co, ci, tap) at co so + ci sc + tap
    int tiles_y, tiles_x;
};

template <typename T>
struct quad {
    T v[4];
};

// four consecutive elements of row `yy` of an (nrow, n)-map inside planes of width `pw`, starting at column x0;
// what lies outside the map is a zero.  Branch-free (the index of an outside element is clamped to the plane's
// first element and the value dropped): with a branch per tap the loads of one tap could not be issued under the
// FMAs of the one before, and the kernel ran at the latency of 2 x 9 x Cout dependent loads per thread.
template <typename T>
__device__ __forceinline__ quad<T> load4(const T* __restrict__ plane, int pw, int yy, int nrow, int x0, int n) {
    quad<T> q;
    const bool rowok = (unsigned)yy < (unsigned)nrow;
    const int base = yy * pw + x0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const bool ok = rowok && (unsigned)(x0 + e) < (unsigned)n;
        const T v = plane[ok ? (unsigned)(base + e) : 0u];        // (uniform base + 32-bit offset)
        q.v[e] = ok ? v : (T)0;
    }
    return q;
}

template <typename T, int K, int CIP>
__global__ __launch_bounds__(256) void conv_small_dgrad_kernel(const dgrad_params p, const T* __restrict__ gout,
                                                               const T* __restrict__ out, const T* __restrict__ Wt,
                                                               T* __restrict__ gx) {
    constexpr int TAPS = K * K;
    typedef T T2 __attribute__((ext_vector_type(2)));
    // the weights of the launch, [co][tap][ci] (channels past nci are zeros): every thread reads the same row
    __shared__ __attribute__((aligned(16))) T sw[16 * TAPS * CIP];
    for (int idx = threadIdx.x; idx < p.Cout * TAPS * CIP; idx += 256) {
        const int ci = idx % CIP, t = (idx / CIP) % TAPS, co = idx / (CIP * TAPS);
        sw[idx] = ci < p.nci ? Wt[(long long)co * p.so + (long long)(p.ci0 + ci) * p.sc + t] : (T)0;
    }
    __syncthreads();
    const int tid = threadIdx.x, tx = tid & 15, tyy = tid >> 4;
    const int tpi = p.tiles_y * p.tiles_x;
    const int b = blockIdx.x / tpi;
    const int tr = blockIdx.x - b * tpi;
    const int ty = tr / p.tiles_x, txx = tr - ty * p.tiles_x;
    const int wy = ty * DG_TH + tyy, wx = txx * DG_TW + tx * 4;        // window coordinates of the first pixel
    const int nv = min(4, p.WW - wx);
    if (wy >= p.WH || nv <= 0) return;                                  // (no barrier after this point)
    const int gy = p.wy0 + wy, gx0 = p.wx0 + wx;                        // coordinates in the whole g_x map

    T2 acc[4][CIP / 2];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int j = 0; j < CIP / 2; ++j) acc[e][j] = T2{(T)0, (T)0};

    const size_t gpl = (size_t)p.OH * p.OW, opl = (size_t)p.oH * p.oW;
    const T* gb = gout + (size_t)b * p.Cout * gpl;
    const T* ob = out ? out + (size_t)b * p.Cout * opl + (size_t)p.oy0 * p.oW + p.ox0 : nullptr;
    for (int co = 0; co < p.Cout; ++co) {
        const T* gc = gb + (size_t)co * gpl;
        const T* oc = ob ? ob + (size_t)co * opl : nullptr;
#pragma unroll
        for (int t = 0; t < TAPS; ++t) {
            const int yy = gy - (t / K) * p.dil, xx = gx0 - (t % K) * p.dil;
            // (one tap row's loads in flight at a time: all nine would spill)
            if (t % K == 0) __builtin_amdgcn_sched_barrier(0);
            quad<T> g = load4<T>(gc, p.OW, yy, p.OH, xx, p.OW);
            if (oc) {
                const quad<T> o = load4<T>(oc, p.oW, yy, p.OH, xx, p.OW);
#pragma unroll
                for (int e = 0; e < 4; ++e) g.v[e] = o.v[e] > (T)0 ? g.v[e] : (T)0;            // relu'(0) = 0
            }
            const T2* wr = reinterpret_cast<const T2*>(sw + (co * TAPS + t) * CIP);
#pragma unroll
            for (int j = 0; j < CIP / 2; ++j) {
                const T2 w = wr[j];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e][j] = __builtin_elementwise_fma(T2{g.v[e], g.v[e]}, w, acc[e][j]);
            }
        }
    }
    T* xb = gx + (((size_t)b * p.gxC + p.gxc0) * p.gxH + p.gxy0 + wy) * p.gxW + p.gxx0 + wx;
    const size_t xpl = (size_t)p.gxH * p.gxW;
#pragma unroll
    for (int ci = 0; ci < CIP; ++ci) {
        if (ci >= p.nci) continue;                 // (no `break`: the loop must unroll, acc lives in registers)
        quad<T> q;
#pragma unroll
        for (int e = 0; e < 4; ++e) q.v[e] = acc[e][ci / 2][ci & 1];
        T* dst = xb + (size_t)ci * xpl;
        if (nv == 4) {
            memcpy(dst, &q, sizeof(q));
        } else {
#pragma unroll
            for (int e = 0; e < 3; ++e)
                if (e < nv) dst[e] = q.v[e];
        }
    }
}

// ---- the head of the chain: one thread per pixel ----
template <typename T>
__global__ __launch_bounds__(256) void ctx_grad_head_kernel(const T* __restrict__ score, const T* __restrict__ yin,
                                                            const T* __restrict__ out6, const T* __restrict__ W7,
                                                            long long so, long long sc, T* __restrict__ gs,
                                                            T* __restrict__ g6, int C, int Cin, int HW) {
    __shared__ T sw[16][16];                   // [co][ci] of the 1x1 layer
    {
        const int co = threadIdx.x >> 4, ci = threadIdx.x & 15;
        sw[co][ci] = (co < C && ci < Cin) ? W7[(long long)co * so + (long long)ci * sc] : (T)0;
    }
    __syncthreads();
    const int pix = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (pix >= HW) return;
    const T* sp = score + (size_t)b * C * HW + pix;
    const T* yp = yin + (size_t)b * C * HW + pix;
    T r[16], g[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        r[c] = c < C ? sp[(size_t)c * HW] : (T)0;
        g[c] = c < C ? yp[(size_t)c * HW] : (T)0;
    }
    // (the arithmetic of sqerr_softmax_bwd_kernel, tail.hip: the same bits)
    softmax_column<16, T>(C, r);
    T dot = 0;
#pragma unroll
    for (int c = 0; c < 16; ++c)
        if (c < C) {
            g[c] = (T)2 * (r[c] - g[c]);
            dot = fma(r[c], g[c], dot);
        }
#pragma unroll
    for (int c = 0; c < 16; ++c) g[c] = c < C ? r[c] * (g[c] - dot) : (T)0;
    if (gs) {
        T* gp = gs + (size_t)b * C * HW + pix;
#pragma unroll
        for (int c = 0; c < 16; ++c)
            if (c < C) gp[(size_t)c * HW] = g[c];
    }
    // g6 = W7^T g_s (the FMA chain of conv_small_dgrad_kernel<T, 1, .>), masked by [out6 > 0]
    const T* op = out6 ? out6 + (size_t)b * Cin * HW + pix : nullptr;
    T* xp = g6 + (size_t)b * Cin * HW + pix;
#pragma unroll
    for (int ci = 0; ci < 16; ++ci) {
        if (ci >= Cin) continue;
        T a = 0;
#pragma unroll
        for (int co = 0; co < 16; ++co)
            if (co < C) a = fma(g[co], sw[co][ci], a);
        if (op && !(op[(size_t)ci * HW] > (T)0)) a = 0;
        xp[(size_t)ci * HW] = a;
    }
}

// ---- host side ----
int dgrad_check(const iiseg_dgrad_desc* d) {
    if (d->K != 1 && d->K != 3) return IISEG_ERR_SHAPE;
    if (d->B < 1 || d->B > 65535 || d->Cin < 1 || d->Cin > 16 || d->Cout < 1 || d->Cout > 16 || d->dil < 1 ||
        d->OH < 1 || d->OW < 1 || (int64_t)d->OH * d->OW > (int64_t)1 << 30 || d->dil > 1 << 20)
        return IISEG_ERR_SHAPE;
    const int64_t XH = (int64_t)d->OH + (int64_t)d->dil * (d->K - 1), XW = (int64_t)d->OW + (int64_t)d->dil * (d->K - 1);
    // the map `out` is read on: (OH, OW) at (out_y0, out_x0) of (out_H, out_W) planes
    if (d->out_y0 < 0 || d->out_x0 < 0 || (int64_t)d->out_H < (int64_t)d->out_y0 + d->OH ||
        (int64_t)d->out_W < (int64_t)d->out_x0 + d->OW || (int64_t)d->out_H * d->out_W > (int64_t)1 << 30)
        return IISEG_ERR_SHAPE;
    // the window of g_x and the channel range
    if (d->wy0 < 0 || d->wx0 < 0 || d->WH < 1 || d->WW < 1 || (int64_t)d->wy0 + d->WH > XH || (int64_t)d->wx0 + d->WW > XW)
        return IISEG_ERR_SHAPE;
    if (d->ci0 < 0 || d->nci < 1 || (int64_t)d->ci0 + d->nci > d->Cin) return IISEG_ERR_SHAPE;
    // the destination: channels [gx_c0, gx_c0 + nci) of (B, gx_C, gx_H, gx_W), the window at (gx_y0, gx_x0)
    if (d->gx_c0 < 0 || d->gx_y0 < 0 || d->gx_x0 < 0 || (int64_t)d->gx_c0 + d->nci > d->gx_C ||
        (int64_t)d->gx_y0 + d->WH > d->gx_H || (int64_t)d->gx_x0 + d->WW > d->gx_W ||
        (int64_t)d->gx_H * d->gx_W > (int64_t)1 << 30)
        return IISEG_ERR_SHAPE;
    const int64_t kk = d->K * d->K;
    if (!((d->so == d->Cin * kk && d->sc == kk) || (d->so == kk && d->sc == d->Cout * kk))) return IISEG_ERR_SHAPE;
    return IISEG_OK;
}

int dgrad_blocks(const iiseg_dgrad_desc* d) {
    if (!d) return IISEG_ERR_NULL;
    if (int st = dgrad_check(d)) return st;
    const int64_t n = (int64_t)((d->WW + DG_TW - 1) / DG_TW) * ((d->WH + DG_TH - 1) / DG_TH) * d->B;
    return n > (int64_t)1 << 30 ? IISEG_ERR_SHAPE : (int)n;
}

template <typename T, int K>
void dgrad_launch(hipStream_t s, dim3 grid, int cip, const dgrad_params& p, const T* gout, const T* out, const T* W, T* gx) {
    switch (cip) {
        case 4: IISEG_LAUNCH((conv_small_dgrad_kernel<T, K, 4>), grid, dim3(256), 0, s, p, gout, out, W, gx); break;
        case 8: IISEG_LAUNCH((conv_small_dgrad_kernel<T, K, 8>), grid, dim3(256), 0, s, p, gout, out, W, gx); break;
        case 12: IISEG_LAUNCH((conv_small_dgrad_kernel<T, K, 12>), grid, dim3(256), 0, s, p, gout, out, W, gx); break;
        default: IISEG_LAUNCH((conv_small_dgrad_kernel<T, K, 16>), grid, dim3(256), 0, s, p, gout, out, W, gx); break;
    }
}

template <typename T>
int dgrad(void* stream, const iiseg_dgrad_desc* d, const T* gout, const T* out, const T* W, T* gx) {
    if (!d || !gout || !W || !gx) return IISEG_ERR_NULL;
    const int nblk = dgrad_blocks(d);
    if (nblk < 0) return nblk;
    dgrad_params p;
    p.B = d->B; p.Cout = d->Cout; p.dil = d->dil; p.OH = d->OH; p.OW = d->OW;
    p.oH = d->out_H; p.oW = d->out_W; p.oy0 = d->out_y0; p.ox0 = d->out_x0;
    p.wy0 = d->wy0; p.wx0 = d->wx0; p.WH = d->WH; p.WW = d->WW;
    p.ci0 = d->ci0; p.nci = d->nci;
    p.gxC = d->gx_C; p.gxH = d->gx_H; p.gxW = d->gx_W; p.gxc0 = d->gx_c0; p.gxy0 = d->gx_y0; p.gxx0 = d->gx_x0;
    p.so = d->so; p.sc = d->sc;
    p.tiles_y = (d->WH + DG_TH - 1) / DG_TH;
    p.tiles_x = (d->WW + DG_TW - 1) / DG_TW;
    const dim3 grid((unsigned)nblk);
    const int cip = (d->nci + 3) / 4 * 4;
    hipStream_t s = (hipStream_t)stream;
    if (d->K == 1) dgrad_launch<T, 1>(s, grid, cip, p, gout, out, W, gx);
    else dgrad_launch<T, 3>(s, grid, cip, p, gout, out, W, gx);
    return iiseg_check_launch();
}

int head_blocks(int B, int C, int Cin, int H, int W) {
    if (B < 1 || B > 65535 || C < 2 || C > 16 || Cin < 1 || Cin > 16 || H < 1 || W < 1 || (int64_t)H * W > (int64_t)1 << 30)
        return IISEG_ERR_SHAPE;
    return B * ((H * W + 255) / 256);
}

template <typename T>
int grad_head(void* stream, const T* score, const T* y, const T* out6, const T* W7, int64_t so, int64_t sc, T* gs, T* g6,
              int B, int C, int Cin, int H, int W) {
    if (!score || !y || !W7 || !g6) return IISEG_ERR_NULL;
    const int nblk = head_blocks(B, C, Cin, H, W);
    if (nblk < 0) return nblk;
    if (!((so == Cin && sc == 1) || (so == 1 && sc == C))) return IISEG_ERR_SHAPE;
    IISEG_LAUNCH(ctx_grad_head_kernel<T>, dim3((unsigned)(nblk / B), (unsigned)B), dim3(256), 0, (hipStream_t)stream, score, y,
                 out6, W7, (long long)so, (long long)sc, gs, g6, C, Cin, H * W);
    return iiseg_check_launch();
}

}  // namespace

extern "C" int iiseg_conv_small_dgrad_blocks(const iiseg_dgrad_desc* d) { return dgrad_blocks(d); }
extern "C" int iiseg_conv_small_dgrad_f32(void* stream, const iiseg_dgrad_desc* d, const float* gout, const float* out,
                                          const float* W, float* gx) {
    return dgrad<float>(stream, d, gout, out, W, gx);
}
extern "C" int iiseg_conv_small_dgrad_f64(void* stream, const iiseg_dgrad_desc* d, const double* gout, const double* out,
                                          const double* W, double* gx) {
    return dgrad<double>(stream, d, gout, out, W, gx);
}
extern "C" int iiseg_ctx_grad_head_blocks(int32_t B, int32_t C, int32_t Cin, int32_t H, int32_t W) {
    return head_blocks(B, C, Cin, H, W);
}
extern "C" int iiseg_ctx_grad_head_f32(void* stream, const float* score, const float* y, const float* out6, const float* W7,
                                       int64_t so, int64_t sc, float* gs, float* g6, int32_t B, int32_t C, int32_t Cin,
                                       int32_t H, int32_t W) {
    return grad_head<float>(stream, score, y, out6, W7, so, sc, gs, g6, B, C, Cin, H, W);
}
extern "C" int iiseg_ctx_grad_head_f64(void* stream, const double* score, const double* y, const double* out6,
                                       const double* W7, int64_t so, int64_t sc, double* gs, double* g6, int32_t B, int32_t C,
                                       int32_t Cin, int32_t H, int32_t W) {
    return grad_head<double>(stream, score, y, out6, W7, so, sc, gs, g6, B, C, Cin, H, W);
}
