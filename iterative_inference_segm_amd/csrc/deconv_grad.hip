// Backward of the strided transposed convolution of deconv.hip (FCN-8's score2 / score4 / upsample; DESIGN.md
// section 14).  The forward scatters x through W[in,out,k,k] (Lasagne's spatially flipped filter, as deconv.hip
// reads it) into `full`, (H - 1) s + K on a side, and only the window (oy0, ox0, OH, OW) of it is computed:
//
//   full[b][co][s i + a][s j + c] += x[b][ci][i][j] * W[ci][co][K-1-a][K-1-c]   (+ bias[co])        0 <= a, c < K
//
// g is dL/d(window).  With g_full = g at the window's offset inside `full` and zero elsewhere (the crop's adjoint):
//
//   gx[b][ci][i][j]        = sum_{co,a,c} W[ci][co][K-1-a][K-1-c] * g_full[b][co][s i + a][s j + c]
//   dW[ci][co][K-1-a][K-1-c] = sum_{b,i,j}  x[b][ci][i][j]        * g_full[b][co][s i + a][s j + c]
//   db[co]                 = sum g
//
// Any K, stride, channel counts and window; tuned for K = 2 s, a few dozen channels (under 1 GFLOP per batch in
// all): vector-ALU kernels in both precisions.
//   dgrad : a thread owns one element of gx and walks (co, a, c) restricted to the window.
//   wgrad : a thread owns one element of dW (neighbouring threads neighbouring taps: g is read along its rows) and
//           a SLAB of the B H input rows; the workgroups after those of dW own one output channel of db each and
//           the slab's share of the window's pixels.  Every slab goes to the workspace, a finalize launch adds
//           the slabs in slab order in double.  No atomics: the same inputs give the same bits.
#include "common.h"

namespace {

constexpr int TARGET_WORKGROUPS = 2048;                  // eight per CU: short serial walks, many of them

struct dg_params {
    int B, Cin, H, W, Cout, K, s;
    int oy0, ox0, OH, OW;
    long long nW, S;              // Cin Cout K^2, nW + Cout
    int nblkW;                    // workgroups of dW in one slab
    int nslab, rps;               // slabs, input rows (of B H) per slab
    long long pps;                // window pixels (of B OH OW) per slab
};

template <typename T>
__global__ __launch_bounds__(256) void deconv_dgrad_kernel(dg_params p, const T* __restrict__ g, const T* __restrict__ w,
                                                           T* __restrict__ gx) {
    const long long n = (long long)p.B * p.Cin * p.H * p.W;
    const int KK = p.K * p.K;
    const long long OHW = (long long)p.OH * p.OW;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long long)gridDim.x * 256) {
        const int j = (int)(idx % p.W), i = (int)((idx / p.W) % p.H);
        const int ci = (int)((idx / ((long long)p.W * p.H)) % p.Cin), b = (int)(idx / ((long long)p.W * p.H * p.Cin));
        // rows / columns of `full` this element reaches, cut to the window
        const int a0 = max(0, p.oy0 - p.s * i), a1 = min(p.K, p.oy0 + p.OH - p.s * i);
        const int c0 = max(0, p.ox0 - p.s * j), c1 = min(p.K, p.ox0 + p.OW - p.s * j);
        // four chains in flight: the walk is latency-bound (one FMA between two loads)
        T acc0 = 0, acc1 = 0, acc2 = 0, acc3 = 0;
        for (int co = 0; co < p.Cout; ++co) {
            const T* wp = w + ((long long)ci * p.Cout + co) * KK;
            const T* gp = g + ((long long)b * p.Cout + co) * OHW;
            for (int a = a0; a < a1; ++a) {
                const T* gr = gp + (long long)(p.s * i + a - p.oy0) * p.OW + (p.s * j - p.ox0);
                const T* wr = wp + (p.K - 1 - a) * p.K + (p.K - 1);
                int c = c0;
                for (; c + 4 <= c1; c += 4) {
                    acc0 = fma(wr[-c], gr[c], acc0);
                    acc1 = fma(wr[-c - 1], gr[c + 1], acc1);
                    acc2 = fma(wr[-c - 2], gr[c + 2], acc2);
                    acc3 = fma(wr[-c - 3], gr[c + 3], acc3);
                }
                for (; c < c1; ++c) acc0 = fma(wr[-c], gr[c], acc0);
            }
        }
        gx[idx] = (acc0 + acc1) + (acc2 + acc3);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void deconv_wgrad_kernel(dg_params p, const T* __restrict__ x, const T* __restrict__ g,
                                                           T* __restrict__ ws) {
    __shared__ T red[4];
    const int slab = blockIdx.y;
    T* out = ws + (long long)slab * p.S;
    const long long OHW = (long long)p.OH * p.OW;
    if ((int)blockIdx.x >= p.nblkW) {
        // ---- db: one output channel, this slab's share of the window's pixels ----
        const int co = blockIdx.x - p.nblkW;
        const long long NP = (long long)p.B * OHW;
        const long long q0 = min(NP, (long long)slab * p.pps), q1 = min(NP, q0 + p.pps);
        T sum = 0;
        for (long long q = q0 + threadIdx.x; q < q1; q += 256)
            sum += g[((q / OHW) * p.Cout + co) * OHW + q % OHW];
        sum = wave_sum(sum);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
        __syncthreads();
        if (threadIdx.x == 0) out[p.nW + co] = ((red[0] + red[1]) + red[2]) + red[3];
        return;
    }
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.nW) return;
    const int KK = p.K * p.K;
    const int tap = (int)(idx % KK), co = (int)((idx / KK) % p.Cout), ci = (int)(idx / ((long long)KK * p.Cout));
    const int a = p.K - 1 - tap / p.K, c = p.K - 1 - tap % p.K;         // offsets inside `full` of this tap
    // input columns j whose s j + c lies in the window's columns
    const int lo = p.ox0 - c, hi = p.ox0 + p.OW - c;                    // lo <= s j < hi
    const int j0 = lo <= 0 ? 0 : (lo + p.s - 1) / p.s;
    const int j1 = hi <= 0 ? 0 : min(p.W, (hi + p.s - 1) / p.s);
    const int r0 = slab * p.rps, r1 = min(p.B * p.H, r0 + p.rps);
    T acc0 = 0, acc1 = 0, acc2 = 0, acc3 = 0;                            // four chains in flight, as in dgrad
    for (int r = r0; r < r1; ++r) {
        const int b = r / p.H, i = r % p.H;
        const int y = p.s * i + a - p.oy0;
        if (y < 0 || y >= p.OH) continue;
        const T* xr = x + (((long long)b * p.Cin + ci) * p.H + i) * p.W;
        const T* gr = g + (((long long)b * p.Cout + co) * p.OH + y) * p.OW + (c - p.ox0);
        int j = j0;
        for (; j + 4 <= j1; j += 4) {
            acc0 = fma(xr[j], gr[p.s * j], acc0);
            acc1 = fma(xr[j + 1], gr[p.s * (j + 1)], acc1);
            acc2 = fma(xr[j + 2], gr[p.s * (j + 2)], acc2);
            acc3 = fma(xr[j + 3], gr[p.s * (j + 3)], acc3);
        }
        for (; j < j1; ++j) acc0 = fma(xr[j], gr[p.s * j], acc0);
    }
    out[idx] = (acc0 + acc1) + (acc2 + acc3);
}

template <typename T>
__global__ __launch_bounds__(256) void deconv_wgrad_finalize_kernel(const T* __restrict__ ws, int nslab, long long S,
                                                                    long long nW, T* __restrict__ dW, T* __restrict__ db) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= S) return;
    double v = 0.0;
    for (int k = 0; k < nslab; ++k) v += (double)ws[(long long)k * S + idx];
    if (idx < nW) dW[idx] = (T)v;
    else if (db) db[idx - nW] = (T)v;
}

int dg_plan(const iiseg_deconv_desc* d, dg_params& p) {
    if (!d) return IISEG_ERR_NULL;
    if (d->B <= 0 || d->Cin <= 0 || d->H <= 0 || d->W <= 0 || d->Cout <= 0 || d->K <= 0 || d->stride <= 0 ||
        d->OH <= 0 || d->OW <= 0 || d->oy0 < 0 || d->ox0 < 0)
        return IISEG_ERR_SHAPE;
    if (d->B > 65535 || d->Cin > 65535 || d->Cout > 65535 || d->K > 1024 || d->stride > 1024 ||
        (int64_t)d->H * d->W > (int64_t)1 << 30)
        return IISEG_ERR_SHAPE;
    const int64_t fullH = (int64_t)(d->H - 1) * d->stride + d->K, fullW = (int64_t)(d->W - 1) * d->stride + d->K;
    if (fullH > (int64_t)1 << 30 || fullW > (int64_t)1 << 30) return IISEG_ERR_SHAPE;
    if ((int64_t)d->oy0 + d->OH > fullH || (int64_t)d->ox0 + d->OW > fullW) return IISEG_ERR_SHAPE;
    if ((int64_t)d->OH * d->OW > (int64_t)1 << 30 || (int64_t)d->B * d->H > (int64_t)1 << 30) return IISEG_ERR_SHAPE;
    const int64_t nW = (int64_t)d->Cin * d->Cout * d->K * d->K;
    if (nW > ((int64_t)1 << 31) - 1) return IISEG_ERR_SHAPE;
    p.B = d->B; p.Cin = d->Cin; p.H = d->H; p.W = d->W; p.Cout = d->Cout; p.K = d->K; p.s = d->stride;
    p.oy0 = d->oy0; p.ox0 = d->ox0; p.OH = d->OH; p.OW = d->OW;
    p.nW = nW; p.S = nW + d->Cout;
    p.nblkW = (int)((nW + 255) / 256);
    const int rows = d->B * d->H;
    int want = p.nblkW >= TARGET_WORKGROUPS ? 1 : (TARGET_WORKGROUPS + p.nblkW - 1) / p.nblkW;
    if (want > rows) want = rows;
    p.rps = (rows + want - 1) / want;
    p.nslab = (rows + p.rps - 1) / p.rps;
    const long long NP = (long long)d->B * d->OH * d->OW;
    p.pps = (NP + p.nslab - 1) / p.nslab;
    return IISEG_OK;
}

template <typename T>
int dgrad_run(void* stream, const iiseg_deconv_desc* d, const T* g, const T* w, T* gx) {
    dg_params p;
    if (int st = dg_plan(d, p)) return st;
    if (!g || !w || !gx) return IISEG_ERR_NULL;
    const long long n = (long long)p.B * p.Cin * p.H * p.W;
    long long blocks = (n + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    IISEG_LAUNCH(deconv_dgrad_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, w, gx);
    return iiseg_check_launch();
}

template <typename T>
int wgrad_run(void* stream, const iiseg_deconv_desc* d, const T* x, const T* g, T* ws, T* dW, T* db) {
    dg_params p;
    if (int st = dg_plan(d, p)) return st;
    if (!x || !g || !ws || !dW) return IISEG_ERR_NULL;
    hipStream_t s = (hipStream_t)stream;
    IISEG_LAUNCH(deconv_wgrad_kernel<T>, dim3((unsigned)(p.nblkW + (db ? p.Cout : 0)), (unsigned)p.nslab), dim3(256), 0,
                 s, p, x, g, ws);
    IISEG_LAUNCH(deconv_wgrad_finalize_kernel<T>, dim3((unsigned)((p.S + 255) / 256)), dim3(256), 0, s, (const T*)ws,
                 p.nslab, p.S, p.nW, dW, db);
    return iiseg_check_launch();
}

}  // namespace

extern "C" int iiseg_deconv_wgrad_partials(const iiseg_deconv_desc* d) {
    dg_params p;
    if (int st = dg_plan(d, p)) return st;
    return p.nslab;
}
extern "C" int iiseg_deconv_dgrad_f32(void* stream, const iiseg_deconv_desc* d, const float* g, const float* w,
                                      float* gx) {
    return dgrad_run<float>(stream, d, g, w, gx);
}
extern "C" int iiseg_deconv_dgrad_f64(void* stream, const iiseg_deconv_desc* d, const double* g, const double* w,
                                      double* gx) {
    return dgrad_run<double>(stream, d, g, w, gx);
}
extern "C" int iiseg_deconv_wgrad_f32(void* stream, const iiseg_deconv_desc* d, const float* x, const float* g,
                                      float* ws, float* dW, float* db) {
    return wgrad_run<float>(stream, d, x, g, ws, dW, db);
}
extern "C" int iiseg_deconv_wgrad_f64(void* stream, const iiseg_deconv_desc* d, const double* x, const double* g,
                                      double* ws, double* dW, double* db) {
    return wgrad_run<double>(stream, d, x, g, ws, dW, db);
}
