// Weight and bias gradient of a 'valid' K x K stride-1 layer, 1 <= K <= 7, between 1 and 65535 channels (FCN-8's
// 7x7 fc6 and its 1x1 fc7 / score layers):
//
//   dW[co][ci0 + ci][ky][kx] = sum_{b,y,x} g_z[b][co][y][x] * x[b][ci][y + ky][x + kx]      0 <= ky, kx < K
//   db[co]                   = sum_{b,y,x} g_z[b][co][y][x]
//
// x is an (H, W) window of a larger map: element (b, ci, y, x) lies at b x_image + ci x_plane + (x_y0 + y) x_row +
// x_x0 + x, so the centre windows of pool4 / pool3 are read in place.  The sibling of conv_wgrad.hip: a GEMM with
// M = Cout, N = Cin K^2 and the reduction over the B OH OW output pixels, but K^2 accumulators of 16 registers do
// not fit at K = 7, so a workgroup owns (CB output channels) x (CB input channels) x ONE FILTER ROW ky (ky rides in
// the grid) and a SLAB of pixel tiles; per 64-pixel tile it stages g_z [pixel][co] and the rows y + ky of the x
// patch with their K - 1 halo columns [patch pixel][ci] in LDS once, and the K taps of the row read that one patch
// at compile-time offsets.  The tile is 4 x 16 pixels, or 8 x 8 for maps at most 8 wide (fc6's 7 x 7); K = 1 has no
// halo and takes 64 consecutive pixels of the flat (b, y, x) range (fc7 at B images of 1 x 1: one tile, not B).
//   float  : CB = 64, wave w owns the 32 x 32 sub-block (co half w & 1, ci half w >> 1); per pixel pair one
//            v_mfma_f32_32x32x2_f32 per tap (A = g_z: row co, k = pixel; B = x: k = pixel, column ci), K
//            accumulators of 16 registers.
//   double : CB = 32, plain vector-ALU FMAs (thread = one co x four ci x K taps); the parity leg.
// One slab: the block goes straight into dW.  More slabs: each workgroup writes its block into its slab of the
// workspace, and a finalize launch adds the slabs in slab order (in double).  db comes from the workgroups of the
// first input-channel block and filter row: the g_z values summed as they are read as the A operand.  No atomics:
// every sum has a fixed order, the same inputs give the same bits.
#include "mma16_common.h"

namespace {

constexpr int PIX = 64;                                  // output pixels per tile
constexpr int MIN_TILES_PER_SLAB = 4;
constexpr int TARGET_WORKGROUPS = 512;                   // two per CU
constexpr int KMAX = 7;

template <typename T> constexpr int chan_block() { return sizeof(T) == 4 ? 64 : 32; }

struct ck_params {
    int B, Cin, Cout, H, W, OH, OW;
    long long x_row, x_plane, x_image, x_org;   // strides of x and the offset of the window's first element
    int tilesX, tilesY;
    long long T;                   // pixel tiles in all: B * tilesY * tilesX
    int tps, nslab;                // tiles per slab, slabs
    int tw;                        // tile width: 16 (4 rows) or 8 (8 rows)
    long long so, sc;              // strides of dW
    int ci0;                       // first input channel in dW
    int want_db;
    long long S, nW;               // elements of one slab: nW = Cout Cin K^2, S = nW + Cout
};

template <typename T, int K, int TW>
__global__ __launch_bounds__(256, 2) void conv_wgrad_kxk_kernel(ck_params p, const T* __restrict__ x,
                                                                const T* __restrict__ gz, T* __restrict__ dst,
                                                                T* __restrict__ dbdst) {
    constexpr int CB = chan_block<T>();
    constexpr int LD = CB + 1;
    constexpr int TH = PIX / TW, PW = TW + K - 1, PPIX = TH * PW;
    __shared__ T gs[PIX * LD];
    __shared__ T xs[PPIX * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slab = blockIdx.x, co0 = blockIdx.y * CB;
    const int ky = blockIdx.z % K, cb0 = (blockIdx.z / K) * CB;
    const int nco = min(CB, p.Cout - co0), nci = min(CB, p.Cin - cb0);
    const bool do_db = p.want_db && blockIdx.z == 0;

    // channels past nco / nci are never staged: zero them once (their products are never stored either)
    for (int i = tid; i < PIX * LD; i += 256) gs[i] = 0;
    for (int i = tid; i < PPIX * LD; i += 256) xs[i] = 0;

    // ---- accumulators ----
    constexpr bool MFMA = sizeof(T) == 4;
    f32x16 acc[MFMA ? K : 1];
    T vacc[MFMA ? 1 : 4][MFMA ? 1 : K];
    if constexpr (MFMA) {
#pragma unroll
        for (int t = 0; t < K; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < K; ++t) vacc[j][t] = 0;
    }
    T asum = 0;                                                          // db: the A operand values of this lane
    // float: wave -> (co half, ci half), lane -> channel within the half and pixel of the pair
    const int cw = wave & 1, ciw = wave >> 1, l31 = lane & 31, half = lane >> 5;
    const bool wave_on = cw * 32 < nco && ciw * 32 < nci;                // wave-uniform
    // double: thread -> one co, four ci
    const int vco = tid >> 3, vci = (tid & 7) * 4;

    const long long t0 = (long long)slab * p.tps, t1 = min(p.T, t0 + p.tps);
    const int per_img = p.tilesY * p.tilesX;
    const long long OHW = (long long)p.OH * p.OW;
    int npix = PIX;                                                      // K = 1: pixels of this tile
    for (long long t = t0; t < t1; ++t) {
        __syncthreads();                                                 // the previous tile has been read
        if constexpr (K == 1) {
            // no halo: the tile is 64 consecutive pixels of the flat (b, y, x) range -- no partial tiles at the
            // map's edges, and the 1 x 1 maps of fc7 / score_fr at B images fill one tile instead of B
            const long long q0 = t * PIX, q = q0 + lane;
            npix = (int)min((long long)PIX, (long long)p.B * OHW - q0);
            const bool on = lane < npix;
            const long long b = on ? q / OHW : 0, r = on ? q % OHW : 0;
            const T* gp = gz + ((size_t)b * p.Cout + co0) * OHW + r;
            const T* xp = x + p.x_org + b * p.x_image + (long long)cb0 * p.x_plane + (r / p.OW) * p.x_row + r % p.OW;
            for (int c = wave; c < nco; c += 4) gs[lane * LD + c] = on ? gp[(size_t)c * OHW] : (T)0;
            for (int c = wave; c < nci; c += 4) xs[lane * LD + c] = on ? xp[(long long)c * p.x_plane] : (T)0;
        } else {
            const int b = (int)(t / per_img), rem = (int)(t % per_img);
            const int y0 = (rem / p.tilesX) * TH, x0 = (rem % p.tilesX) * TW;
            for (int idx = tid; idx < nco * PIX; idx += 256) {
                const int col = idx % TW, row = (idx / TW) % TH, c = idx / PIX;
                const int y = y0 + row, xx = x0 + col;
                T v = 0;
                if (y < p.OH && xx < p.OW)
                    v = gz[(((size_t)b * p.Cout + co0 + c) * p.OH + y) * p.OW + xx];
                gs[(row * TW + col) * LD + c] = v;
            }
            for (int idx = tid; idx < nci * PPIX; idx += 256) {
                const int pc = idx % PW, pr = (idx / PW) % TH, c = idx / PPIX;
                const int iy = y0 + ky + pr, ix = x0 + pc;
                T v = 0;
                if (iy < p.H && ix < p.W)
                    v = x[p.x_org + (long long)b * p.x_image + (long long)(cb0 + c) * p.x_plane + (long long)iy * p.x_row + ix];
                xs[(pr * PW + pc) * LD + c] = v;
            }
        }
        __syncthreads();
        if constexpr (MFMA) {
            if (wave_on) {
                const T* ga = gs + cw * 32 + l31 + half * LD;
                const T* xb = xs + ciw * 32 + l31 + half * LD;
#pragma unroll
                for (int s = 0; s < PIX / 2; ++s) {                      // pixel pair: columns c, c + 1 of row r
                    if (K == 1 && 2 * s >= npix) break;                  // wave-uniform: a short last tile
                    const int r = s / (TW / 2), c = 2 * (s % (TW / 2));
                    const float a = ga[(r * TW + c) * LD];
                    asum += a;
#pragma unroll
                    for (int kx = 0; kx < K; ++kx) {
                        const float bv = xb[(r * PW + c + kx) * LD];
                        acc[kx] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc[kx], 0, 0, 0);
                    }
                }
            }
        } else {
#pragma unroll 2
            for (int pix = 0; pix < npix; ++pix) {
                const int r = pix / TW, c = pix % TW;
                const T a = gs[pix * LD + vco];
                asum += a;
#pragma unroll
                for (int kx = 0; kx < K; ++kx) {
                    const T* xp = xs + (r * PW + c + kx) * LD + vci;
#pragma unroll
                    for (int j = 0; j < 4; ++j) vacc[j][kx] = fma(a, xp[j], vacc[j][kx]);
                }
            }
        }
    }

    // ---- the block's row of dW: into dW itself (one slab) or into this slab of the workspace ----
    T* out;
    long long so, sc;
    if (p.nslab == 1) { out = dst + (long long)p.ci0 * p.sc; so = p.so; sc = p.sc; }
    else { out = dst + (long long)slab * p.S; so = (long long)p.Cin * K * K; sc = K * K; }
    out += ky * K;
    if constexpr (MFMA) {
        if (wave_on) {
            const int ci = ciw * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = cw * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (co < nco && ci < nci) {
                    T* o = out + (long long)(co0 + co) * so + (long long)(cb0 + ci) * sc;
#pragma unroll
                    for (int kx = 0; kx < K; ++kx) o[kx] = acc[kx][r];
                }
            }
        }
    } else {
        if (vco < nco)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (vci + j < nci) {
                    T* o = out + (long long)(co0 + vco) * so + (long long)(cb0 + vci + j) * sc;
#pragma unroll
                    for (int kx = 0; kx < K; ++kx) o[kx] = vacc[j][kx];
                }
    }

    // ---- db: the A operand sums ----
    if (!do_db) return;                                                  // block-uniform
    T* dbo = p.nslab == 1 ? dbdst : dst + (long long)slab * p.S + p.nW;
    if constexpr (MFMA) {
        if (ciw == 0 && cw * 32 < nco) {
            const T v = asum + __shfl_xor(asum, 32, 64);                 // the two pixels of the pair
            const int co = cw * 32 + l31;
            if (half == 0 && co < nco) dbo[co0 + co] = v;
        }
    } else {
        if ((tid & 7) == 0 && vco < nco) dbo[co0 + vco] = asum;
    }
}

// dW / db = the slabs added in slab order, in double
template <typename T>
__global__ __launch_bounds__(256) void conv_wgrad_kxk_finalize_kernel(const T* __restrict__ slab, int nslab, long long S,
                                                                      long long nW, int Cin, int KK, long long so,
                                                                      long long sc, int ci0, T* __restrict__ dW,
                                                                      T* __restrict__ db) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= S) return;
    double v = 0.0;
    for (int k = 0; k < nslab; ++k) v += (double)slab[(long long)k * S + idx];
    if (idx < nW) {
        const long long co = idx / ((long long)Cin * KK);
        const int rem = (int)(idx % ((long long)Cin * KK));
        dW[co * so + (long long)(ci0 + rem / KK) * sc + rem % KK] = (T)v;
    } else if (db) {
        db[idx - nW] = (T)v;
    }
}

// ---- host side ----
template <typename T>
int ck_plan(const iiseg_conv_wgrad_kxk_desc* d, ck_params& p) {
    if (!d) return IISEG_ERR_NULL;
    if (d->K < 1 || d->K > KMAX) return IISEG_ERR_SHAPE;
    if (d->B < 1 || d->B > 65535 || d->Cin < 1 || d->Cin > 65535 || d->Cout < 1 || d->Cout > 65535 || d->H < d->K ||
        d->W < d->K || (int64_t)d->H * d->W > (int64_t)1 << 30)
        return IISEG_ERR_SHAPE;
    // the window of x inside its map: rows do not overlap, planes hold the window's rows, images the planes
    if (d->x_y0 < 0 || d->x_x0 < 0 || d->x_row < (int64_t)d->x_x0 + d->W ||
        d->x_plane < ((int64_t)d->x_y0 + d->H) * d->x_row || d->x_plane > (int64_t)1 << 40 ||
        d->x_image < (int64_t)d->Cin * d->x_plane || d->x_image > (int64_t)1 << 46)
        return IISEG_ERR_SHAPE;
    const int KK = d->K * d->K;
    if (!param_layout_ok(d->so, d->sc, d->ci0, d->Cin, d->Cin_tot, d->Cout, KK)) return IISEG_ERR_SHAPE;
    constexpr int CB = chan_block<T>();
    const long long ciB = (d->Cin + CB - 1) / CB, coB = (d->Cout + CB - 1) / CB;
    if (ciB * d->K > 65535) return IISEG_ERR_SHAPE;                      // grid z
    p.B = d->B; p.Cin = d->Cin; p.Cout = d->Cout; p.H = d->H; p.W = d->W;
    p.OH = d->H - d->K + 1; p.OW = d->W - d->K + 1;
    p.x_row = d->x_row; p.x_plane = d->x_plane; p.x_image = d->x_image;
    p.x_org = (long long)d->x_y0 * d->x_row + d->x_x0;
    p.tw = (p.OW <= 8 && d->K > 1) ? 8 : 16;
    const int th = PIX / p.tw;
    p.tilesY = (p.OH + th - 1) / th;
    p.tilesX = (p.OW + p.tw - 1) / p.tw;
    p.T = (long long)d->B * p.tilesY * p.tilesX;
    if (d->K == 1) p.T = ((long long)d->B * p.OH * p.OW + PIX - 1) / PIX;          // flat pixel tiles
    int64_t tps;
    split_slabs(p.T, coB * ciB * d->K, TARGET_WORKGROUPS, MIN_TILES_PER_SLAB, &tps, &p.nslab);
    if (tps > ((long long)1 << 30)) return IISEG_ERR_SHAPE;
    p.tps = (int)tps;
    p.so = d->so; p.sc = d->sc; p.ci0 = d->ci0;
    p.nW = (long long)d->Cout * d->Cin * KK;
    p.S = p.nW + d->Cout;
    p.want_db = 0;
    return IISEG_OK;
}

template <typename T, int K>
void ck_launch(hipStream_t s, const ck_params& p, const dim3& grid, const T* x, const T* gz, T* dst, T* db) {
    if constexpr (K > 1) {
        if (p.tw == 8) {
            IISEG_LAUNCH((conv_wgrad_kxk_kernel<T, K, 8>), grid, dim3(256), 0, s, p, x, gz, dst, db);
            return;
        }
    }
    IISEG_LAUNCH((conv_wgrad_kxk_kernel<T, K, 16>), grid, dim3(256), 0, s, p, x, gz, dst, db);
}

template <typename T>
int ck_run(void* stream, const iiseg_conv_wgrad_kxk_desc* d, const T* x, const T* gz, T* ws, T* dW, T* db) {
    ck_params p;
    if (int st = ck_plan<T>(d, p)) return st;
    if (!x || !gz || !dW || (p.nslab > 1 && !ws)) return IISEG_ERR_NULL;
    p.want_db = db != nullptr;
    constexpr int CB = chan_block<T>();
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)p.nslab, (unsigned)((p.Cout + CB - 1) / CB), (unsigned)(((p.Cin + CB - 1) / CB) * d->K));
    T* dst = p.nslab == 1 ? dW : ws;
    dispatch_k(d->K, [&](auto k) { ck_launch<T, decltype(k)::value>(s, p, grid, x, gz, dst, db); });
    if (p.nslab > 1)
        IISEG_LAUNCH(conv_wgrad_kxk_finalize_kernel<T>, dim3((unsigned)((p.S + 255) / 256)), dim3(256), 0, s,
                     (const T*)ws, p.nslab, p.S, p.nW, p.Cin, d->K * d->K, p.so, p.sc, p.ci0, dW, db);
    return iiseg_check_launch();
}

template <typename T>
int ck_slabs(const iiseg_conv_wgrad_kxk_desc* d) {
    ck_params p;
    if (int st = ck_plan<T>(d, p)) return st;
    return p.nslab;
}

}  // namespace

extern "C" int iiseg_conv_wgrad_kxk_check(const iiseg_conv_wgrad_kxk_desc* d) {
    ck_params p;
    return ck_plan<float>(d, p);
}
extern "C" int iiseg_conv_wgrad_kxk_slabs(const iiseg_conv_wgrad_kxk_desc* d, int32_t elem_bytes) {
    if (elem_bytes == 4) return ck_slabs<float>(d);
    if (elem_bytes == 8) return ck_slabs<double>(d);
    return d ? IISEG_ERR_SHAPE : IISEG_ERR_NULL;
}
extern "C" int64_t iiseg_conv_wgrad_kxk_workspace_elems(const iiseg_conv_wgrad_kxk_desc* d, int32_t elem_bytes) {
    const int n = iiseg_conv_wgrad_kxk_slabs(d, elem_bytes);
    if (n < 0) return n;
    return n == 1 ? 0 : (int64_t)n * ((int64_t)d->Cout * d->Cin * d->K * d->K + d->Cout);
}
extern "C" int iiseg_conv_wgrad_kxk_f32(void* stream, const iiseg_conv_wgrad_kxk_desc* d, const float* x,
                                        const float* gz, float* ws, float* dW, float* db) {
    return ck_run<float>(stream, d, x, gz, ws, dW, db);
}
extern "C" int iiseg_conv_wgrad_kxk_f64(void* stream, const iiseg_conv_wgrad_kxk_desc* d, const double* x,
                                        const double* gz, double* ws, double* dW, double* db) {
    return ck_run<double>(stream, d, x, gz, ws, dW, db);
}
