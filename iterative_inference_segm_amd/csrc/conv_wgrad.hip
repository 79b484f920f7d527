// Weight and bias gradient of a zero-padded 3x3 stride-1 layer between 1 and 65535 channels (the layers of the
// standard pool / unpool DAE):
//
//   dW[co][ci0 + ci][ky][kx] = sum_{b,y,x} g_z[b][co][y][x] * xpad[b][ci][y + ky][x + kx]
//   db[co]                   = sum_{b,y,x} g_z[b][co][y][x]
//
// It is a GEMM with M = Cout, N = 9 Cin and the reduction over the B OH OW output pixels.  A workgroup owns a
// (CB output channels) x (CB input channels) x 9 taps block of dW and a SLAB of pixel tiles; per 4 x 16 pixel tile
// it stages g_z [pixel][co] and the x patch with its halo [6 x 18 patch pixel][ci] in LDS once, and all nine
// taps read that one patch at compile-time offsets.
//   float  : CB = 64, wave w owns the 32 x 32 sub-block (co half w & 1, ci half w >> 1); per pixel pair one
//            v_mfma_f32_32x32x2_f32 per tap (A = g_z: row co, k = pixel; B = x: k = pixel, column ci), nine
//            accumulators of 16 registers.  The result is the k-ordered fmaf chain over the slab's pixels.
//   double : CB = 32, plain vector-ALU FMAs (thread = one co x four ci x nine taps); the parity leg.
// One slab: the block goes straight into dW.  More slabs: each workgroup writes its block into its slab of the
// workspace, and a finalize launch adds the slabs in slab order (in double).  db rides along: the active pixels'
// g_z values are summed as they are read as the A operand; pixels of a wide zero padding whose patch misses the
// real input (the pad-100 first layer) never reach the matrix pipe -- the workgroups of the first input-channel
// block add their slab's share of those to db straight from global memory.  No atomics: every sum has a fixed
// order, the same inputs give the same bits.
#include "conv_wgrad_common.h"

namespace {

constexpr int TH = 4, TW = 16, PIX = TH * TW;            // output pixel tile
constexpr int PH = TH + 2, PW = TW + 2, PPIX = PH * PW;  // its x patch
constexpr int MIN_TILES_PER_SLAB = 4;
constexpr int TARGET_WORKGROUPS = 512;                   // two per CU

template <typename T> constexpr int chan_block() { return sizeof(T) == 4 ? 64 : 32; }

typedef float f32x16 __attribute__((ext_vector_type(16)));

template <typename T>
__global__ __launch_bounds__(256, 2) void conv_wgrad_kernel(cw_params p, const T* __restrict__ x, const T* __restrict__ gz,
                                                         T* __restrict__ dst, T* __restrict__ dbdst) {
    constexpr int CB = chan_block<T>();
    constexpr int LD = CB + 1;
    __shared__ T gs[PIX * LD];
    __shared__ T xs[PPIX * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slab = blockIdx.x, co0 = blockIdx.y * CB, cb0 = blockIdx.z * CB;
    const int nco = min(CB, p.Cout - co0), nci = min(CB, p.Cin - cb0);
    const bool do_db = p.want_db && blockIdx.z == 0;

    // channels past nco / nci are never staged: zero them once (their products are never stored either)
    for (int i = tid; i < PIX * LD; i += 256) gs[i] = 0;
    for (int i = tid; i < PPIX * LD; i += 256) xs[i] = 0;

    // ---- accumulators ----
    constexpr bool MFMA = sizeof(T) == 4;
    f32x16 acc[MFMA ? 9 : 1];
    T vacc[MFMA ? 1 : 4][MFMA ? 1 : 9];
    if constexpr (MFMA) {
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < 9; ++t) vacc[j][t] = 0;
    }
    T asum = 0;                                                          // db: the A operand values of this lane
    // float: wave -> (co half, ci half), lane -> channel within the half and pixel of the pair
    const int cw = wave & 1, ciw = wave >> 1, l31 = lane & 31, half = lane >> 5;
    const bool wave_on = cw * 32 < nco && ciw * 32 < nci;                // wave-uniform
    // double: thread -> one co, four ci
    const int vco = tid >> 3, vci = (tid & 7) * 4;

    const long long t0 = (long long)slab * p.tps, t1 = min(p.T, t0 + p.tps);
    const int per_img = p.tilesY * p.tilesX;
    for (long long t = t0; t < t1; ++t) {
        const int b = (int)(t / per_img), rem = (int)(t % per_img);
        const int y0 = p.ay0 + (rem / p.tilesX) * TH, x0 = p.ax0 + (rem % p.tilesX) * TW;
        __syncthreads();                                                 // the previous tile has been read
        for (int idx = tid; idx < nco * PIX; idx += 256) {
            const int col = idx & (TW - 1), row = (idx >> 4) & (TH - 1), c = idx >> 6;
            const int y = y0 + row, xx = x0 + col;
            T v = 0;
            if (y < p.ay0 + p.AH && xx < p.ax0 + p.AW)
                v = gz[(((size_t)b * p.Cout + co0 + c) * p.OH + y) * p.OW + xx];
            gs[(row * TW + col) * LD + c] = v;
        }
        for (int idx = tid; idx < nci * PPIX; idx += 256) {
            const int pc = idx % PW, pr = (idx / PW) % PH, c = idx / PPIX;
            const int iy = y0 - p.pad + pr, ix = x0 - p.pad + pc;
            T v = 0;
            if (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W)
                v = x[(((size_t)b * p.Cin + cb0 + c) * p.H + iy) * p.W + ix];
            xs[(pr * PW + pc) * LD + c] = v;
        }
        __syncthreads();
        if constexpr (MFMA) {
            if (wave_on) {
                const T* ga = gs + cw * 32 + l31 + half * LD;
                const T* xb = xs + ciw * 32 + l31 + half * LD;
#pragma unroll
                for (int s = 0; s < PIX / 2; ++s) {                      // pixel pair: columns 2 (s & 7) + {0, 1} of row s >> 3
                    const int r = s >> 3, c = 2 * (s & 7);
                    const float a = ga[(r * TW + c) * LD];
                    asum += a;
#pragma unroll
                    for (int tap = 0; tap < 9; ++tap) {
                        const float bv = xb[((r + tap / 3) * PW + c + tap % 3) * LD];
                        acc[tap] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc[tap], 0, 0, 0);
                    }
                }
            }
        } else {
#pragma unroll 2
            for (int pix = 0; pix < PIX; ++pix) {
                const int r = pix >> 4, c = pix & (TW - 1);
                const T a = gs[pix * LD + vco];
                asum += a;
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const T* xp = xs + ((r + tap / 3) * PW + c + tap % 3) * LD + vci;
#pragma unroll
                    for (int j = 0; j < 4; ++j) vacc[j][tap] = fma(a, xp[j], vacc[j][tap]);
                }
            }
        }
    }

    // ---- the block of dW: into dW itself (one slab) or into this slab of the workspace ----
    T* out;
    long long so, sc;
    if (p.nslab == 1) { out = dst + (long long)p.ci0 * p.sc; so = p.so; sc = p.sc; }
    else { out = dst + (long long)slab * p.S; so = (long long)p.Cin * 9; sc = 9; }
    if constexpr (MFMA) {
        if (wave_on) {
            const int ci = ciw * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = cw * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (co < nco && ci < nci) {
                    T* o = out + (long long)(co0 + co) * so + (long long)(cb0 + ci) * sc;
#pragma unroll
                    for (int tap = 0; tap < 9; ++tap) o[tap] = acc[tap][r];
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
                    for (int tap = 0; tap < 9; ++tap) o[tap] = vacc[j][tap];
                }
    }

    // ---- db: active pixels (the A operand sums) + this slab's share of the border pixels ----
    if (!do_db) return;                                                  // block-uniform
    __syncthreads();                                                     // gs is free
    T* bsum = gs;                                                        // [CB]
    const long long NB = (long long)p.B * p.nb;
    const long long q0 = min(NB, (long long)slab * p.bps), q1 = min(NB, q0 + p.bps);
    for (int c = wave; c < nco; c += 4) {
        T s = 0;
        for (long long q = q0 + lane; q < q1; q += 64) {
            int y, xx;
            border_pixel(p, q % p.nb, y, xx);
            s += gz[(((size_t)(q / p.nb) * p.Cout + co0 + c) * p.OH + y) * p.OW + xx];
        }
        s = wave_sum(s);
        if (lane == 0) bsum[c] = s;
    }
    __syncthreads();
    T* dbo = p.nslab == 1 ? dbdst : dst + (long long)slab * p.S + p.nW;
    if constexpr (MFMA) {
        if (ciw == 0 && cw * 32 < nco) {
            const T v = asum + __shfl_xor(asum, 32, 64);                 // the two pixels of the pair
            const int co = cw * 32 + l31;
            if (half == 0 && co < nco) dbo[co0 + co] = v + bsum[co];
        }
    } else {
        if ((tid & 7) == 0 && vco < nco) dbo[co0 + vco] = asum + bsum[vco];
    }
}

// db alone, with the bits conv_wgrad_kernel<float> gives it for the same descriptor: for the modes that form dW
// elsewhere (wgrad='bf16' on FC-DenseNet) and must leave every db as it is.  It is that kernel
// without x and without the products: the same plan (so the slabs depend on Cin as there), the same values (zero
// outside the active region), the same two chains per output channel (even and odd columns, in tile order), the
// same border share, the slabs (here [slab][Cout]) added in slab order in double.  Only the staging differs: the
// g_z tiles of a slab come into LDS several at a time, [tile][pixel][co] with an odd channel stride, with eight
// loads per thread in flight.
constexpr int DB_LDS = 12288;                                            // floats: 48 KiB
constexpr int DB_UNROLL = 8, DB_THREADS = 1024;                          // sixteen waves load; two walk the chains

__global__ __launch_bounds__(DB_THREADS) void conv_wgrad_db_kernel(cw_params p, const float* __restrict__ gz,
                                                               float* __restrict__ dst) {
    constexpr int CB = chan_block<float>();
    __shared__ float gs[DB_LDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slab = blockIdx.x, co0 = blockIdx.y * CB;
    const int nco = min(CB, p.Cout - co0);
    const int LD = nco | 1, tile_ld = PIX * LD, K = DB_LDS / tile_ld;    // K >= 2: PIX * 65 = 4160 floats
    float asum = 0;
    const int cw = wave & 1, l31 = lane & 31, half = lane >> 5;
    const bool chain_on = wave < 2 && cw * 32 < nco;                     // that kernel's waves with ci half 0
    const int cc = min(cw * 32 + l31, nco - 1);                          // (a lane past nco: its sum is not stored)
    const long long t0 = (long long)slab * p.tps, t1 = min(p.T, t0 + p.tps);
    const int per_img = p.tilesY * p.tilesX;
    for (long long tb = t0; tb < t1; tb += K) {
        const int kt = (int)min((long long)K, t1 - tb), n = kt * nco * PIX;
        __syncthreads();                                                 // the previous tiles have been read
        for (int base = tid; base < n; base += DB_THREADS * DB_UNROLL) {
            float v[DB_UNROLL];
            int off[DB_UNROLL];
#pragma unroll
            for (int u = 0; u < DB_UNROLL; ++u) {
                const int idx = base + DB_THREADS * u;
                v[u] = 0;
                off[u] = -1;
                if (idx < n) {
                    const int tt = idx / (nco * PIX), r = idx - tt * (nco * PIX);
                    const int col = r & (TW - 1), row = (r >> 4) & (TH - 1), c = r >> 6;
                    const long long t = tb + tt;
                    const int b = (int)(t / per_img), rem = (int)(t % per_img);
                    const int y = p.ay0 + (rem / p.tilesX) * TH + row, xx = p.ax0 + (rem % p.tilesX) * TW + col;
                    off[u] = tt * tile_ld + (row * TW + col) * LD + c;
                    if (y < p.ay0 + p.AH && xx < p.ax0 + p.AW)
                        v[u] = gz[(((size_t)b * p.Cout + co0 + c) * p.OH + y) * p.OW + xx];
                }
            }
#pragma unroll
            for (int u = 0; u < DB_UNROLL; ++u)
                if (off[u] >= 0) gs[off[u]] = v[u];
        }
        __syncthreads();
        if (chain_on) {
            for (int tt = 0; tt < kt; ++tt) {
                const float* ga = gs + tt * tile_ld + cc + half * LD;
#pragma unroll
                for (int s = 0; s < PIX / 2; ++s) asum += ga[((s >> 3) * TW + 2 * (s & 7)) * LD];
            }
        }
    }
    __syncthreads();
    float* bsum = gs;
    const long long NB = (long long)p.B * p.nb;
    const long long q0 = min(NB, (long long)slab * p.bps), q1 = min(NB, q0 + p.bps);
    for (int c = wave; c < nco; c += DB_THREADS / 64) {        // (a channel is one wave's, whichever)
        float s = 0;
        for (long long q = q0 + lane; q < q1; q += 64) {
            int y, xx;
            border_pixel(p, q % p.nb, y, xx);
            s += gz[(((size_t)(q / p.nb) * p.Cout + co0 + c) * p.OH + y) * p.OW + xx];
        }
        s = wave_sum(s);
        if (lane == 0) bsum[c] = s;
    }
    __syncthreads();
    float* dbo = dst + (p.nslab == 1 ? 0 : (long long)slab * p.Cout);
    if (chain_on) {
        const float v = asum + __shfl_xor(asum, 32, 64);
        const int co = cw * 32 + l31;
        if (half == 0 && co < nco) dbo[co0 + co] = v + bsum[co];
    }
}

// db = the slabs added in slab order, in double (conv_wgrad_finalize_kernel's sum): a wave per channel brings the
// slabs' values into LDS with 64 loads in flight, one lane adds them in order.
constexpr int DB_FIN = 1024;

__global__ __launch_bounds__(64) void conv_wgrad_db_finalize_kernel(const float* __restrict__ slab, int nslab, int Cout,
                                                                    float* __restrict__ db) {
    __shared__ float v[DB_FIN];
    const int c = blockIdx.x, lane = threadIdx.x;
    double s = 0.0;
    for (int k0 = 0; k0 < nslab; k0 += DB_FIN) {
        const int n = min(DB_FIN, nslab - k0);
        __syncthreads();
        for (int k = lane; k < n; k += 64) v[k] = slab[(long long)(k0 + k) * Cout + c];
        __syncthreads();
        if (lane == 0)
            for (int k = 0; k < n; ++k) s += (double)v[k];
    }
    if (lane == 0) db[c] = (float)s;
}

// ---- host side ----
template <typename T>
int cw_plan(const iiseg_conv_wgrad_desc* d, cw_params& p) {
    return cw_plan(d, p, TH, TW, chan_block<T>(), MIN_TILES_PER_SLAB, TARGET_WORKGROUPS);
}

template <typename T>
int cw_run(void* stream, const iiseg_conv_wgrad_desc* d, const T* x, const T* gz, T* ws, T* dW, T* db) {
    cw_params p;
    if (int st = cw_plan<T>(d, p)) return st;
    if (!x || !gz || !dW || (p.nslab > 1 && !ws)) return IISEG_ERR_NULL;
    p.want_db = db != nullptr;
    constexpr int CB = chan_block<T>();
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)p.nslab, (unsigned)((p.Cout + CB - 1) / CB), (unsigned)((p.Cin + CB - 1) / CB));
    IISEG_LAUNCH(conv_wgrad_kernel<T>, grid, dim3(256), 0, s, p, x, gz, p.nslab == 1 ? dW : ws, db);
    if (p.nslab > 1)
        IISEG_LAUNCH(conv_wgrad_finalize_kernel<T>, dim3((unsigned)((p.S + 255) / 256)), dim3(256), 0, s, (const T*)ws,
                     p.nslab, p.S, p.nW, p.Cin, p.so, p.sc, p.ci0, dW, db);
    return iiseg_check_launch();
}

template <typename T>
int cw_slabs(const iiseg_conv_wgrad_desc* d) {
    cw_params p;
    if (int st = cw_plan<T>(d, p)) return st;
    return p.nslab;
}

}  // namespace

extern "C" int iiseg_conv_wgrad_check(const iiseg_conv_wgrad_desc* d) {
    cw_params p;
    return cw_plan<float>(d, p);
}
extern "C" int iiseg_conv_wgrad_slabs(const iiseg_conv_wgrad_desc* d, int32_t elem_bytes) {
    if (elem_bytes == 4) return cw_slabs<float>(d);
    if (elem_bytes == 8) return cw_slabs<double>(d);
    return d ? IISEG_ERR_SHAPE : IISEG_ERR_NULL;
}
extern "C" int64_t iiseg_conv_wgrad_workspace_elems(const iiseg_conv_wgrad_desc* d, int32_t elem_bytes) {
    const int n = iiseg_conv_wgrad_slabs(d, elem_bytes);
    if (n < 0) return n;
    return n == 1 ? 0 : (int64_t)n * ((int64_t)d->Cout * d->Cin * 9 + d->Cout);
}
extern "C" int iiseg_conv_wgrad_f32(void* stream, const iiseg_conv_wgrad_desc* d, const float* x, const float* gz,
                                    float* ws, float* dW, float* db) {
    return cw_run<float>(stream, d, x, gz, ws, dW, db);
}
extern "C" int iiseg_conv_wgrad_f64(void* stream, const iiseg_conv_wgrad_desc* d, const double* x, const double* gz,
                                    double* ws, double* dW, double* db) {
    return cw_run<double>(stream, d, x, gz, ws, dW, db);
}
extern "C" int64_t iiseg_conv_wgrad_db_workspace_elems(const iiseg_conv_wgrad_desc* d) {
    const int n = cw_slabs<float>(d);
    if (n < 0) return n;
    return n == 1 ? 0 : (int64_t)n * d->Cout;
}
extern "C" int iiseg_conv_wgrad_db_f32(void* stream, const iiseg_conv_wgrad_desc* d, const float* gz, float* ws,
                                       float* db) {
    cw_params p;
    if (int st = cw_plan<float>(d, p)) return st;
    if (!gz || !db || (p.nslab > 1 && !ws)) return IISEG_ERR_NULL;
    p.want_db = 1;
    hipStream_t s = (hipStream_t)stream;
    const int CB = chan_block<float>();
    const dim3 grid((unsigned)p.nslab, (unsigned)((p.Cout + CB - 1) / CB));
    IISEG_LAUNCH(conv_wgrad_db_kernel, grid, dim3(DB_THREADS), 0, s, p, gz, p.nslab == 1 ? db : ws);
    if (p.nslab > 1)
        IISEG_LAUNCH(conv_wgrad_db_finalize_kernel, dim3((unsigned)p.Cout), dim3(64), 0, s,
                     (const float*)ws, p.nslab, p.Cout, db);
    return iiseg_check_launch();
}
