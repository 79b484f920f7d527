// Weight and data gradient of a 'valid' K x K stride-1 layer, 1 <= K <= 7, with the products on the 16-bit matrix
// pipe (kxk='bf16': FCN-8's 7x7 fc6 and 1x1 fc7):
//
//   dW[co][ci0 + ci][ky][kx] = sum_{b,y,x}    bf16(g_z[b][co][y][x]) * bf16(x[b][ci][y + ky][x + kx])
//   db[co]                   = sum_{b,y,x}    g_z[b][co][y][x]                                    (not rounded)
//   gx[b][ci][y][x]          = sum_{co,ky,kx} bf16(W[co][ci0 + ci][ky][kx]) * bf16(g_z[b][co][y - ky][x - kx])
//
// and (fwd='bf16') the layer's forward itself, on the fp32 parameter as it is:
//
//   z[b][co][y][x]           = relu(sum_{ci,ky,kx} bf16(W[co][ci][ky][kx]) * bf16(x[b][ci][y + ky][x + kx]) + b[co])
//
// g_z (B, Cout, OH, OW) is zero outside its plane; x is an (H, W) = (OH + K - 1, OW + K - 1) window of a larger map
// and gx is (B, Cin, H, W).  Every operand arrives as fp32 and is rounded once, to nearest even, as it is staged; a
// product of two bf16 values is exact in fp32, v_mfma_f32_32x32x16_bf16 accumulates in fp32 in a fixed order, and
// the slabs of a split reduction are added in slab order by a second launch.  No atomics: the same inputs give the
// same bits.  Every load is at a clamped, always valid address and zero is selected when the value is stored, so
// the channels past Cout / Cin of the last k-tile contribute exactly nothing.
//
// Weight gradient.  The reduction runs over pixels, so an MFMA lane needs eight consecutive pixels of one channel
// as its eight k values.  The pixel range is cut into GROUPS of eight slots: for K > 1 eight consecutive columns of
// one output row (rows are padded to a multiple of eight slots; the groups of all rows and images follow each
// other, so a tile fills across image boundaries), for K = 1 eight consecutive pixels of the flat (b, y, x) range.
// LDS holds, per group, g_z as [group][co][8 slots] and the x row y + ky as [group][2][ci][8]: the sixteen columns
// from the group's first on.  The operand of tap kx is columns kx .. kx + 7 of those sixteen: for even kx four of
// the eight dwords the lane has read, for odd kx four v_alignbit_b32 of neighbours.  As in conv_wgrad_kxk.hip a
// workgroup owns 64 x 64 channels, ONE filter row ky (in the grid) and a slab of tiles of 16 groups; wave w the
// 32 x 32 sub-block (co half w & 1, ci half w >> 1) with K accumulators.  db: the staged, unrounded g_z values
// summed per thread, then over the sixteen threads of a channel in thread order; for K = 1 in the order of the
// float kernel of conv_wgrad_kxk.hip (FCN-8's fc7 keeps the bits of its db between the modes).
//
// Data gradient.  The reduction runs over output channels and taps.  A pack kernel rounds the layer's own fp32
// parameter (either layout, a channel slice) once into [k-tile of 16 co][tap][co chunk of 8][ci][8 co] bf16 -- the
// flip and the transpose are indices -- reading runs of the parameter and turning them in LDS.  A workgroup of the
// main kernel owns 64 input channels x a 16 x 16 pixel tile of one image (K = 1: 256 consecutive pixels of the flat
// range, no halo) x a SLAB of k-tiles; per k-tile it stages the g_z patch with its K - 1 halo once as
// [co chunk][patch pixel][8 co], per filter row the K taps of the filter image, loaded one row ahead into registers.
// Wave w owns tile rows 4w .. 4w + 3 as two 32-pixel blocks and both 32-channel blocks.  One slab: the epilogue
// adds what gx held (accumulate) and applies the gate (gx * [gate > 0]), in that order; more: the finalize does.
//
// Forward.  The reduction runs over (tap, 8-channel chunk) UNITS: a k-tile is NCH chunks of eight input channels x
// all K^2 taps, a k-step two consecutive units (the two k halves of the MFMA; the odd unit past the last multiplies a
// zero A fragment).  In 'oihw' the (ci, ky, kx) run of an output channel is contiguous, so the k-tile of W is read as
// 64 runs of 8 NCH K^2 floats straight from the parameter -- no packed image, nothing to refresh -- and turned while
// it is staged: the thread of (co, unit) gathers the unit's eight channels at stride K^2 and writes one 16-byte word
// of [co][unit].  A PIXEL TILE is 8 x 8 outputs of one image (K = 1: 64 consecutive pixels of the flat (b, y, x)
// range), its x patch with the K - 1 halo staged once per k-tile as [chunk][patch pixel][8 ci]: the B operand of a
// unit is one 16-byte read at the tap's offset.  A workgroup owns, for a slab of k-tiles, 64 output channels x eight
// pixel tiles (two per wave; K = 1, where nothing is re-used across taps: 128 output channels x four tiles, one per
// wave): eight accumulators per wave either way.  One slab: the epilogue adds the bias and applies ReLU; more: the
// slabs go to the workspace and the finalize adds them in slab order, then the bias, then ReLU.
#include "mma16_common.h"

namespace {

constexpr int CB = 64;                                   // channels of a workgroup (per side)
constexpr int KMAX = 7;

// ================================================ weight gradient ================================================
constexpr int GT = 16;                                   // groups of 8 pixel slots per tile: 8 k-steps
constexpr int W_MIN_TILES_PER_SLAB = 2;
constexpr int W_TARGET_WORKGROUPS = 512;

struct kw_params {
    int B, Cin, Cout, H, W, OH, OW;
    long long x_row, x_plane, x_image, x_org;
    int gpr;                       // K > 1: groups per output row
    unsigned P;                    // K = 1: pixels in all
    long long G, T;                // groups, tiles
    int tps, nslab;
    long long so, sc;
    int ci0, want_db;
    long long S, nW;
};

template <int K>
__global__ __launch_bounds__(256, 2) void conv_wgrad_kxk_bf16_kernel(kw_params p, const float* __restrict__ x,
                                                                     const float* __restrict__ gz,
                                                                     float* __restrict__ dst, float* __restrict__ dbdst) {
    constexpr int NP = K > 1 ? 2 : 1;                    // 8-column parts of an x row segment
    __shared__ __attribute__((aligned(16))) u32x4 As[GT * CB];
    __shared__ __attribute__((aligned(16))) u32x4 Bs[GT * NP * CB];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int slab = blockIdx.x, co0 = blockIdx.y * CB;
    const int ky = blockIdx.z % K, cb0 = (blockIdx.z / K) * CB;
    const int nco = min(CB, p.Cout - co0), nci = min(CB, p.Cin - cb0);
    const bool do_db = p.want_db && blockIdx.z == 0;
    // staging: thread -> (channel cs + 16 pass, group gi of the tile)
    const int cs = tid & 15, gi = tid >> 4;
    // multiplying: wave -> (co half, ci half), lane -> (channel of the half, k half)
    const int cw = wave & 1, ciw = wave >> 1, l31 = lane & 31, half = lane >> 5;
    const bool wave_on = cw * 32 < nco && ciw * 32 < nci;

    f32x16 acc[K];
#pragma unroll
    for (int t = 0; t < K; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    float dbsum[4] = {0.f, 0.f, 0.f, 0.f};

    const long long t0 = (long long)slab * p.tps, t1 = min(p.T, t0 + p.tps);
    const size_t OHW = (size_t)p.OH * p.OW;
    for (long long t = t0; t < t1; ++t) {
        const long long g = t * GT + gi;
        const bool gvalid = g < p.G;
        __syncthreads();                                                 // the previous tile has been read
        if constexpr (K > 1) {
            const long long gg = gvalid ? g : 0;
            const int xg = (int)(gg % p.gpr);
            const long long row = gg / p.gpr;
            const int y = (int)(row % p.OH), b = (int)(row / p.OH), c0 = xg * 8;
#pragma unroll
            for (int pass = 0; pass < 4; ++pass) {
                const int c = pass * 16 + cs;
                const float* gp = gz + (((size_t)b * p.Cout + min(co0 + c, p.Cout - 1)) * p.OH + y) * p.OW;
                float v[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = gp[min(c0 + i, p.OW - 1)];
                float s = 0.f;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    v[i] = gvalid && c < nco && c0 + i < p.OW ? v[i] : 0.f;
                    s += v[i];
                }
                dbsum[pass] += s;
                As[gi * CB + c] = pack8(v);
            }
#pragma unroll
            for (int pass = 0; pass < 4; ++pass) {
                const int c = pass * 16 + cs;
                const float* xp = x + p.x_org + (long long)b * p.x_image +
                                  (long long)min(cb0 + c, p.Cin - 1) * p.x_plane + (long long)(y + ky) * p.x_row;
                float v[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) v[i] = xp[min(c0 + i, p.W - 1)];
#pragma unroll
                for (int i = 0; i < 16; ++i) v[i] = gvalid && c < nci && c0 + i < p.W ? v[i] : 0.f;
                Bs[(gi * NP + 0) * CB + c] = pack8(v);
                Bs[(gi * NP + NP - 1) * CB + c] = pack8(v + 8 * (NP - 1));
            }
        } else {
            // no halo: eight consecutive pixels of the flat (b, y, x) range
            size_t go[8];
            long long xo[8];
            bool on[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const long long q = g * 8 + i;
                on[i] = gvalid && q < (long long)p.P;
                const unsigned qq = on[i] ? (unsigned)q : 0u;
                const unsigned b = qq / (unsigned)OHW, r = qq % (unsigned)OHW;
                go[i] = (size_t)b * p.Cout * OHW + r;
                xo[i] = p.x_org + (long long)b * p.x_image + (long long)(r / (unsigned)p.OW) * p.x_row + r % (unsigned)p.OW;
            }
#pragma unroll
            for (int pass = 0; pass < 4; ++pass) {
                const int c = pass * 16 + cs;
                const float* gp = gz + (size_t)min(co0 + c, p.Cout - 1) * OHW;
                const float* xp = x + (long long)min(cb0 + c, p.Cin - 1) * p.x_plane;
                float v[8], u[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) { v[i] = gp[go[i]]; u[i] = xp[xo[i]]; }
                float s = 0.f;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    v[i] = on[i] && c < nco ? v[i] : 0.f;
                    u[i] = on[i] && c < nci ? u[i] : 0.f;
                    s += v[i];
                }
                dbsum[pass] += s;
                As[gi * CB + c] = pack8(v);
                Bs[gi * CB + c] = pack8(u);
            }
        }
        __syncthreads();
        if (wave_on) {
            const int nks = (int)min((long long)(GT / 2), (p.G - t * GT + 1) / 2);   // k-steps with a real group
            const u32x4* ap = As + half * CB + cw * 32 + l31;
            const u32x4* bp = Bs + half * NP * CB + ciw * 32 + l31;
            for (int s = 0; s < nks; ++s) {
                const bf16x8 a = __builtin_bit_cast(bf16x8, ap[2 * s * CB]);
                const u32x4 d0 = bp[2 * s * NP * CB];
                u32x4 d1 = d0;
                if constexpr (NP == 2) d1 = bp[(2 * s * NP + 1) * CB];
                const unsigned d[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
#pragma unroll
                for (int kx = 0; kx < K; ++kx) {
                    const int j = kx >> 1;
                    u32x4 o;
                    if (kx & 1) {
                        o.x = __builtin_amdgcn_alignbit(d[j + 1], d[j], 16);
                        o.y = __builtin_amdgcn_alignbit(d[j + 2], d[j + 1], 16);
                        o.z = __builtin_amdgcn_alignbit(d[j + 3], d[j + 2], 16);
                        o.w = __builtin_amdgcn_alignbit(d[j + 4], d[j + 3], 16);
                    } else {
                        o.x = d[j]; o.y = d[j + 1]; o.z = d[j + 2]; o.w = d[j + 3];
                    }
                    acc[kx] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(bf16x8, o), acc[kx], 0, 0, 0);
                }
            }
        }
    }

    // ---- the block's row of dW: into dW itself (one slab) or into this slab of the workspace ----
    float* out;
    long long so, sc;
    if (p.nslab == 1) { out = dst + (long long)p.ci0 * p.sc; so = p.so; sc = p.sc; }
    else { out = dst + (long long)slab * p.S; so = (long long)p.Cin * K * K; sc = K * K; }
    out += ky * K;
    if (wave_on) {
        const int ci = ciw * 32 + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = cw * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (co < nco && ci < nci) {
                float* o = out + (long long)(co0 + co) * so + (long long)(cb0 + ci) * sc;
#pragma unroll
                for (int kx = 0; kx < K; ++kx) o[kx] = acc[kx][r];
            }
        }
    }

    if (!do_db) return;                                                  // block-uniform
    if constexpr (K == 1) {
        // ---- db in the order of conv_wgrad_kxk.hip's float kernel: the even and the odd pixels of the slab's flat
        // range in two running sums, then their sum -- with one slab in both kernels (fc7: always) the same bits ----
        if (tid < nco) {
            const long long q0 = t0 * GT * 8, q1 = min((long long)p.P, t1 * GT * 8);
            const float* gp = gz + (size_t)(co0 + tid) * OHW;
            unsigned b = (unsigned)q0 / (unsigned)OHW, r = (unsigned)q0 % (unsigned)OHW;
            float se = 0.f, so_ = 0.f;
            for (long long q = q0; q < q1; ++q) {
                const float v = gp[(size_t)b * p.Cout * OHW + r];
                if (q & 1) so_ += v; else se += v;
                if (++r == (unsigned)OHW) { r = 0; ++b; }
            }
            float* dbo = p.nslab == 1 ? dbdst : dst + (long long)slab * p.S + p.nW;
            dbo[co0 + tid] = se + so_;
        }
        return;
    }
    // ---- db: the sixteen threads of a channel, in thread order ----
    __syncthreads();
    float* red = reinterpret_cast<float*>(As);
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) red[(pass * 16 + cs) * 16 + gi] = dbsum[pass];
    __syncthreads();
    if (tid < nco) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) s += red[tid * 16 + i];
        float* dbo = p.nslab == 1 ? dbdst : dst + (long long)slab * p.S + p.nW;
        dbo[co0 + tid] = s;
    }
}

// dW / db = the slabs added in slab order, in double
__global__ __launch_bounds__(256) void conv_wgrad_kxk_bf16_finalize_kernel(const float* __restrict__ slab, int nslab,
                                                                           long long S, long long nW, int Cin, int KK,
                                                                           long long so, long long sc, int ci0,
                                                                           float* __restrict__ dW, float* __restrict__ db) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= S) return;
    double v = 0.0;
    for (int k = 0; k < nslab; ++k) v += (double)slab[(long long)k * S + idx];
    if (idx < nW) {
        const long long co = idx / ((long long)Cin * KK);
        const int rem = (int)(idx % ((long long)Cin * KK));
        dW[co * so + (long long)(ci0 + rem / KK) * sc + rem % KK] = (float)v;
    } else if (db) {
        db[idx - nW] = (float)v;
    }
}

int kw_plan(const iiseg_conv_wgrad_kxk_desc* d, kw_params& p) {
    if (!d) return IISEG_ERR_NULL;
    if (d->K < 1 || d->K > KMAX) return IISEG_ERR_SHAPE;
    if (d->B < 1 || d->B > 65535 || d->Cin < 1 || d->Cin > 65535 || d->Cout < 1 || d->Cout > 65535 || d->H < d->K ||
        d->W < d->K || (int64_t)d->H * d->W > (int64_t)1 << 30)
        return IISEG_ERR_SHAPE;
    if (d->x_y0 < 0 || d->x_x0 < 0 || d->x_row < (int64_t)d->x_x0 + d->W ||
        d->x_plane < ((int64_t)d->x_y0 + d->H) * d->x_row || d->x_plane > (int64_t)1 << 40 ||
        d->x_image < (int64_t)d->Cin * d->x_plane || d->x_image > (int64_t)1 << 46)
        return IISEG_ERR_SHAPE;
    const int KK = d->K * d->K;
    if (!param_layout_ok(d->so, d->sc, d->ci0, d->Cin, d->Cin_tot, d->Cout, KK)) return IISEG_ERR_SHAPE;
    const long long ciB = (d->Cin + CB - 1) / CB, coB = (d->Cout + CB - 1) / CB;
    if (ciB * d->K > 65535) return IISEG_ERR_SHAPE;                      // grid z
    p.B = d->B; p.Cin = d->Cin; p.Cout = d->Cout; p.H = d->H; p.W = d->W;
    p.OH = d->H - d->K + 1; p.OW = d->W - d->K + 1;
    const long long pix = (long long)d->B * p.OH * p.OW;
    if (pix > ((long long)1 << 31) - 16) return IISEG_ERR_SHAPE;
    p.x_row = d->x_row; p.x_plane = d->x_plane; p.x_image = d->x_image;
    p.x_org = (long long)d->x_y0 * d->x_row + d->x_x0;
    p.gpr = (p.OW + 7) / 8;
    p.P = (unsigned)pix;
    p.G = d->K == 1 ? (pix + 7) / 8 : (long long)d->B * p.OH * p.gpr;
    p.T = (p.G + GT - 1) / GT;
    int64_t tps;
    split_slabs(p.T, coB * ciB * d->K, W_TARGET_WORKGROUPS, W_MIN_TILES_PER_SLAB, &tps, &p.nslab);
    p.tps = (int)tps;
    p.so = d->so; p.sc = d->sc; p.ci0 = d->ci0;
    p.nW = (long long)d->Cout * d->Cin * KK;
    p.S = p.nW + d->Cout;
    p.want_db = 0;
    return IISEG_OK;
}

template <int K>
void kw_launch(hipStream_t s, const kw_params& p, const dim3& grid, const float* x, const float* gz, float* dst, float* db) {
    IISEG_LAUNCH((conv_wgrad_kxk_bf16_kernel<K>), grid, dim3(256), 0, s, p, x, gz, dst, db);
}

// ================================================= data gradient =================================================
constexpr int TH = 16, TW = 16;                          // output pixel tile
constexpr int KT = 16;                                   // output channels of a k-tile: one k-step, two chunks of 8
constexpr int PCB = 32;                                  // input channels of a pack workgroup
constexpr int D_TARGET_WORKGROUPS = 1024;
constexpr int D_MIN_KT_PER_SLAB = 2;

struct kd_params {
    int B, Cin, Cout, OH, OW, H, W;                      // g_z is (OH, OW), gx (H, W)
    int cin_pad, nkt;
    int tilesX, tilesY, ntile;
    int kps, nslab;                                      // k-tiles per slab, slabs
    unsigned P;                                          // K = 1: pixels in all
    int ci0, accumulate;
    long long so, sc;
    long long N;                                         // elements of gx
};

// The packed filter [k-tile][tap][chunk][cin_pad][8 co]: workgroup (ci block of PCB, k-tile), all K^2 taps.
__global__ __launch_bounds__(256) void conv_dgrad_kxk_bf16_pack_kernel(kd_params p, int KK, const float* __restrict__ Wp,
                                                                       u32x4* __restrict__ packed) {
    extern __shared__ __attribute__((aligned(16))) u32x4 img[];            // [tap][chunk][PCB] words of 8 co
    const int tid = threadIdx.x, cib0 = blockIdx.x * PCB, kt = blockIdx.y;
    const int n = PCB * KK;
    // consecutive threads walk the (ci, tap) run of a filter row; each gathers its sixteen output channels (sixteen
    // independent loads at clamped addresses, zero selected past Cout / Cin) into the two words of its (tap, ci)
    for (int idx = tid; idx < n; idx += 256) {
        const int ci = idx / KK, tap = idx % KK;
        const float* wsrc = Wp + (long long)(p.ci0 + min(cib0 + ci, p.Cin - 1)) * p.sc + tap;
        float v[KT];
#pragma unroll
        for (int j = 0; j < KT; ++j) v[j] = wsrc[(long long)min(kt * KT + j, p.Cout - 1) * p.so];
#pragma unroll
        for (int j = 0; j < KT; ++j) v[j] = cib0 + ci < p.Cin && kt * KT + j < p.Cout ? v[j] : 0.f;
        img[(tap * 2 + 0) * PCB + ci] = pack8(v);
        img[(tap * 2 + 1) * PCB + ci] = pack8(v + 8);
    }
    __syncthreads();
    const u32x4* src = img;
    for (int w = tid; w < KK * 2 * PCB; w += 256) {
        const int slice = w / PCB, ci = w % PCB;
        packed[((size_t)kt * KK * 2 + slice) * p.cin_pad + cib0 + ci] = src[w];
    }
}

template <int K>
__global__ __launch_bounds__(256, 2) void conv_dgrad_kxk_bf16_kernel(kd_params p, const float* __restrict__ gz,
                                                                     const u32x4* __restrict__ packed,
                                                                     const float* __restrict__ gate,
                                                                     float* __restrict__ dst) {
    constexpr int PH = TH + K - 1, PW = TW + K - 1, NPIX = PH * PW, KK = K * K;
    constexpr int GN = (NPIX + 255) / 256;               // patch pixels of a thread: tid + 256 j
    constexpr int WWORDS = K * 2 * CB, WN = (WWORDS + 255) / 256;
    __shared__ __attribute__((aligned(16))) u32x4 gs[2 * NPIX];          // [chunk][patch pixel]
    __shared__ __attribute__((aligned(16))) u32x4 ws[WWORDS];            // [kx][chunk][ci]
    const int tid = threadIdx.x, lane = tid & 63, sw = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nblk = p.cin_pad / CB;
    const int tile = blockIdx.x / nblk, cb0 = (blockIdx.x % nblk) * CB, slab = blockIdx.y;
    const int per_img = p.tilesY * p.tilesX;
    const int b = tile / per_img, rem = tile % per_img;
    const int y0 = (rem / p.tilesX) * TH, x0 = (rem % p.tilesX) * TW;   // K > 1
    const size_t OHW = (size_t)p.OH * p.OW;

    // the patch pixels of this thread: the offset of channel 0 (clamped into the map), and whether the pixel is real
    size_t go[GN];
    bool gin[GN];
#pragma unroll
    for (int j = 0; j < GN; ++j) {
        const int k = min(tid + 256 * j, NPIX - 1);
        if constexpr (K > 1) {
            const int y = y0 - (K - 1) + k / PW, xx = x0 - (K - 1) + k % PW;
            gin[j] = y >= 0 && y < p.OH && xx >= 0 && xx < p.OW;
            go[j] = (size_t)b * p.Cout * OHW + (size_t)min(max(y, 0), p.OH - 1) * p.OW + min(max(xx, 0), p.OW - 1);
        } else {
            const long long q = (long long)tile * NPIX + k;
            gin[j] = q < (long long)p.P;
            const unsigned qq = gin[j] ? (unsigned)q : 0u;
            go[j] = (size_t)(qq / (unsigned)OHW) * p.Cout * OHW + qq % (unsigned)OHW;
        }
    }

    const int l31 = lane & 31, half = lane >> 5;
    f32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

    const int kt0 = slab * p.kps, kt1 = min(p.nkt, kt0 + p.kps);
    u32x4 wv[WN];
    auto fetch = [&](int kt, int ky) {
        const u32x4* src = packed + ((size_t)kt * KK + ky * K) * 2 * p.cin_pad + cb0;
#pragma unroll
        for (int i = 0; i < WN; ++i) {
            const int w = min(tid + 256 * i, WWORDS - 1);
            wv[i] = src[(size_t)(w / CB) * p.cin_pad + w % CB];
        }
    };
    fetch(kt0, 0);
    for (int kt = kt0; kt < kt1; ++kt) {
        for (int ky = 0; ky < K; ++ky) {
            __syncthreads();                                             // the previous filter row has been read
#pragma unroll
            for (int i = 0; i < WN; ++i)
                if (tid + 256 * i < WWORDS) ws[tid + 256 * i] = wv[i];
            if (ky == 0) {
#pragma unroll
                for (int chunk = 0; chunk < 2; ++chunk) {
                    const int c0 = kt * KT + chunk * 8;
                    float gv[GN][8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const float* gp = gz + (size_t)min(c0 + i, p.Cout - 1) * OHW;
#pragma unroll
                        for (int j = 0; j < GN; ++j) gv[j][i] = gp[go[j]];
                    }
#pragma unroll
                    for (int j = 0; j < GN; ++j) {
#pragma unroll
                        for (int i = 0; i < 8; ++i) gv[j][i] = gin[j] && c0 + i < p.Cout ? gv[j][i] : 0.f;
                        if (tid + 256 * j < NPIX) gs[chunk * NPIX + tid + 256 * j] = pack8(gv[j]);
                    }
                }
            }
            __syncthreads();
            if (ky + 1 < K) fetch(kt, ky + 1);
            else if (kt + 1 < kt1) fetch(kt + 1, 0);
            // pixel (row 4 sw + 2 n + (l31 >> 4), column l31 & 15) of block n at the tap's offset: the flip
            const u32x4* gb = gs + half * NPIX + (4 * sw + (l31 >> 4) + K - 1 - ky) * PW + (l31 & 15) + K - 1;
            const u32x4* wa = ws + half * CB + l31;
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
                const bf16x8 a0 = __builtin_bit_cast(bf16x8, wa[kx * 2 * CB]);
                const bf16x8 a1 = __builtin_bit_cast(bf16x8, wa[kx * 2 * CB + 32]);
                const bf16x8 b0 = __builtin_bit_cast(bf16x8, gb[-kx]);
                const bf16x8 b1 = __builtin_bit_cast(bf16x8, gb[2 * PW - kx]);
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0][0], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc[1][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
    }

    // ---- epilogue: gx (+ what it held) (gated), or this slab of the workspace ----
    const bool direct = p.nslab == 1;
    float* out = direct ? dst : dst + (size_t)slab * p.N;
    const size_t HW = (size_t)p.H * p.W;
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int ty = 4 * sw + 2 * n + (l31 >> 4), tx = l31 & 15;
        size_t o0;                                                       // the pixel in channel 0 of its image
        if constexpr (K > 1) {
            if (y0 + ty >= p.H || x0 + tx >= p.W) continue;
            o0 = (size_t)b * p.Cin * HW + (size_t)(y0 + ty) * p.W + x0 + tx;
        } else {
            const long long q = (long long)tile * NPIX + ty * TW + tx;
            if (q >= (long long)p.P) continue;
            o0 = (size_t)((unsigned)q / (unsigned)HW) * p.Cin * HW + (unsigned)q % (unsigned)HW;
        }
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ci = cb0 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (ci >= p.Cin) continue;
                const size_t o = o0 + (size_t)ci * HW;
                float v = acc[m][n][r];
                if (direct) {
                    if (p.accumulate) v += out[o];
                    if (gate) v = gate[o] > 0.f ? v : 0.f;
                }
                out[o] = v;
            }
    }
}

// gx = the slabs added in slab order, in double (+ what gx held) (gated)
__global__ __launch_bounds__(256) void conv_dgrad_kxk_bf16_finalize_kernel(const float* __restrict__ slab, int nslab,
                                                                           long long N, int accumulate,
                                                                           const float* __restrict__ gate,
                                                                           float* __restrict__ gx) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= N) return;
    double v = 0.0;
    for (int k = 0; k < nslab; ++k) v += (double)slab[(long long)k * N + idx];
    if (accumulate) v += (double)gx[idx];
    float f = (float)v;
    if (gate) f = gate[idx] > 0.f ? f : 0.f;
    gx[idx] = f;
}

int kd_plan(const iiseg_conv_dgrad_desc* d, kd_params& p) {
    if (!d) return IISEG_ERR_NULL;
    if (d->K < 1 || d->K > KMAX) return IISEG_ERR_SHAPE;
    if (d->B < 1 || d->B > 65535 || d->Cin < 1 || d->Cin > 65535 || d->Cout < 1 || d->Cout > 65535 || d->H < 1 ||
        d->W < 1)
        return IISEG_ERR_SHAPE;
    const int KK = d->K * d->K;
    const int64_t H = (int64_t)d->H + d->K - 1, W = (int64_t)d->W + d->K - 1;
    if (H * W > (int64_t)1 << 28) return IISEG_ERR_SHAPE;
    if (!param_layout_ok(d->so, d->sc, d->ci0, d->Cin, d->Cin_tot, d->Cout, KK)) return IISEG_ERR_SHAPE;
    if (d->accumulate != 0 && d->accumulate != 1) return IISEG_ERR_SHAPE;
    p.B = d->B; p.Cin = d->Cin; p.Cout = d->Cout; p.OH = d->H; p.OW = d->W; p.H = (int)H; p.W = (int)W;
    p.cin_pad = (d->Cin + CB - 1) / CB * CB;
    p.nkt = (d->Cout + KT - 1) / KT;
    p.tilesY = (p.H + TH - 1) / TH;
    p.tilesX = (p.W + TW - 1) / TW;
    const int64_t pix = (int64_t)d->B * H * W;
    if (pix > ((int64_t)1 << 31) - 512) return IISEG_ERR_SHAPE;
    p.P = (unsigned)pix;
    const int64_t ntile = d->K == 1 ? (pix + TH * TW - 1) / (TH * TW) : (int64_t)d->B * p.tilesY * p.tilesX;
    const int64_t base = ntile * (p.cin_pad / CB);
    if (base > ((int64_t)1 << 31) - 1) return IISEG_ERR_SHAPE;
    p.ntile = (int)ntile;
    if (d->K == 1) { p.tilesY = 1; p.tilesX = (int)ntile; }              // one "image" of flat tiles
    int64_t kps;
    split_slabs(p.nkt, base, D_TARGET_WORKGROUPS, D_MIN_KT_PER_SLAB, &kps, &p.nslab);
    p.kps = (int)kps;
    p.ci0 = d->ci0; p.accumulate = d->accumulate;
    p.so = d->so; p.sc = d->sc;
    p.N = (long long)d->B * d->Cin * H * W;
    return IISEG_OK;
}

int64_t kd_pack_elems(const kd_params& p, int K) { return (int64_t)p.nkt * K * K * KT * p.cin_pad; }

template <int K>
void kd_launch(hipStream_t s, const kd_params& p, const dim3& grid, const float* gz, const u32x4* packed,
               const float* gate, float* dst) {
    IISEG_LAUNCH((conv_dgrad_kxk_bf16_kernel<K>), grid, dim3(256), 0, s, p, gz, packed, gate, dst);
}

// ==================================================== forward ====================================================
constexpr int FT = 8;                                    // output pixel tile edge (K > 1)
constexpr int FPX = FT * FT;                             // pixels of a tile: two 32-pixel MFMA blocks
constexpr int F_TARGET_WORKGROUPS = 512;
constexpr int F_MIN_KT_PER_SLAB = 2;

// A wave owns MB blocks of 32 output channels x TPW pixel tiles (eight accumulators either way): K = 1 stages no
// halo and re-uses nothing across taps, so its x tile serves 128 output channels; K > 1 gives a W tile 128 pixels.
constexpr int kf_mb(int K) { return K == 1 ? 4 : 2; }
constexpr int kf_tpw(int K) { return K == 1 ? 1 : 2; }
// chunks of eight input channels in a k-tile: K^2 NCH units
constexpr int kf_nch(int K) { return K == 1 ? 8 : K == 2 ? 4 : K == 3 ? 2 : 1; }
// units of W staged at a time (K = 7: the 49 taps in two parts, to keep LDS below 64 KiB)
constexpr int kf_ua(int K) { return K == 7 ? 26 : kf_nch(K) * K * K; }

struct kf_params {
    int B, Cin, Cout, H, W, OH, OW;
    int tilesX, tilesY;
    long long ntile;                                     // pixel tiles
    unsigned P;                                          // K = 1: pixels in all
    int nkt, kps, nslab;                                 // k-tiles, k-tiles per slab, slabs
    int relu;
    long long N;                                         // elements of z
};

template <int K>
__global__ __launch_bounds__(256, 2) void conv_fwd_kxk_bf16_kernel(kf_params p, const float* __restrict__ x,
                                                                   const float* __restrict__ Wp,
                                                                   const float* __restrict__ bias,
                                                                   float* __restrict__ dst) {
    constexpr int KK = K * K, NCH = kf_nch(K), NU = NCH * KK, UA = kf_ua(K);
    constexpr int MB = kf_mb(K), TPW = kf_tpw(K), CBF = 32 * MB, FWT = 4 * TPW;
    constexpr int PW = K > 1 ? FT + K - 1 : FPX, NPIX = K > 1 ? PW * PW : FPX;
    constexpr int AI = (CBF * UA + 255) / 256;           // (co, unit) items of a thread
    constexpr int BI = (FWT * NCH * NPIX + 255) / 256;   // (tile, chunk, patch pixel) items of a thread
    __shared__ __attribute__((aligned(16))) u32x4 As[CBF * UA];           // [co][unit of the part]
    __shared__ __attribute__((aligned(16))) u32x4 Bs[FWT * NCH * NPIX];   // [tile][chunk][patch pixel]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int co0 = blockIdx.y * CBF, slab = blockIdx.z;
    const int nco = min(CBF, p.Cout - co0);
    const size_t HW = (size_t)p.H * p.W, OHW = (size_t)p.OH * p.OW;
    const int per_img = p.tilesY * p.tilesX;

    // the patch pixels this thread stages: the offset of channel 0 (clamped into the map), the chunk, whether real
    size_t xo[BI];
    int xc[BI];
    bool xin[BI];
#pragma unroll
    for (int j = 0; j < BI; ++j) {
        const int it = min(tid + 256 * j, FWT * NCH * NPIX - 1);
        const int t = it / (NCH * NPIX), k = it % NPIX;
        xc[j] = (it / NPIX) % NCH;
        const long long tile = (long long)blockIdx.x * FWT + t;
        if constexpr (K > 1) {
            const long long tt = min(tile, p.ntile - 1);
            const int b = (int)(tt / per_img), rem = (int)(tt % per_img);
            const int y = (rem / p.tilesX) * FT + k / PW, xx = (rem % p.tilesX) * FT + k % PW;
            xin[j] = tile < p.ntile && y < p.H && xx < p.W;
            xo[j] = (size_t)b * p.Cin * HW + (size_t)min(y, p.H - 1) * p.W + min(xx, p.W - 1);
        } else {
            const long long q = tile * FPX + k;
            xin[j] = q < (long long)p.P;
            const unsigned qq = xin[j] ? (unsigned)q : 0u;
            xo[j] = (size_t)(qq / (unsigned)HW) * p.Cin * HW + qq % (unsigned)HW;
        }
    }

    // multiplying: wave -> TPW pixel tiles, lane -> (row of A / pixel of the 32-pixel block, k half)
    const int l31 = lane & 31, half = lane >> 5;
    const long long tile0 = (long long)blockIdx.x * FWT + wave * TPW;
    const bool wave_on = tile0 < p.ntile;
    int pb[2];                                           // the lane's pixel of block n inside the patch
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int pn = n * 32 + l31;
        pb[n] = K > 1 ? (pn / FT) * PW + pn % FT : pn;
    }
    f32x16 acc[MB][2 * TPW];
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
        for (int n = 0; n < 2 * TPW; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

    const int kt0 = slab * p.kps, kt1 = min(p.nkt, kt0 + p.kps);
    const long long so = (long long)p.Cin * KK;
    for (int kt = kt0; kt < kt1; ++kt) {
        const int cb = kt * NCH * 8;
#pragma unroll
        for (int ua = 0; ua < NU; ua += UA) {
            const int nu = min(UA, NU - ua);                             // units of this part
            __syncthreads();                                             // the previous part has been read
            // ---- W: the thread of (co, unit) gathers the unit's eight channels at the tap, rounds, one 16-byte write
#pragma unroll 2
            for (int j = 0; j < AI; ++j) {
                const int it = tid + 256 * j;
                const int itc = min(it, CBF * UA - 1);
                const int co = itc / UA, u = min(ua + itc % UA, NU - 1), chunk = u / KK, tap = u % KK;
                const float* wsrc = Wp + (long long)min(co0 + co, p.Cout - 1) * so + tap;
                const int c0 = cb + chunk * 8;
                float v[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = wsrc[(long long)min(c0 + i, p.Cin - 1) * KK];
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = co < nco && c0 + i < p.Cin ? v[i] : 0.f;
                if (it < CBF * UA) As[itc] = pack8(v);
            }
            // ---- x, with the k-tile's first part: the patches of the tiles, eight channels of a pixel per word ----
            if (ua == 0) {
#pragma unroll
                for (int j = 0; j < BI; ++j) {
                    const int c0 = cb + xc[j] * 8;
                    float v[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) v[i] = x[xo[j] + (size_t)min(c0 + i, p.Cin - 1) * HW];
#pragma unroll
                    for (int i = 0; i < 8; ++i) v[i] = xin[j] && c0 + i < p.Cin ? v[i] : 0.f;
                    if (tid + 256 * j < FWT * NCH * NPIX) Bs[tid + 256 * j] = pack8(v);
                }
            }
            __syncthreads();
            if (wave_on) {
                const u32x4* ap = As + l31 * UA;
                const u32x4* bp = Bs + wave * TPW * NCH * NPIX;
#pragma unroll 2
                for (int s = 0; s < (nu + 1) / 2; ++s) {
                    const int ul = 2 * s + half;
                    const int ulc = min(ul, nu - 1);                     // the odd unit past the last: A = 0
                    const int u = ua + ulc, chunk = u / KK, tap = u % KK;
                    const int off = chunk * NPIX + (tap / K) * PW + tap % K;
                    bf16x8 a[MB];
#pragma unroll
                    for (int m = 0; m < MB; ++m) {
                        u32x4 w = ap[m * 32 * UA + ulc];
                        if (ul >= nu) w = u32x4{0u, 0u, 0u, 0u};
                        a[m] = __builtin_bit_cast(bf16x8, w);
                    }
#pragma unroll
                    for (int n = 0; n < 2 * TPW; ++n) {
                        const bf16x8 b = __builtin_bit_cast(bf16x8, bp[(n >> 1) * NCH * NPIX + off + pb[n & 1]]);
#pragma unroll
                        for (int m = 0; m < MB; ++m)
                            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[m], b, acc[m][n], 0, 0, 0);
                    }
                }
            }
        }
    }

    // ---- epilogue: z = relu(sum + bias), or this slab of the workspace ----
    if (!wave_on) return;
    const bool direct = p.nslab == 1;
    float* out = direct ? dst : dst + (size_t)slab * p.N;
#pragma unroll
    for (int n = 0; n < 2 * TPW; ++n) {
        const long long tile = tile0 + (n >> 1);
        if (tile >= p.ntile) continue;
        const int pn = (n & 1) * 32 + l31;
        size_t o0;                                                       // the pixel in channel 0 of its image
        if constexpr (K > 1) {
            const int b = (int)(tile / per_img), rem = (int)(tile % per_img);
            const int y = (rem / p.tilesX) * FT + pn / FT, xx = (rem % p.tilesX) * FT + pn % FT;
            if (y >= p.OH || xx >= p.OW) continue;
            o0 = (size_t)b * p.Cout * OHW + (size_t)y * p.OW + xx;
        } else {
            const long long q = tile * FPX + pn;
            if (q >= (long long)p.P) continue;
            o0 = (size_t)((unsigned)q / (unsigned)OHW) * p.Cout * OHW + (unsigned)q % (unsigned)OHW;
        }
#pragma unroll
        for (int m = 0; m < MB; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (co >= nco) continue;
                float v = acc[m][n][r];
                if (direct) {
                    if (bias) v += bias[co0 + co];
                    if (p.relu) v = fmaxf(v, 0.f);
                }
                out[o0 + (size_t)(co0 + co) * OHW] = v;
            }
    }
}

// z = relu(the slabs added in slab order, in double, + bias)
__global__ __launch_bounds__(256) void conv_fwd_kxk_bf16_finalize_kernel(const float* __restrict__ slab, int nslab,
                                                                         long long N, long long OHW, int Cout,
                                                                         const float* __restrict__ bias, int relu,
                                                                         float* __restrict__ z) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= N) return;
    double v = 0.0;
    for (int k = 0; k < nslab; ++k) v += (double)slab[(long long)k * N + idx];
    float f = (float)v;
    if (bias) f += bias[(idx / OHW) % Cout];
    if (relu) f = fmaxf(f, 0.f);
    z[idx] = f;
}

int kf_plan(const iiseg_conv_fwd_kxk_desc* d, kf_params& p) {
    if (!d) return IISEG_ERR_NULL;
    if (d->K < 1 || d->K > KMAX) return IISEG_ERR_SHAPE;
    if (d->B < 1 || d->B > 65535 || d->Cin < 1 || d->Cin > 65535 || d->Cout < 1 || d->Cout > 65535 || d->H < d->K ||
        d->W < d->K || (int64_t)d->H * d->W > (int64_t)1 << 28)
        return IISEG_ERR_SHAPE;
    if (d->relu != 0 && d->relu != 1) return IISEG_ERR_SHAPE;
    const int KK = d->K * d->K;
    if ((int64_t)d->Cout * d->Cin * KK > ((int64_t)1 << 31) - 1) return IISEG_ERR_SHAPE;
    p.B = d->B; p.Cin = d->Cin; p.Cout = d->Cout; p.H = d->H; p.W = d->W;
    p.OH = d->H - d->K + 1; p.OW = d->W - d->K + 1;
    if ((int64_t)d->B * d->H * d->W > ((int64_t)1 << 31) - 512) return IISEG_ERR_SHAPE;
    const int64_t pix = (int64_t)d->B * p.OH * p.OW;
    p.P = (unsigned)pix;
    p.tilesY = (p.OH + FT - 1) / FT;
    p.tilesX = (p.OW + FT - 1) / FT;
    p.ntile = d->K == 1 ? (pix + FPX - 1) / FPX : (int64_t)d->B * p.tilesY * p.tilesX;
    const int fwt = 4 * kf_tpw(d->K), cbf = 32 * kf_mb(d->K);
    const int64_t groups = (p.ntile + fwt - 1) / fwt;
    if (groups > ((int64_t)1 << 31) - 1) return IISEG_ERR_SHAPE;
    const int64_t coB = (d->Cout + cbf - 1) / cbf;
    p.nkt = (d->Cin + kf_nch(d->K) * 8 - 1) / (kf_nch(d->K) * 8);
    int64_t kps;
    split_slabs(p.nkt, groups * coB, F_TARGET_WORKGROUPS, F_MIN_KT_PER_SLAB, &kps, &p.nslab);
    p.kps = (int)kps;
    if (p.nslab > 65535) return IISEG_ERR_SHAPE;                         // grid z
    p.relu = d->relu;
    p.N = (long long)d->B * d->Cout * p.OH * p.OW;
    return IISEG_OK;
}

template <int K>
void kf_launch(hipStream_t s, const kf_params& p, const dim3& grid, const float* x, const float* W, const float* bias,
               float* dst) {
    IISEG_LAUNCH((conv_fwd_kxk_bf16_kernel<K>), grid, dim3(256), 0, s, p, x, W, bias, dst);
}

}  // namespace

extern "C" int iiseg_conv_wgrad_kxk_bf16_check(const iiseg_conv_wgrad_kxk_desc* d) {
    kw_params p;
    return kw_plan(d, p);
}
extern "C" int iiseg_conv_wgrad_kxk_bf16_slabs(const iiseg_conv_wgrad_kxk_desc* d) {
    kw_params p;
    if (int st = kw_plan(d, p)) return st;
    return p.nslab;
}
extern "C" int64_t iiseg_conv_wgrad_kxk_bf16_workspace_elems(const iiseg_conv_wgrad_kxk_desc* d) {
    kw_params p;
    if (int st = kw_plan(d, p)) return st;
    return p.nslab == 1 ? 0 : (int64_t)p.nslab * p.S;
}
extern "C" int iiseg_conv_wgrad_kxk_bf16(void* stream, const iiseg_conv_wgrad_kxk_desc* d, const float* x,
                                         const float* gz, float* ws, float* dW, float* db) {
    kw_params p;
    if (int st = kw_plan(d, p)) return st;
    if (!x || !gz || !dW || (p.nslab > 1 && !ws)) return IISEG_ERR_NULL;
    if ((uintptr_t)x % 4 || (uintptr_t)gz % 4 || (uintptr_t)dW % 4 || (uintptr_t)db % 4 || (uintptr_t)ws % 4)
        return IISEG_ERR_ALIGN;
    p.want_db = db != nullptr;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)p.nslab, (unsigned)((p.Cout + CB - 1) / CB), (unsigned)(((p.Cin + CB - 1) / CB) * d->K));
    float* dst = p.nslab == 1 ? dW : ws;
    dispatch_k(d->K, [&](auto k) { kw_launch<decltype(k)::value>(s, p, grid, x, gz, dst, db); });
    if (p.nslab > 1)
        IISEG_LAUNCH(conv_wgrad_kxk_bf16_finalize_kernel, dim3((unsigned)((p.S + 255) / 256)), dim3(256), 0, s,
                     (const float*)ws, p.nslab, p.S, p.nW, p.Cin, d->K * d->K, p.so, p.sc, p.ci0, dW, db);
    return iiseg_check_launch();
}

extern "C" int iiseg_conv_dgrad_kxk_bf16_check(const iiseg_conv_dgrad_desc* d) {
    kd_params p;
    return kd_plan(d, p);
}
extern "C" int iiseg_conv_dgrad_kxk_bf16_slabs(const iiseg_conv_dgrad_desc* d) {
    kd_params p;
    if (int st = kd_plan(d, p)) return st;
    return p.nslab;
}
extern "C" int64_t iiseg_conv_dgrad_kxk_bf16_workspace_elems(const iiseg_conv_dgrad_desc* d) {
    kd_params p;
    if (int st = kd_plan(d, p)) return st;
    return p.nslab == 1 ? 0 : (int64_t)p.nslab * p.N;
}
extern "C" int64_t iiseg_conv_dgrad_kxk_bf16_pack_elems(const iiseg_conv_dgrad_desc* d) {
    kd_params p;
    if (int st = kd_plan(d, p)) return st;
    return kd_pack_elems(p, d->K);
}
extern "C" int iiseg_conv_dgrad_kxk_bf16_pack(void* stream, const iiseg_conv_dgrad_desc* d, const float* W, void* packed) {
    kd_params p;
    if (int st = kd_plan(d, p)) return st;
    if (!W || !packed) return IISEG_ERR_NULL;
    if ((uintptr_t)W % 4 || (uintptr_t)packed % 16) return IISEG_ERR_ALIGN;
    const int KK = d->K * d->K;
    const int64_t n = kd_pack_elems(p, d->K);
    if (ranges_overlap(W, (int64_t)d->Cout * d->Cin_tot * KK * 4, packed, n * 2)) return IISEG_ERR_UNSUPPORTED;
    IISEG_LAUNCH(conv_dgrad_kxk_bf16_pack_kernel, dim3((unsigned)(p.cin_pad / PCB), (unsigned)p.nkt), dim3(256),
                 (size_t)KK * 2 * PCB * 16, (hipStream_t)stream, p, KK, W, reinterpret_cast<u32x4*>(packed));
    return iiseg_check_launch();
}
extern "C" int iiseg_conv_dgrad_kxk_bf16(void* stream, const iiseg_conv_dgrad_desc* d, const float* gz, const void* packed,
                                         const float* gate, float* ws, float* gx) {
    kd_params p;
    if (int st = kd_plan(d, p)) return st;
    if (!gz || !packed || !gx || (p.nslab > 1 && !ws)) return IISEG_ERR_NULL;
    if ((uintptr_t)gz % 4 || (uintptr_t)gx % 4 || (uintptr_t)gate % 4 || (uintptr_t)ws % 4 || (uintptr_t)packed % 16)
        return IISEG_ERR_ALIGN;
    const int64_t gzb = (int64_t)d->B * d->Cout * d->H * d->W * 4, gxb = p.N * 4;
    // gx is written while other workgroups still read g_z and the filter image
    if (ranges_overlap(gx, gxb, gz, gzb) || ranges_overlap(gx, gxb, packed, kd_pack_elems(p, d->K) * 2)) return IISEG_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(p.ntile * (p.cin_pad / CB)), (unsigned)p.nslab);
    const u32x4* pk = reinterpret_cast<const u32x4*>(packed);
    float* dst = p.nslab == 1 ? gx : ws;
    dispatch_k(d->K, [&](auto k) { kd_launch<decltype(k)::value>(s, p, grid, gz, pk, gate, dst); });
    if (p.nslab > 1)
        IISEG_LAUNCH(conv_dgrad_kxk_bf16_finalize_kernel, dim3((unsigned)((p.N + 255) / 256)), dim3(256), 0, s,
                     (const float*)ws, p.nslab, p.N, p.accumulate, gate, gx);
    return iiseg_check_launch();
}

extern "C" int iiseg_conv_fwd_kxk_bf16_check(const iiseg_conv_fwd_kxk_desc* d) {
    kf_params p;
    return kf_plan(d, p);
}
extern "C" int iiseg_conv_fwd_kxk_bf16_slabs(const iiseg_conv_fwd_kxk_desc* d) {
    kf_params p;
    if (int st = kf_plan(d, p)) return st;
    return p.nslab;
}
extern "C" int64_t iiseg_conv_fwd_kxk_bf16_workspace_elems(const iiseg_conv_fwd_kxk_desc* d) {
    kf_params p;
    if (int st = kf_plan(d, p)) return st;
    return p.nslab == 1 ? 0 : (int64_t)p.nslab * p.N;
}
extern "C" int iiseg_conv_fwd_kxk_bf16(void* stream, const iiseg_conv_fwd_kxk_desc* d, const float* x, const float* W,
                                       const float* bias, float* ws, float* z) {
    kf_params p;
    if (int st = kf_plan(d, p)) return st;
    if (!x || !W || !z || (p.nslab > 1 && !ws)) return IISEG_ERR_NULL;
    if ((uintptr_t)x % 4 || (uintptr_t)W % 4 || (uintptr_t)bias % 4 || (uintptr_t)ws % 4 || (uintptr_t)z % 4)
        return IISEG_ERR_ALIGN;
    const int64_t zb = p.N * 4;
    // z is written while other workgroups still read x and W
    if (ranges_overlap(z, zb, x, (int64_t)d->B * d->Cin * d->H * d->W * 4) ||
        ranges_overlap(z, zb, W, (int64_t)d->Cout * d->Cin * d->K * d->K * 4))
        return IISEG_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const int fwt = 4 * kf_tpw(d->K), cbf = 32 * kf_mb(d->K);
    const dim3 grid((unsigned)((p.ntile + fwt - 1) / fwt), (unsigned)((p.Cout + cbf - 1) / cbf), (unsigned)p.nslab);
    float* dst = p.nslab == 1 ? z : ws;
    dispatch_k(d->K, [&](auto k) { kf_launch<decltype(k)::value>(s, p, grid, x, W, bias, dst); });
    if (p.nslab > 1)
        IISEG_LAUNCH(conv_fwd_kxk_bf16_finalize_kernel, dim3((unsigned)((p.N + 255) / 256)), dim3(256), 0, s,
                     (const float*)ws, p.nslab, p.N, (long long)p.OH * p.OW, p.Cout, bias, p.relu, z);
    return iiseg_check_launch();
}
