// What the zero-padded 3x3 weight-gradient kernels share (conv_wgrad.hip: float / double; conv_wgrad_bf16.hip's two
// forms: bf16 operands): the launch parameters, the plan of pixel tiles and slabs, the border pixels of a wide zero
// padding and the finalize launch that adds the slabs in slab order.
#pragma once
#include "mma16_common.h"

namespace {

struct cw_params {
    int B, Cin, Cout, H, W, pad, OH, OW;
    int ay0, ax0, AH, AW;          // active region of the output map: pixels whose patch meets the real input
    int tilesX, tilesY;
    long long T;                   // pixel tiles in all: B * tilesY * tilesX
    int tps, nslab;                // tiles per slab, slabs
    long long so, sc;              // strides of dW
    int ci0;                       // first input channel in dW
    int want_db;
    long long S, nW;               // elements of one slab: nW = Cout Cin 9, S = nW + Cout
    long long nb, bps;             // border pixels per image, border pixels (of B nb) per slab
};

// pixel q of the border of one image (the map minus the active rectangle), rows first
__device__ inline void border_pixel(const cw_params& p, long long q, int& y, int& x) {
    const long long top = (long long)p.ay0 * p.OW, bottom = (long long)(p.OH - p.ay0 - p.AH) * p.OW;
    if (q < top) { y = (int)(q / p.OW); x = (int)(q % p.OW); return; }
    q -= top;
    if (q < bottom) { y = p.ay0 + p.AH + (int)(q / p.OW); x = (int)(q % p.OW); return; }
    q -= bottom;
    const int side = p.OW - p.AW;
    y = p.ay0 + (int)(q / side);
    const int c = (int)(q % side);
    x = c < p.ax0 ? c : c + p.AW;
}

// dW / db = the slabs added in slab order, in double
template <typename T>
__global__ __launch_bounds__(256) void conv_wgrad_finalize_kernel(const T* __restrict__ slab, int nslab, long long S,
                                                                  long long nW, int Cin, long long so, long long sc,
                                                                  int ci0, T* __restrict__ dW, T* __restrict__ db) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= S) return;
    double v = 0.0;
    for (int k = 0; k < nslab; ++k) v += (double)slab[(long long)k * S + idx];
    if (idx < nW) {
        const long long co = idx / ((long long)Cin * 9);
        const int rem = (int)(idx % ((long long)Cin * 9));
        dW[co * so + (long long)(ci0 + rem / 9) * sc + rem % 9] = (T)v;
    } else if (db) {
        db[idx - nW] = (T)v;
    }
}

// ---- host side ----
// The plan of a kernel with th x tw pixel tiles and cbo output x cbi input channel blocks: slabs of at least
// min_tps tiles, as many as bring the launch to target_wgs workgroups.
inline int cw_plan(const iiseg_conv_wgrad_desc* d, cw_params& p, int th, int tw, int cbo, int cbi, int min_tps,
                   int target_wgs) {
    if (!d) return IISEG_ERR_NULL;
    if (d->K != 3) return IISEG_ERR_SHAPE;
    if (d->B < 1 || d->B > 65535 || d->Cin < 1 || d->Cin > 65535 || d->Cout < 1 || d->Cout > 65535 || d->H < 1 ||
        d->W < 1 || d->pad < 0 || d->pad > 4096 || (int64_t)d->H * d->W > (int64_t)1 << 30)
        return IISEG_ERR_SHAPE;
    const int64_t OH = (int64_t)d->H + 2 * d->pad - 2, OW = (int64_t)d->W + 2 * d->pad - 2;
    if (OH < 1 || OW < 1 || OH * OW > (int64_t)1 << 30) return IISEG_ERR_SHAPE;
    if (!param_layout_ok(d->so, d->sc, d->ci0, d->Cin, d->Cin_tot, d->Cout, 9)) return IISEG_ERR_SHAPE;
    p.B = d->B; p.Cin = d->Cin; p.Cout = d->Cout; p.H = d->H; p.W = d->W; p.pad = d->pad;
    p.OH = (int)OH; p.OW = (int)OW;
    // output pixel y reads input rows y - pad .. y - pad + 2: it meets [0, H) for y in [pad - 2, H + pad)
    p.ay0 = d->pad > 2 ? d->pad - 2 : 0;
    p.ax0 = p.ay0;
    p.AH = (int)(OH < (int64_t)d->H + d->pad ? OH : (int64_t)d->H + d->pad) - p.ay0;
    p.AW = (int)(OW < (int64_t)d->W + d->pad ? OW : (int64_t)d->W + d->pad) - p.ax0;
    p.tilesY = (p.AH + th - 1) / th;
    p.tilesX = (p.AW + tw - 1) / tw;
    p.T = (long long)d->B * p.tilesY * p.tilesX;
    const long long blocks = (long long)((d->Cout + cbo - 1) / cbo) * ((d->Cin + cbi - 1) / cbi);
    int64_t tps;
    split_slabs(p.T, blocks, target_wgs, min_tps, &tps, &p.nslab);
    if (tps > ((long long)1 << 30)) return IISEG_ERR_SHAPE;
    p.tps = (int)tps;
    p.so = d->so; p.sc = d->sc; p.ci0 = d->ci0;
    p.nW = (long long)d->Cout * d->Cin * 9;
    p.S = p.nW + d->Cout;
    p.nb = (long long)p.OH * p.OW - (long long)p.AH * p.AW;
    const long long NB = p.nb * d->B;
    p.bps = (NB + p.nslab - 1) / p.nslab;
    p.want_db = 0;
    return IISEG_OK;
}
// ... with cb x cb channel blocks
inline int cw_plan(const iiseg_conv_wgrad_desc* d, cw_params& p, int th, int tw, int cb, int min_tps, int target_wgs) {
    return cw_plan(d, p, th, tw, cb, cb, min_tps, target_wgs);
}

}  // namespace
