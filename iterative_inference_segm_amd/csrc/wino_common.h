// The Winograd F(2x2, 3x3) core shared by conv_wino.hip (fp32), conv_wino_bf16.hip (bf16 operands) and
// conv_wino_f64.hip (float64): the three transform matrices, the tile grid of a windowed launch and the
// output placement.  A family keeps what really differs: its element type, the layout of U / V / M, how
// it loads its patches, its GEMMs and its epilogues.
//
// The arithmetic is written ONCE here because two properties of the hot path hang on it being the same
// everywhere: equal patches must give equal bits (DePool2D's equality masks, the pad-100 borders), and a
// windowed launch must reproduce the full-map launch bit for bit (tiles anchored at absolute output
// coordinates of a fixed parity).  Nothing in this header depends on how NaNs are honoured: the float64
// per-tile DePool2D selection, which uses NaN as its never-equal marker, stays in conv_wino_f64.hip.
// Device helpers take and return plain C arrays by reference (no ext_vector_type element stores indexed
// by an unrolled loop variable: DESIGN.md 3.12).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "iiseg.h"
#include "conv_common.h"

namespace iiseg {

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// ---- host: tile grid and output placement ---------------------------------------------------------
struct WinoTiles {
    int ty0, tx0, nty, ntx;   // first tile's output row / column (absolute), tile counts
    int64_t T;                // B * nty * ntx
};

// Descriptor validation common to the three families, then the tile grid of the window.  `kmult` is the
// family's channel-multiple requirement (1: none); it is checked HERE, between the window and the tile
// anchor, where every family checked it, so that each input keeps the status code it had.
inline int wino_tiles(const iiseg_conv_desc* d, WinoTiles& w, int kmult) {
    if (!d) return IISEG_ERR_NULL;
    if (d->KH != 3 || d->KW != 3 || d->dil != 1 || (d->flags & IISEG_CONV_TRANSPOSED2))
        return IISEG_ERR_UNSUPPORTED;
    if ((d->flags & IISEG_CONV_UNPOOL) && d->C2 != 0) return IISEG_ERR_UNSUPPORTED;
    if (d->B <= 0 || d->C1 <= 0 || d->C2 < 0 || d->H <= 0 || d->W <= 0 || d->Cout <= 0 ||
        d->pad < 0 || d->OH <= 0 || d->OW <= 0 || d->oy0 < 0 || d->ox0 < 0)
        return IISEG_ERR_SHAPE;
    const int fullH = d->H + 2 * d->pad - 2, fullW = d->W + 2 * d->pad - 2;
    if (d->oy0 + d->OH > fullH || d->ox0 + d->OW > fullW) return IISEG_ERR_SHAPE;
    if ((d->C1 + d->C2) % kmult) return IISEG_ERR_UNSUPPORTED;
    // tiles cover output rows r, r+1 with r = tile_y0 (mod 2): the first one is the last such row
    // at or before the window origin
    if ((d->tile_y0 | d->tile_x0) & ~1) return IISEG_ERR_SHAPE;
    w.ty0 = d->oy0 - ((d->oy0 - d->tile_y0) & 1);
    w.tx0 = d->ox0 - ((d->ox0 - d->tile_x0) & 1);
    w.nty = (d->oy0 + d->OH - w.ty0 + 1) >> 1;
    w.ntx = (d->ox0 + d->OW - w.tx0 + 1) >> 1;
    w.T = (int64_t)d->B * w.nty * w.ntx;
    return IISEG_OK;
}

// destination channel slice and planes of a params struct (dense: Cout channels, OH x OW planes)
template <typename P>
inline int wino_out_place(const iiseg_conv_desc* d, P& p) {
    p.out_ctot = d->out_ctot > 0 ? d->out_ctot : d->Cout;
    p.out_c0 = d->out_ctot > 0 ? d->out_c0 : 0;
    if (p.out_c0 < 0 || p.out_c0 + d->Cout > p.out_ctot) return IISEG_ERR_SHAPE;
    p.out_H = d->out_H > 0 ? d->out_H : d->OH;
    p.out_W = d->out_H > 0 ? d->out_W : d->OW;
    p.out_y0 = d->out_H > 0 ? d->out_y0 : 0;
    p.out_x0 = d->out_H > 0 ? d->out_x0 : 0;
    if (p.out_y0 < 0 || p.out_x0 < 0 || p.out_y0 + d->OH > p.out_H || p.out_x0 + d->OW > p.out_W)
        return IISEG_ERR_SHAPE;
    return IISEG_OK;
}

// ---- device: the three transforms -------------------------------------------------------------------
// Each is a pass over columns, then a pass over rows; the row pass is a function of ONE row, so that a
// kernel can store a row's results before it forms the next one (its live values stay few).  The
// expressions and their order are the ones every family had.

// t = G g, then one row of (G g) G^T -- in double whatever the family stores (the +-1/2 factors are exact)
__device__ __forceinline__ void wino_Gg(const double (&g)[3][3], double (&t)[4][3]) {
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        t[0][b] = g[0][b];
        t[1][b] = 0.5 * (g[0][b] + g[1][b] + g[2][b]);
        t[2][b] = 0.5 * (g[0][b] - g[1][b] + g[2][b]);
        t[3][b] = g[2][b];
    }
}
__device__ __forceinline__ void wino_tGt(const double (&t)[3], double (&u)[4]) {
    u[0] = t[0];
    u[1] = 0.5 * (t[0] + t[1] + t[2]);
    u[2] = 0.5 * (t[0] - t[1] + t[2]);
    u[3] = t[2];
}

// u[4a + b] = (G g G^T)[a][b], all 16 at once
__device__ __forceinline__ void wino_GgGt(const double (&g)[3][3], double (&u)[16]) {
    double t[4][3];
    wino_Gg(g, t);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        double r[4];
        wino_tGt(t[a], r);
#pragma unroll
        for (int b = 0; b < 4; ++b) u[a * 4 + b] = r[b];
    }
}

// e = B^T d, then one row of (B^T d) B
template <typename T>
__device__ __forceinline__ void wino_Btd(const T (&d)[4][4], T (&e)[4][4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        e[0][j] = d[0][j] - d[2][j];
        e[1][j] = d[1][j] + d[2][j];
        e[2][j] = d[2][j] - d[1][j];
        e[3][j] = d[1][j] - d[3][j];
    }
}
template <typename T>
__device__ __forceinline__ void wino_eB(const T (&e)[4], T (&v)[4]) {
    v[0] = e[0] - e[2];
    v[1] = e[1] + e[2];
    v[2] = e[2] - e[1];
    v[3] = e[1] - e[3];
}
// v[4i + j] = (B^T d B)[i][j], all 16 at once
template <typename T>
__device__ __forceinline__ void wino_BtdB(const T (&d)[4][4], T (&v)[16]) {
    T e[4][4];
    wino_Btd(d, e);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        T r[4];
        wino_eB(e[i], r);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[i * 4 + j] = r[j];
    }
}

// s = A^T m (m[4i + j] the product at transform point (i, j)), then one row of (A^T m) A
template <typename T>
__device__ __forceinline__ void wino_Atm(const T (&m)[16], T (&s)[2][4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const T m0 = m[j], m1 = m[4 + j], m2 = m[8 + j], m3 = m[12 + j];
        s[0][j] = m0 + m1 + m2;
        s[1][j] = m1 - m2 - m3;
    }
}
template <typename T>
__device__ __forceinline__ void wino_sA(const T (&s)[4], T (&y)[2]) {
    y[0] = s[0] + s[1] + s[2];
    y[1] = s[1] - s[2] - s[3];
}

// ---- device: the tile of a thread ------------------------------------------------------------------------
// tile t of a launch (t = (b * nty + tyl) * ntx + txl): its image and its first output row / column
struct WinoTile {
    int b, y, x;
    template <typename P>
    __device__ __forceinline__ WinoTile(const P& p, int t) {
        const int ntt = p.nty * p.ntx;
        b = t / ntt;
        const int r = t - b * ntt;
        const int tyl = r / p.ntx, txl = r - tyl * p.ntx;
        y = p.ty0 + 2 * tyl;
        x = p.tx0 + 2 * txl;
    }
};

}  // namespace iiseg
