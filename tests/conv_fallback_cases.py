"""The cases of test_gpu_conv_fallbacks.py, and the kernel each of them takes: the table that
test_host_conv_dispatch.py checks on the host against the library's own dispatch
(include/iiseg.h, iiseg_conv_direct_kernel) and that the GPU test asserts again before it launches.

A case is one call of ops.Conv in float32 with fp32 matrix operands.  `route` = (family, BM, BN, pixel
tiles, channel tiles) of the direct kernel that runs it; for the rows of the im2col + split-K GEMM form
(`S` set) it is what the direct dispatch WOULD take, and `S` is the number of K slices, read from
iiseg_conv_gemm_workspace_elems = Tpad * (Kpad + S * Mpad)."""
import os
from collections import namedtuple

# include/iiseg.h: IISEG_CONV_KERNEL_*
SMALL, HALO, HALO16, TAPS, IGEMM = 1, 2, 3, 4, 5

Case = namedtuple('Case', 'name B C1 C2 H W Cout k pad dil relu transposed unpool window placed add route S')


def case(name, B, cin, hw, cout, k, route, pad=0, dil=1, relu=False, transposed=False, unpool=False,
         window=None, placed='slice', add=False, S=None):
    """cin: channels, or (C1, C2) of two sources.  hw: the logical input map (DePool2D input: the pre-pool
    size).  window: (oy0, ox0, OH, OW).  placed: 'slice' (a window of larger planes AND a channel slice of a
    wider tensor), 'plane' (larger planes only) or 'guard' (a dense tensor between guard bands: the GEMM form
    takes dense outputs only).  add: a skip-add larger than the window, read from its own offset."""
    C1, C2 = cin if isinstance(cin, tuple) else (cin, 0)
    return Case(name, B, C1, C2, hw[0], hw[1], cout, k, pad, dil, relu, transposed, unpool, window, placed, add,
                route, S)


IGEMM_CASES = [
    # 7x7 valid, K = 245 (11 zero k rows): one ragged pixel tile
    case('igemm-bm32-ragged-k', 2, 5, (15, 14), 24, 7, (IGEMM, 32, 256, 1, 1)),
    # 11 pixel tiles: a partial second group of 8, and 11 blocks over 8 XCDs
    case('igemm-bm64-11-ptiles', 3, 7, (31, 30), 40, 5, (IGEMM, 64, 256, 11, 1), pad=2, relu=True),
    # 2 channel tiles x 19 pixel tiles = 38 blocks, Cout 130 < Mpad 256
    case('igemm-bm128-38-blocks', 2, 6, (33, 35), 130, 7, (IGEMM, 128, 128, 19, 2), pad=3),
    # everything the GEMM form refuses at once: window with odd origin, placement, skip-add, ReLU
    case('igemm-bm128-window-add', 2, 16, (13, 12), 200, 7, (IGEMM, 128, 128, 1, 2), relu=True,
         window=(1, 1, 5, 4), add=True),
    case('igemm-bm64-two-sources-dil2', 2, (5, 6), (14, 13), 40, 5, (IGEMM, 64, 256, 1, 1), dil=2),
    # DePool2D input on an odd map: the UNPOOL instantiation of the 256- and the 128-pixel tile
    case('igemm-bm64-unpool', 2, 5, (13, 11), 40, 7, (IGEMM, 64, 256, 2, 1), pad=3, unpool=True),
    case('igemm-bm128-unpool', 2, 5, (13, 11), 130, 7, (IGEMM, 128, 128, 3, 2), pad=3, unpool=True, relu=True),
    case('igemm-bm32-unpool', 2, 5, (13, 11), 24, 7, (IGEMM, 32, 256, 2, 1), pad=3, unpool=True),
    # 1x1 output map: one pixel tile spanning 70 images
    case('igemm-bm64-70-images', 70, 3, (7, 7), 40, 7, (IGEMM, 64, 256, 1, 1)),
]

TAPS_CASES = [
    # ---- 1x1, Cin 70 -> Kpad 80: the last k-tile's channels 70..79 are clamped to channel 69
    # 1x1 map, 300 images: the buffer descriptor of a tile spans 256/1 + 2 = 258 images
    case('taps1x1-bm32-300-images', 300, 70, (1, 1), 11, 1, (TAPS, 32, 256, 2, 1), relu=True),
    # the score_pool4 pattern: window with odd origin + placement + skip-add
    case('taps1x1-bm64-window-add', 2, 70, (12, 11), 33, 1, (TAPS, 64, 256, 1, 1), window=(3, 1, 7, 6), add=True),
    # 10 pixel tiles x 2 channel tiles: a partial second group of 8 under two channel tiles, 20 blocks
    case('taps1x1-bm128-20-blocks', 3, 70, (19, 21), 130, 1, (TAPS, 128, 128, 10, 2)),
    # one 16-channel k-tile holds both sources (5 + 11 of the second), the next the second alone
    case('taps1x1-bm64-two-sources', 2, (5, 27), (9, 10), 33, 1, (TAPS, 64, 256, 1, 1), relu=True),
    # DePool2D input (Cin 20 -> Kpad 32, clamped channels again)
    case('taps1x1-bm32-unpool', 2, 20, (9, 11), 11, 1, (TAPS, 32, 256, 1, 1), unpool=True),
    case('taps1x1-bm64-unpool', 2, 20, (9, 11), 33, 1, (TAPS, 64, 256, 1, 1), unpool=True, relu=True),
    case('taps1x1-bm128-unpool', 2, 20, (9, 11), 130, 1, (TAPS, 128, 128, 2, 2), unpool=True),
    # ---- 3x3 off the halo kernels
    # the 256-channel 8-wave tile, Mpad 512
    case('taps3x3-bm256', 2, 6, (9, 10), 260, 3, (TAPS, 256, 128, 2, 2), pad=1),
    case('taps3x3-bm32-dil2', 2, 17, (11, 13), 24, 3, (TAPS, 32, 256, 2, 1), pad=2, dil=2),
    case('taps3x3-bm64-dil3', 2, 17, (11, 13), 40, 3, (TAPS, 64, 256, 1, 1), dil=3, relu=True),
    case('taps3x3-bm128-dil2', 2, 17, (11, 13), 130, 3, (TAPS, 128, 128, 3, 2), pad=2, dil=2),
    # (the halo kernel refuses C1 % 4 != 0: a 4-channel k-tile would straddle the sources)
    case('taps3x3-bm64-two-sources', 2, (6, 10), (10, 11), 40, 3, (TAPS, 64, 256, 1, 1), pad=1, relu=True),
    # DePool2D input on an odd map, 260 output channels: UNPOOL keeps to the 128-channel tile
    case('taps3x3-bm128-unpool', 2, 8, (9, 11), 260, 3, (TAPS, 128, 128, 2, 4), pad=1, unpool=True),
    # (dilated DePool2D layers: the halo kernels take dilation only up to 16 output channels)
    case('taps3x3-bm32-dil2-unpool', 2, 8, (9, 11), 24, 3, (TAPS, 32, 256, 1, 1), pad=2, dil=2, unpool=True),
    case('taps3x3-bm64-dil2-unpool', 2, 8, (9, 11), 40, 3, (TAPS, 64, 256, 1, 1), pad=2, dil=2, unpool=True,
         relu=True),
    # ---- transposed 3x3 stride 2 (FC-DenseNet's TransitionUp), 7x6 -> 15x13
    case('tconv3x3-bm32-full', 2, 20, (7, 6), 12, 3, (TAPS, 32, 256, 2, 1), transposed=True, placed='plane'),
    case('tconv3x3-bm64-odd-window', 2, 20, (7, 6), 48, 3, (TAPS, 64, 256, 1, 1), transposed=True,
         window=(1, 3, 11, 9)),
    case('tconv3x3-bm128-even-window-slice', 2, 20, (7, 6), 130, 3, (TAPS, 128, 128, 3, 2), transposed=True,
         window=(2, 0, 12, 12)),
    # ---- transposed 4x4 stride 2 (the DAE's unpool_type='standard'), 5x6 -> 12x14
    case('tconv4x4-bm32', 2, 9, (5, 6), 11, 4, (TAPS, 32, 128, 3, 1), transposed=True),
    case('tconv4x4-bm64', 2, 9, (5, 6), 40, 4, (TAPS, 64, 128, 2, 1), transposed=True, window=(1, 2, 10, 11)),
    # ---- the 4x4 tiles' UNPOOL instantiations: a plain (not transposed) 4x4 layer with DePool2D input
    case('taps4x4-bm32-unpool', 2, 6, (9, 11), 11, 4, (TAPS, 32, 128, 2, 1), pad=1, unpool=True),
    case('taps4x4-bm64-unpool', 2, 6, (9, 11), 40, 4, (TAPS, 64, 128, 2, 1), pad=1, unpool=True),
    case('taps4x4-bm128-unpool', 2, 6, (9, 11), 130, 4, (TAPS, 128, 128, 2, 2), pad=1, unpool=True, relu=True),
]

# B = 5 and a 7x10 output map: T = 350 is no multiple of 128 and takes two 256-thread blocks
GEMM_CASES = [
    # Kpad 608 > K 600, Mpad 128
    case('gemm-5x5-s2', 5, 24, (11, 14), 70, 5, (IGEMM, 128, 128, 3, 1), relu=True, placed='guard', S=2),
    # Kpad 2352, Mpad 256: both grid-stride loops idle, the longest K
    case('gemm-7x7-s7', 5, 48, (13, 16), 130, 7, (IGEMM, 128, 128, 3, 2), placed='guard', S=7),
    # the score_fr pattern: Cout far below Mpad 128, Kpad 1040 > K 1030
    case('gemm-1x1-s5', 5, 1030, (7, 10), 11, 1, (TAPS, 32, 256, 2, 4), relu=True, placed='guard', S=5),
    # Kpad 1968 > 1024 rows of the im2col grid, Cout 1100 > 1024 rows of the output grid
    case('gemm-7x7-grid-stride', 5, 40, (13, 16), 1100, 7, (IGEMM, 128, 128, 3, 9), placed='guard', S=1),
]

FALLBACK_CASES = IGEMM_CASES + TAPS_CASES + GEMM_CASES

# test_gpu_ops.py::CONV_CASES (dense, full map), and where each of them runs today
OPS_CONV_CASES = [
    case('ops-0', 2, 3, (17, 19), 11, 3, (HALO16, 16, 256, 6, 1), pad=1, placed=None),
    case('ops-1', 1, 11, (20, 20), 64, 3, (HALO, 64, 256, 4, 1), pad=5, relu=True, placed=None),
    case('ops-2', 3, 40, (13, 9), 130, 3, (HALO, 128, 128, 12, 2), pad=1, relu=True, placed=None),
    case('ops-3', 2, 16, (9, 9), 200, 7, (IGEMM, 128, 128, 1, 2), relu=True, placed=None, S=1),
    case('ops-4', 2, 70, (7, 7), 33, 1, (TAPS, 64, 256, 1, 1), relu=True, placed=None),
    case('ops-5', 1, 11, (40, 36), 11, 3, (SMALL, 16, 1024, 2, 1), dil=4, placed=None),
    case('ops-6', 1, 5, (300, 7), 12, 3, (HALO16, 16, 256, 38, 1), pad=1, placed=None),
]


def switches(c):
    """The environment switches a case's route depends on (all of them default to '1')."""
    names = set()
    if c.k == 3 and not c.transposed:
        names.add('IISEG_CONV_HALO')
        if c.Cout <= 16:
            names.add('IISEG_CONV_HALO16')
    if c.S is not None:
        names.add('IISEG_CONV_GEMM')
    if c.C1 + c.C2 <= 16 and c.Cout <= 16:
        names.add('IISEG_CONV_SMALL')
    return sorted(names)


def switched_off(c):
    """The name of a switch the environment moved off its default, if `c` depends on one."""
    for name in switches(c):
        if os.environ.get(name, '1') != '1':
            return name
    return None


def out_hw(c):
    if c.transposed:
        return (c.H - 1) * 2 + c.k, (c.W - 1) * 2 + c.k
    return c.H + 2 * c.pad - c.dil * (c.k - 1), c.W + 2 * c.pad - c.dil * (c.k - 1)


def geometry(c, placed=None):
    """The shapes and offsets of a case's call: {'x1', 'x2', 'pre', 'pooled', 'add', 'out': shapes or None;
    'add_off', 'window', 'place', 'out_c0'; 'win': the computed window (oy0, ox0, OH, OW)}.  `placed`
    overrides the case's own placement (None: a dense output)."""
    fh, fw = out_hw(c)
    win = c.window or (0, 0, fh, fw)
    OH, OW = win[2:]
    g = dict(x1=(c.B, c.C1, c.H, c.W), x2=None, pre=None, pooled=None, add=None, add_off=(0, 0),
             window=c.window, out=None, place=None, out_c0=None, win=win)
    if c.unpool:
        g.update(x1=(c.B, c.C1, c.H // 2, c.W // 2), pre=(c.B, c.C1, c.H, c.W), pooled=(c.B, c.C1, c.H // 2, c.W // 2))
    if c.C2:
        g['x2'] = (c.B, c.C2, c.H, c.W)
    if c.add:
        g.update(add=(c.B, c.Cout, OH + 3, OW + 2), add_off=(2, 1))
    if placed == 'slice':
        g.update(out=(c.B, c.Cout + 3, OH + 3, OW + 5), place=(1, 2), out_c0=2)
    elif placed == 'plane':
        g.update(out=(c.B, c.Cout, OH + 3, OW + 5), place=(1, 2))
    return g


def call_kwargs(g, tensor):
    """Keyword arguments of Conv.__call__ / Conv._describe_call (without x1) for the geometry `g`;
    tensor(name, shape) makes each operand."""
    kw = {k: tensor(k, g[k]) for k in ('x2', 'pre', 'pooled', 'add', 'out') if g[k] is not None}
    if g['add'] is not None:
        kw['add_off'] = g['add_off']
    for k in ('window', 'place', 'out_c0'):
        if g[k] is not None:
            kw[k] = g[k]
    return kw
