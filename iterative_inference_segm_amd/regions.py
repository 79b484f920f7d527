"""Rectangle arithmetic of the window optimisations: which part of a map a
changed input can reach (loop-invariant encoder maps, border stores) and which part of a map the final
crop reads (decoder dead-code elimination).  Integers in, tuples out: no torch, no launches.

A region is (y0, x0, h, w) in the coordinates of the map it lies in."""
from collections import namedtuple


def center(big, small):
    return (big - small) // 2  # lasagne autocrop 'center' (P6)


def clip(lo, hi, size):
    lo, hi = max(lo, 0), min(hi, size)
    return lo, max(hi - lo, 0)


def conv_region(dep, conv, fh, fw):
    """Outputs (y0, x0, h, w) of a stride-1 conv whose receptive field meets input region dep.
    `conv`: (pad, KH, KW, dil) or an object with these attributes; (fh, fw): the conv's output size."""
    pad, KH, KW, dil = conv if isinstance(conv, tuple) else (conv.pad, conv.KH, conv.KW, conv.dil)
    y0, h = clip(dep[0] + pad - dil * (KH - 1), dep[0] + dep[2] + pad, fh)
    x0, w = clip(dep[1] + pad - dil * (KW - 1), dep[1] + dep[3] + pad, fw)
    return (y0, x0, h, w)


def pool_region(dep, ph, pw):
    """Outputs of a 2x2 / 2 max-pool (odd last row / column dropped: (ph, pw) is the pooled size)
    that read input region dep."""
    y0, h = clip(dep[0] // 2, (dep[0] + dep[2] + 1) // 2, ph)
    x0, w = clip(dep[1] // 2, (dep[1] + dep[3] + 1) // 2, pw)
    return (y0, x0, h, w)


def union(a, b):
    """Bounding rectangle of two regions."""
    y0, x0 = min(a[0], b[0]), min(a[1], b[1])
    return (y0, x0, max(a[0] + a[2], b[0] + b[2]) - y0, max(a[1] + a[3], b[1] + b[3]) - x0)


def unpool_reads(geom_p, window, whole_pairs=False):
    """Rows / columns of the unpooled (pre-pool sized) map that decoder level p's 3x3 'same' conv reads
    for `window` of fused_up_p.  whole_pairs: clamped to the part DePool2D writes, 2 * (size // 2)."""
    ph, pw, _, _, cy, cx = geom_p
    if whole_pairs:
        ph, pw = 2 * (ph // 2), 2 * (pw // 2)
    y0, x0, nh, nw = window
    uy0, ux0 = max(cy + y0 - 1, 0), max(cx + x0 - 1, 0)
    return (uy0, ux0, min(cy + y0 + nh + 1, ph) - uy0, min(cx + x0 + nw + 1, pw) - ux0)


def unpool_reads_pooled(geom_p, window):
    """`unpool_reads` in the coordinates of the pooled map: the pooling windows a materialising
    DePool2D has to expand (the odd last row / column belongs to none and stays zero)."""
    uy0, ux0, uh, uw = unpool_reads(geom_p, window, whole_pairs=True)
    return (uy0 // 2, ux0 // 2, (uy0 + uh + 1) // 2 - uy0 // 2, (ux0 + uw + 1) // 2 - ux0 // 2)


def decoder_windows(pre_hw, pool_hw):
    """pre_hw[p], pool_hw[p] (p = 1..total; pool_hw[0]: the input): sizes of the encoder maps.
    Returns geom[p] = (ph, pw, oh, ow, cy, cx) -- up_conv_p runs 'same' on the pre-pool size (ph, pw),
    fused_up_p is its center crop (oh, ow) at (cy, cx) -- and win[p], the window of fused_up_p that
    reaches the final crop: level p needs fused_up_{p+1} on [floor((lo-1)/2), ceil((hi+1)/2))."""
    total = len(pre_hw)
    geom = {}
    for p in range(total, 0, -1):
        ph, pw = pre_hw[p]                           # up_conv 'same' keeps the pre-pool size
        oh, ow = min(ph, pool_hw[p - 1][0]), min(pw, pool_hw[p - 1][1])   # pre-concat pool (the input for p=1)
        geom[p] = (ph, pw, oh, ow, center(ph, oh), center(pw, ow))
    win = {1: (0, 0, geom[1][2], geom[1][3])}
    for p in range(1, total):
        win[p + 1] = pool_region(unpool_reads(geom[p], win[p]), geom[p + 1][2], geom[p + 1][3])
    return geom, win


def concat_feeds(concat_h, total, n_pool):
    """{level: index into h_list}: h is concatenated in front of the first conv of encoder level
    `level` (0-based; model_helpers.py:86-94 at the input, fcn_down.py:131-134 behind pool_level).
    Key `total`: an h behind the last pool, which no conv takes."""
    feeds, pos = {}, 0
    if concat_h[0] == 'input':
        feeds[0], pos = 0, 1
    for p in range(total):
        if p < n_pool and pos < len(concat_h) and concat_h[pos] == 'pool%d' % (p + 1):
            feeds[p + 1], pos = pos, pos + 1
    return feeds


# One encoder conv: level (0-based), i (1-based within the level), its output size, `ydep` (what y alone
# reaches: its origin parity anchors the Winograd tiles), `dep` (the window a primed call recomputes, else
# None), `pooled` (dep behind the level's pool; last conv of a primed level, else None), `h` (index of the
# h concatenated in front of it, or None), `h_window` (what a fresh h changes of its h-half, or None).
EncStep = namedtuple('EncStep', 'level i out_hw ydep dep pooled h h_window')
DaePlan = namedtuple('DaePlan', 'enc feeds geom win need')


def dae_plan(convs, conv_before_pool, total, n_pool, concat_h, y_hw, primed=False, h_dep=None, dce=True):
    """Windows of one StandardDAE.scores call.  convs: (pad, KH, KW, dil) per encoder conv in running
    order; primed: the session holds the maps of an earlier call with the same h (or, h_dep given, with
    an h that differs inside h_dep[k] only).  `need`: what each decoder level computes -- `win`, or the
    full maps with dce off (their Winograd tiles stay anchored at the parity of `win`, so that both modes
    agree bit for bit)."""
    feeds = concat_feeds(concat_h, total, n_pool)
    hw = tuple(y_hw)
    ydep = (0, 0) + hw
    dep = ydep if primed else None
    enc, pre_hw, pool_hw = [], {}, {0: hw}
    for p in range(total):
        for i in range(1, conv_before_pool + 1):
            conv = convs[len(enc)]
            pad, KH, KW, dil = conv
            hw = (hw[0] + 2 * pad - dil * (KH - 1), hw[1] + 2 * pad - dil * (KW - 1))
            h = feeds.get(p) if i == 1 else None
            hd = h_dep[h] if h is not None and h_dep is not None else None
            ydep = conv_region(ydep, conv, *hw)
            if primed:
                if hd is not None:       # a new batch in a reused session: h changed inside its tagged region
                    dep = union(dep, hd)
                dep = conv_region(dep, conv, *hw)
            last = i == conv_before_pool
            phw = (hw[0] // 2, hw[1] // 2)
            pooled = pool_region(dep, *phw) if primed and last else None
            enc.append(EncStep(p, i, hw, ydep, dep, pooled, h,
                               conv_region(hd, conv, *hw) if hd is not None else None))
        pre_hw[p + 1], pool_hw[p + 1], hw = hw, phw, phw
        ydep, dep = pool_region(ydep, *phw), pooled
    geom, win = decoder_windows(pre_hw, pool_hw)
    need = win if dce else {p: (0, 0, geom[p][2], geom[p][3]) for p in geom}
    return DaePlan(enc, feeds, geom, win, need)
