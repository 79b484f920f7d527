"""CPU: the rectangle arithmetic of the window optimisations (regions.py) and the StandardDAE plan
built on it, against brute force: a boolean "depends on" map pushed through each layer with numpy,
then its bounding box.  Equality, not containment: the formulas are exact on these geometries."""
import numpy as np
import pytest
import torch

from iterative_inference_segm_amd import regions as R

# (y H x W, first pad, levels, start region or None for the whole y)
GEOMETRIES = [((9, 7), 3, 3, None), ((12, 10), 100, 6, None), ((8, 8), 1, 2, None),
              ((13, 11), 5, 4, (2, 3, 4, 5)), ((6, 6), 0, 1, None)]
IDS = ['9x7-pad3', '12x10-pad100', '8x8-pad1', '13x11-pad5-window', '6x6-pad0']


def box(m):
    ys, xs = np.nonzero(m.any(1))[0], np.nonzero(m.any(0))[0]
    return (int(ys[0]), int(xs[0]), int(ys[-1] - ys[0] + 1), int(xs[-1] - xs[0] + 1))


def rect(shape, r):
    m = np.zeros(shape, bool)
    m[r[0]:r[0] + r[2], r[1]:r[1] + r[3]] = True
    return m


def conv3(m, pad):
    """3x3 stride-1 conv with zero padding: an output depends on the nine inputs under it."""
    q = np.pad(m, pad)
    H, W = q.shape[0] - 2, q.shape[1] - 2
    out = np.zeros((H, W), bool)
    for dy in range(3):
        for dx in range(3):
            out |= q[dy:dy + H, dx:dx + W]
    return out


def pool2(m):
    """2x2 / 2 max-pool, odd last row / column dropped."""
    H, W = m.shape[0] // 2, m.shape[1] // 2
    q = m[:2 * H, :2 * W]
    return q[0::2, 0::2] | q[0::2, 1::2] | q[1::2, 0::2] | q[1::2, 1::2]


def encoder(hw, pad, levels, start):
    """[(conv pad, map behind the conv, map behind its pool)] of one 3x3 conv + pool per level."""
    m = rect(hw, start or (0, 0) + hw)
    out = []
    for p in range(levels):
        c = conv3(m, pad if p == 0 else 1)
        m = pool2(c)
        out.append((pad if p == 0 else 1, c, m))
    return out


def decoder_brute(pre_hw, pool_hw, need_of):
    """Walks fused_up_1 -> fused_up_total.  need_of(p, win_p) is the window of fused_up_p that is
    computed; returns win and, per level, the unpooled rows / columns its conv reads."""
    total = len(pre_hw)
    win, reads = {1: None}, {}
    for p in range(1, total + 1):
        ph, pw = pre_hw[p]
        oh, ow = min(ph, pool_hw[p - 1][0]), min(pw, pool_hw[p - 1][1])
        cy, cx = (ph - oh) // 2, (pw - ow) // 2
        if p == 1:
            win[1] = (0, 0, oh, ow)
        u = np.zeros((ph, pw), bool)                 # the center crop, inside the 'same' conv's output
        u[cy:cy + oh, cx:cx + ow] = rect((oh, ow), need_of(p, win[p]))
        u = conv3(u, 1)                              # 'same': the inputs those outputs read
        reads[p] = u
        if p < total:
            qh, qw = min(pre_hw[p + 1][0], pool_hw[p][0]), min(pre_hw[p + 1][1], pool_hw[p][1])
            src = np.zeros((qh, qw), bool)           # unpooled (r, c) comes from fused_up_{p+1}[r // 2, c // 2]
            for r, c in zip(*np.nonzero(u)):
                if r // 2 < qh and c // 2 < qw:
                    src[r // 2, c // 2] = True
            win[p + 1] = box(src)
    return win, reads


def sizes(enc, hw):
    pre_hw = {p + 1: e[1].shape for p, e in enumerate(enc)}
    pool_hw = {p + 1: e[2].shape for p, e in enumerate(enc)}
    pool_hw[0] = hw
    return pre_hw, pool_hw


@pytest.mark.parametrize('hw,pad,levels,start', GEOMETRIES, ids=IDS)
def test_conv_and_pool_regions_equal_the_brute_force_boxes(hw, pad, levels, start):
    dep = start or (0, 0) + hw
    for cpad, c, m in encoder(hw, pad, levels, start):
        dep = R.conv_region(dep, (cpad, 3, 3, 1), *c.shape)
        assert dep == box(c)
        dep = R.pool_region(dep, *m.shape)
        assert dep == box(m)


@pytest.mark.parametrize('hw,pad,levels,start', GEOMETRIES, ids=IDS)
def test_decoder_windows_equal_the_brute_force_boxes(hw, pad, levels, start):
    pre_hw, pool_hw = sizes(encoder(hw, pad, levels, start), hw)
    geom, win = R.decoder_windows(pre_hw, pool_hw)
    bwin, reads = decoder_brute(pre_hw, pool_hw, lambda p, w: w)
    assert win == bwin
    for p in range(1, levels + 1):
        ph, pw = pre_hw[p]
        assert geom[p][:2] == (ph, pw) and geom[p][4:] == ((ph - geom[p][2]) // 2, (pw - geom[p][3]) // 2)
        assert R.unpool_reads(geom[p], win[p]) == box(reads[p])
        # the materialising C8 unpool expands whole pooling windows only
        pairs = reads[p][:2 * (ph // 2), :2 * (pw // 2)]
        assert R.unpool_reads(geom[p], win[p], whole_pairs=True) == box(pairs)
        assert R.unpool_reads_pooled(geom[p], win[p]) == box(pool2(reads[p]))


def test_decoder_windows_of_the_headline_shape_rules():
    pre_hw, pool_hw = sizes(encoder((12, 10), 100, 6, None), (12, 10))
    assert R.decoder_windows(pre_hw, pool_hw)[1] == {1: (0, 0, 12, 10), 2: (49, 49, 7, 6), 3: (24, 24, 5, 4),
                                                     4: (11, 11, 4, 4), 5: (5, 5, 3, 3), 6: (2, 2, 3, 3)}


def plan_of(hw, pad, levels, concat_h, n_pool, **kw):
    convs = [(pad if p == 0 else 1, 3, 3, 1) for p in range(levels)]
    return R.dae_plan(convs, 1, levels, n_pool, concat_h, hw, **kw)


@pytest.mark.parametrize('hw,pad,levels,start', GEOMETRIES, ids=IDS)
def test_plan_without_h_follows_the_brute_force_maps(hw, pad, levels, start):
    """Whole-y start only (a plan always starts there): dep == ydep == the boxes, per level."""
    enc = encoder(hw, pad, levels, None)
    plan = plan_of(hw, pad, levels, ['input'], 0, primed=True)
    cold = plan_of(hw, pad, levels, ['input'], 0)
    for step, cstep, (_, c, m) in zip(plan.enc, cold.enc, enc):
        assert step.out_hw == c.shape and step.dep == box(c) and step.pooled == box(m)
        assert step.ydep[:2] == box(c)[:2] == cstep.ydep[:2]
        assert cstep.dep is None and cstep.pooled is None
    assert (plan.geom, plan.win) == R.decoder_windows(*sizes(enc, hw))


def test_union_with_an_h_region_partly_outside_dep():
    """concat_h=['pool1'] at 3 levels, a reused session with a fresh h: behind pool1 the recomputed
    region is the box of (what y reaches) OR (where h changed)."""
    hw, pad, hd = (13, 11), 5, (0, 5, 2, 4)
    enc = encoder(hw, pad, 3, None)
    ymap = enc[0][2]
    hmap = rect(ymap.shape, hd)
    assert (hmap & ~ymap).any() and (hmap & ymap).any() and (ymap & ~hmap).any()
    assert R.union(box(ymap), hd) == box(ymap | hmap)
    plan = plan_of(hw, pad, 3, ['pool1'], 1, primed=True, h_dep=[hd])
    assert plan.feeds == {1: 0} and [s.h for s in plan.enc] == [None, 0, None]
    m = ymap | hmap
    for step, ystep in zip(plan.enc[1:], enc[1:]):
        c = conv3(m, 1)
        m = pool2(c)
        assert step.dep == box(c) and step.pooled == box(m)
        assert step.ydep[:2] == box(ystep[1])[:2]          # the anchors follow y alone
    assert plan.enc[1].h_window == box(conv3(hmap, 1))    # the h-half: where h changed, through its conv
    assert plan.enc[0].h_window is None and plan.enc[2].h_window is None
    # no fresh h: no union, no refresh
    same_h = plan_of(hw, pad, 3, ['pool1'], 1, primed=True)
    assert same_h.enc[1].dep == box(conv3(ymap, 1)) and same_h.enc[1].h_window is None


@pytest.mark.parametrize('hw,pad,levels,start', GEOMETRIES, ids=IDS)
def test_dce_off_computes_full_maps_at_the_anchors_of_the_windows(hw, pad, levels, start):
    on = plan_of(hw, pad, levels, ['input'], 0)
    off = plan_of(hw, pad, levels, ['input'], 0, dce=False)
    assert on.need == on.win and off.win == on.win and off.geom == on.geom
    assert off.need == {p: (0, 0, g[2], g[3]) for p, g in on.geom.items()}
    # full maps read what brute force says they read
    pre_hw, pool_hw = sizes(encoder(hw, pad, levels, None), hw)
    _, reads = decoder_brute(pre_hw, pool_hw, lambda p, w: off.need[p])
    for p in range(1, levels + 1):
        assert R.unpool_reads(off.geom[p], off.need[p]) == box(reads[p])


def test_concat_walk():
    from iterative_inference_segm_amd.dae import _n_pool
    walk = lambda concat_h, ap: R.concat_feeds(concat_h, _n_pool(concat_h, ap)[1], _n_pool(concat_h, ap)[0])
    assert walk(['input'], 2) == {0: 0}
    assert walk(['pool4'], 2) == {4: 0}
    assert walk(['input', 'pool2'], 1) == {0: 0, 2: 1}
    assert walk(['pool2'], 0) == {2: 0}              # == total: no conv takes it


@pytest.fixture(scope='module')
def dae(built_lib):
    from iterative_inference_segm_amd import synthetic as S
    from iterative_inference_segm_amd.dae import StandardDAE
    dp = S.make_dae_params(seed=4321)
    return StandardDAE(dp, 11, concat_h=['pool4'], padding=100, n_filters=64, additional_pool=2,
                       skip=True, unpool_type='trackind', device='cpu', dtype=torch.float32)


def test_h_at_the_last_pool_is_refused_by_scores(built_lib):
    from iterative_inference_segm_amd import synthetic as S
    from iterative_inference_segm_amd.dae import StandardDAE
    dp = S.make_dae_params(h_channels=(8,), concat_h=('pool1',), n_filters=4, additional_pool=0)
    net = StandardDAE(dp, 11, concat_h=['pool1'], n_filters=4, additional_pool=0, device='cpu',
                      dtype=torch.float32, mma='f32')
    with pytest.raises(NotImplementedError, match='last pool'):
        net.scores([torch.zeros(1, 8, 104, 104)], torch.zeros(1, 11, 10, 10))


def test_standard_dae_plan_is_the_pure_plan_of_its_integers(dae, monkeypatch):
    monkeypatch.setattr(dae, 'dce', True)
    shape, hd = (2, 11, 12, 10), [(3, 2, 6, 7)]
    convs = [(100 if p == 0 else 1, 3, 3, 1) for p in range(6)]
    for primed, h_dep in ((False, None), (True, None), (True, hd)):
        want = R.dae_plan(convs, 1, 6, 4, ['pool4'], (12, 10), primed, h_dep, True)
        assert dae._plan(shape, primed, h_dep) == want
        assert [s.h for s in want.enc] == [None, None, None, None, 0, None]
    assert dae._plan(shape).win == {1: (0, 0, 12, 10), 2: (49, 49, 7, 6), 3: (24, 24, 5, 4),
                                    4: (11, 11, 4, 4), 5: (5, 5, 3, 3), 6: (2, 2, 3, 3)}
    monkeypatch.setattr(dae, 'dce', False)
    assert dae._plan(shape) == R.dae_plan(convs, 1, 6, 4, ['pool4'], (12, 10), dce=False)
    assert dae._mask_levels(False) == frozenset(range(1, 7))
