"""The per-pixel tail (csrc/tail.hip), the metrics accumulator (csrc/metrics.hip) and the two pool adjoints
(csrc/pool_unpool.hip) at their edges, against the float64 restatements of tests/tail_ref.py (pinned to the
oracle and to autograd by tests/test_tail_ref.py): both template instantiations of every column kernel
(C <= 16 / C > 16) and the class counts around the switch, maps of one pixel, of less than a wave, of exactly one
block and of one pixel more, scores that are all negative (a padded zero lane would win the max), the bf16 C8
mirror bit for bit, the finalize's strided sum and its stop threshold, forced ties and all-zero windows in the
adjoints, and element counts past the capped grids of the grid-stride kernels.

Placement: every tensor a kernel writes lies in the middle of a larger flat allocation with GUARD sentinel
elements on either side, which must be unchanged afterwards, as must every read-only input.

Tolerances (absolute, against float64).  float64 kernels: 1e-14 for maps, 1e-12 for norms; fp32 norms 1e-6 (the
suite's).  fp32 softmax-valued maps and the updated y: 2e-6; fp32 sqerr_softmax_bwd (values bounded by 4): 5e-6.
The two fp32 map bounds are four times what a numpy float32 emulation of tail_math.h's order of operations (max,
exp(v - max), sum in channel order, one reciprocal) differs from float64 on the two score families below
(4 x 64 x 64 pixels, C in {1, 2, 11, 16, 17, 21, 32}: 5.7e-7 for the softmax, 1.2e-6 for the gradient), the
factor covering the ulp or two by which the device's expf and division may differ from numpy's; tail.hip is built
without relaxed-math flags.  A wrong channel, a padded lane in the max or the sum, or a wrong crop offset is an
error of 1e-3 and more.  Each test prints the largest error it saw; on an MI355X the largest over the tables were
(fp32) crop_softmax 4.9e-7, refine_update y 2.7e-7 / norm 1.4e-7, grad_update y 4.8e-7 / norm 3.9e-7,
sqerr_softmax_bwd 1.1e-6; (float64) maps 4.3e-16, norms 1.8e-15.

Each of these changes to a kernel makes tests of this file fail (tried, one at a time): no c < C guard in
softmax_column's max loop (the 'far_negative' cases of all four column kernels, 16 and 32 classes -- no padded
lane -- excepted); `tvoid >= bt` in confusion_kernel
(every confusion case with more than one pixel); `norm <= eps` in refine_finalize_kernel (the finalize test at every
nblk); only the first 64 partials added there (nblk 65 and 200); `pv >= 0` in pool_relu_bwd_kernel and a dropped
fourth term in depool_bwd_kernel (every case of the kernel, the 2 x 2 'tie' map of pool_relu_bwd excepted)."""
import functools

import numpy as np
import pytest
import torch

import tail_ref as R
from _parity_helpers import GUARD, SENTINEL, Placed, same_bits
from oracle import nn as onn

pytestmark = pytest.mark.gpu

DTYPES = {'f32': torch.float32, 'f64': torch.float64}
MAP_TOL = {'f32': 2e-6, 'f64': 1e-14}
BWD_TOL = {'f32': 5e-6, 'f64': 1e-14}
NORM_TOL = {'f32': 1e-6, 'f64': 1e-12}


@pytest.fixture(scope='module')
def ops(built_lib):
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from iterative_inference_segm_amd import ops as _ops
    return _ops


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.array(a)).to(dtype).cuda()          # (a copy: the shared references are read-only)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ---- shared tables of the column kernels (groups A and B) ------------------------------------------------------
CLASSES = (1, 2, 11, 15, 16, 17, 21, 31, 32)
GEOMETRIES = (          # SH, SW, H, W, off
    (1, 1, 1, 1, None),                 # one pixel
    (9, 9, 7, 9, None),                 # less than a wave
    (16, 16, 16, 16, None),             # exactly one block
    (20, 300, 1, 257, (19, 43)),        # one pixel over a block; the window ends at the last row and column
    (300, 3, 300, 1, (0, 2)),           # a tall one-column map
    (30, 29, 24, 20, None),             # the default centre crop, odd margins
    (70, 70, 65, 67, (0, 0)),           # 18 blocks
)
FAMILIES = ('randn', 'negative')
# class i meets the geometries j = i (mod 3): every class at two or three geometries, every geometry at three
# class counts (at least one on either side of the C <= 16 / C > 16 switch), both score families each; the
# batch (1, or 3 with image 1 stopped beforehand) and the step (0.1 / 0.5) alternate along both axes
COLUMN_CASES = [(C, GEOMETRIES[j], 1 if (i + j) % 2 == 0 else 3, fam, 0.1 if (i + j // 3) % 2 == 0 else 0.5)
                for i, C in enumerate(CLASSES) for j in range(len(GEOMETRIES)) if (j - i) % 3 == 0
                for fam in FAMILIES]
assert len(COLUMN_CASES) == 42
for _C in CLASSES:
    assert len({c[1] for c in COLUMN_CASES if c[0] == _C}) >= 2 and {c[2] for c in COLUMN_CASES if c[0] == _C} == {1, 3}
for _g in GEOMETRIES:
    _cs = {c[0] for c in COLUMN_CASES if c[1] == _g}
    assert len(_cs) >= 2 and min(_cs) <= 16 < max(_cs) and {c[2] for c in COLUMN_CASES if c[1] == _g} == {1, 3}
# A third family, once per class count, at the last of its geometries above (always more than one block): scores so
# far below zero that exp(v - 0) is 0 in either precision.  The 'negative' scores let a padded zero win the max, but
# a softmax does not depend on what is subtracted as long as nothing underflows, and exp(-74) does not: a kernel
# without the c < C guard in its max loop passes them (tried).  On these it divides 0 by 0.
COLUMN_CASES += [(C, [g for g in GEOMETRIES if any(c[:2] == (C, g) for c in COLUMN_CASES)][-1], 3, 'far_negative', 0.5)
                 for C in CLASSES]
assert len(COLUMN_CASES) == 51


def _case_id(c):
    C, (SH, SW, H, W, off), B, fam, step = c
    return 'C%d-%dx%d_in_%dx%d-B%d-%s-step%g' % (C, H, W, SH, SW, B, fam, step)


def _scores(rng, shape, fam):
    """All families are exact in float32.  'negative': -64 + k / 8, k an integer in [-80, 80] -- every score is
    negative, so a zero from a padded lane would win the max, and every v - max is exact in fp32.  'far_negative':
    the same around -800."""
    if fam == 'randn':
        return (5 * rng.standard_normal(shape)).astype(np.float32)
    base = {'negative': -64, 'far_negative': -800}[fam]   # (exp(-790) is 0 in float64 too)
    return (base + rng.integers(-80, 81, size=shape) / 8.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _column_data(case):
    """The inputs of a case (float32-exact, so the same values serve both dtypes) and its float64 references;
    computed once, shared by the tests of the four kernels, never modified."""
    C, (SH, SW, H, W, off), B, fam, step = case
    rng = np.random.default_rng(1000 + COLUMN_CASES.index(case))
    d = dict(score=_scores(rng, (B, C, SH, SW), fam),
             y=rng.random((B, C, H, W)).astype(np.float32),
             gthrough=rng.uniform(-1, 1, (B, C, H, W)).astype(np.float32),
             active=np.array([1, 0, 1][:B], np.int32))
    d['r'] = R.crop_softmax(d['score'], H, W, off)
    d['de'] = R.crop_softmax(d['score'], H, W, off, minuend=d['y'])
    d['bwd'] = R.sqerr_softmax_bwd(d['score'], d['y'], off)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _step_ref(case, dt, kind):
    """(new y, norms) of a case with the step the kernel of that dtype multiplies with: the wrappers hand the
    step over as a C float / double, and float32(0.1) is not 0.1."""
    C, (SH, SW, H, W, off), B, fam, step = case
    d = _column_data(case)
    step = float(np.float32(step)) if dt == 'f32' else step
    if kind == 'refine':
        return R.refine_step(d['score'], d['y'], d['active'], step, off)
    return R.grad_step(d['score'], d['gthrough'], d['y'], d['active'], step, off)


column_cases = pytest.mark.parametrize('case', COLUMN_CASES, ids=_case_id)
both_dtypes = pytest.mark.parametrize('dt', ['f32', 'f64'])


# ---- A. column kernels ----------------------------------------------------------------------------------------
@both_dtypes
@column_cases
def test_crop_softmax(ops, case, dt):
    C, (SH, SW, H, W, off), B, fam, step = case
    d, T, p = _column_data(case), DTYPES[dt], Placed()
    score, y = p.inp(d['score'], T), p.inp(d['y'], T)
    out = ops.crop_softmax(score, H, W, off=off, out=p.out((B, C, H, W), T))
    de = ops.crop_softmax(score, H, W, off=off, out=p.out((B, C, H, W), T), minuend=y)
    got, got_de = host(out), host(de)
    p.check()
    err = max(np.abs(got - d['r']).max(), np.abs(got_de - d['de']).max())
    sum_err = np.abs(got.astype(np.float64).sum(1) - 1).max()
    print('crop_softmax %s %s: max |err| %.3e, |channel sum - 1| %.3e (bound %.0e)'
          % (_case_id(case), dt, err, sum_err, MAP_TOL[dt]))
    assert err <= MAP_TOL[dt] and sum_err <= MAP_TOL[dt]


def _finalized(d, norms, eps, HW):
    """What refine_finalize leaves from the reference norms of a step on a fresh state."""
    B = len(d['active'])
    return R.finalize(norms * HW, d['active'], np.zeros(B), np.zeros(B), HW, eps)


def _check_step(p, st, y, d, ref, dt, what, eps):
    """The outputs of an update kernel + finalize against (new y, norms) of the restatement."""
    y_ref, norms = ref
    got = host(y)
    active, iters, last = host(st.active), host(st.iters), host(st.last_norm)
    p.check()
    B, HW = got.shape[0], got.shape[2] * got.shape[3]
    err = np.abs(got - y_ref).max()
    on = d['active'] != 0
    nerr = np.abs(last - norms)[on].max()
    print('%s %s: max |err| y %.3e (bound %.0e), norm %.3e (bound %.0e)'
          % (what, dt, err, MAP_TOL[dt], nerr, NORM_TOL[dt]))
    assert err <= MAP_TOL[dt]
    for b in range(B):
        if not on[b]:                    # a stopped image: bit-identical, and its state untouched
            assert np.array_equal(got[b], d['y'][b].astype(got.dtype))
    a_ref, it_ref, last_ref = _finalized(d, norms, eps, HW)
    assert list(iters) == list(it_ref) and list(active) == list(a_ref)
    assert nerr <= NORM_TOL[dt] and np.array_equal(last[~on], last_ref[~on])


# the norms of the table's cases are far above this (y is uniform noise), so nothing stops: the decision at the
# threshold is group C's, the image that stops in the step it is updated in has its own test below
EPS = 1e-3


@both_dtypes
@column_cases
def test_refine_update_and_finalize(ops, case, dt):
    C, (SH, SW, H, W, off), B, fam, step = case
    d, T, p = _column_data(case), DTYPES[dt], Placed()
    score = p.inp(d['score'], T)
    y = p.out((B, C, H, W), T, dev(d['y'], T))
    st = p.state(ops, B, H, W, active=d['active'])
    ops.refine_update(score, y, st, step, off=off)
    ops.refine_finalize(st, EPS)
    _check_step(p, st, y, d, _step_ref(case, dt, 'refine'), dt, 'refine_update ' + _case_id(case), EPS)


@both_dtypes
@column_cases
def test_grad_update_and_finalize(ops, case, dt):
    C, (SH, SW, H, W, off), B, fam, step = case
    d, T, p = _column_data(case), DTYPES[dt], Placed()
    score, gthrough = p.inp(d['score'], T), p.inp(d['gthrough'], T)
    y = p.out((B, C, H, W), T, dev(d['y'], T))
    st = p.state(ops, B, H, W, active=d['active'])
    ops.grad_update(score, gthrough, y, st, step, off=off)
    ops.refine_finalize(st, EPS)
    _check_step(p, st, y, d, _step_ref(case, dt, 'grad'), dt, 'grad_update ' + _case_id(case), EPS)


@both_dtypes
@column_cases
def test_sqerr_softmax_bwd(ops, case, dt):
    C, (SH, SW, H, W, off), B, fam, step = case
    d, T, p = _column_data(case), DTYPES[dt], Placed()
    score, y = p.inp(d['score'], T), p.inp(d['y'], T)
    with p.allocations():
        g = ops.sqerr_softmax_bwd(score, y, off=off)
    got = host(g)
    p.check()
    assert len(p.flats) == 1 and got.shape == d['bwd'].shape
    err = np.abs(got - d['bwd']).max()
    print('sqerr_softmax_bwd %s %s: max |err| %.3e (bound %.0e)' % (_case_id(case), dt, err, BWD_TOL[dt]))
    assert err <= BWD_TOL[dt]


@both_dtypes
@pytest.mark.parametrize('C', [11, 21])
@pytest.mark.parametrize('kernel', ['refine_update', 'grad_update'])
def test_an_image_that_converges_is_still_updated_in_that_step(ops, kernel, C, dt):
    """Image 2 starts at y = float32(r) (grad_update: and gthrough = 0), so its norm falls below eps in this
    very step: it is updated, counted and then stopped (the stop test comes AFTER the update)."""
    T, p = DTYPES[dt], Placed()
    rng = np.random.default_rng(50 + C)
    B, H, W, off, step, eps = 3, 19, 23, None, 0.5, 1e-3
    d = dict(score=_scores(rng, (B, C, H + 4, W + 3), 'randn'), y=rng.random((B, C, H, W)).astype(np.float32),
             gthrough=rng.uniform(-1, 1, (B, C, H, W)).astype(np.float32), active=np.array([1, 0, 1], np.int32))
    d['y'][2] = R.crop_softmax(d['score'], H, W)[2].astype(np.float32)
    d['gthrough'][2] = 0
    score, gthrough = p.inp(d['score'], T), p.inp(d['gthrough'], T)
    y = p.out((B, C, H, W), T, dev(d['y'], T))
    st = p.state(ops, B, H, W, active=d['active'])
    if kernel == 'refine_update':
        ops.refine_update(score, y, st, step)
        ref = R.refine_step(d['score'], d['y'], d['active'], step)
    else:
        ops.grad_update(score, gthrough, y, st, step)
        ref = R.grad_step(d['score'], d['gthrough'], d['y'], d['active'], step)
    ops.refine_finalize(st, eps)
    assert 0 < ref[1][2] < 1e-6 < eps < ref[1][0]
    assert not np.array_equal(ref[0][2], d['y'][2])                      # (the reference does move it)
    _check_step(p, st, y, d, ref, dt, kernel + ' converging C%d' % C, eps)
    assert list(host(st.active)) == [1, 0, 0] and list(host(st.iters)) == [1, 0, 1]
    if dt == 'f64':
        assert not np.array_equal(host(y)[2], d['y'][2])


@both_dtypes
@pytest.mark.parametrize('C', [2, 16, 17])
@pytest.mark.parametrize('kernel', ['refine_update', 'grad_update'])
def test_the_clip_on_both_sides(ops, kernel, C, dt):
    """y in {0, 1} against a confident softmax of the opposite class.  grad_update leaves [0, 1] on both sides
    at step 0.5 (grad = gthrough -+ 2).  refine_update's y - step (y - r) is a convex combination of y and r for
    step <= 1 and cannot leave the interval, so its clip is driven with step 1.5."""
    T, p = DTYPES[dt], Placed()
    rng = np.random.default_rng(60 + C)
    B, H, W = 2, 9, 31
    step = 1.5 if kernel == 'refine_update' else 0.5
    win = rng.integers(0, C, size=(B, H, W))
    score = np.full((B, C, H, W), -20.0, np.float32)
    np.put_along_axis(score, win[:, None], 20.0, axis=1)
    score += rng.integers(-8, 9, size=score.shape).astype(np.float32) / 8
    y = np.ones((B, C, H, W), np.float32)
    np.put_along_axis(y, win[:, None], 0.0, axis=1)                       # 0 where r ~ 1, 1 where r ~ 0
    d = dict(score=score, y=y, gthrough=rng.uniform(-1, 1, y.shape).astype(np.float32), active=np.ones(B, np.int32))
    r = R.crop_softmax(score, H, W)
    if kernel == 'refine_update':
        free, ref = y - step * (y - r), R.refine_step(score, y, d['active'], step)
    else:
        free, ref = y - step * (d['gthrough'] - 2 * (r - y)), R.grad_step(score, d['gthrough'], y, d['active'], step)
    assert (free < -0.1).any() and (free > 1.1).any() and (ref[0] == 0).any() and (ref[0] == 1).any()
    sc, gt = p.inp(score, T), p.inp(d['gthrough'], T)
    yd = p.out((B, C, H, W), T, dev(y, T))
    st = p.state(ops, B, H, W)
    if kernel == 'refine_update':
        ops.refine_update(sc, yd, st, step)
    else:
        ops.grad_update(sc, gt, yd, st, step)
    ops.refine_finalize(st, EPS)
    _check_step(p, st, yd, d, ref, dt, kernel + ' clip C%d' % C, EPS)
    got = host(yd)
    assert got.min() == 0 and got.max() == 1


def _tail_calls(ops, p, score, y, st, off, H, W):
    gthrough = p.inp(np.zeros(tuple(y.shape), np.float32))
    return {
        'crop_softmax': lambda: ops.crop_softmax(score, H, W, off=off, out=y),
        'refine_update': lambda: ops.refine_update(score, y, st, 0.1, off=off),
        'sqerr_softmax_bwd': lambda: ops.sqerr_softmax_bwd(score, y, off=off),
        'grad_update': lambda: ops.grad_update(score, gthrough, y, st, 0.1, off=off),
    }


def test_more_than_32_classes_and_windows_past_the_map_are_refused(ops):
    """C = 33: status -5 ("no kernel variant") from each of the five wrappers; a window that ends past the score
    map: "shape".  Nothing is launched: every placed tensor keeps its sentinels."""
    p = Placed()
    B, C, H, W = 1, 33, 4, 5
    score = p.inp(np.zeros((B, C, H, W), np.float32))
    y, st = p.out((B, C, H, W), torch.float32), p.state(ops, B, H, W)
    for name, call in _tail_calls(ops, p, score, y, st, (0, 0), H, W).items():
        with pytest.raises(RuntimeError, match=r'no kernel variant.*iiseg_status -5'), p.allocations():
            call()
    cm, sums = p.out((C * (C + 1),), torch.int64), p.out((2,), torch.float64)
    with pytest.raises(RuntimeError, match=r'no kernel variant.*iiseg_status -5'):
        ops.confusion_accumulate(score, p.inp(np.zeros((B, C + 1, H, W), np.float32)), cm, sums)
    # an 11-class score map one row and one column larger than the window
    score11, y11 = p.inp(np.zeros((B, 11, H + 1, W + 1), np.float32)), p.out((B, 11, H, W), torch.float32)
    for off in ((2, 0), (0, 2), (-1, 0), (0, -1)):
        for name, call in _tail_calls(ops, p, score11, y11, st, off, H, W).items():
            with pytest.raises(RuntimeError, match='shape'), p.allocations():
                call()
    p.check()
    assert len(p.blank) >= 6 and p.nothing_written()                     # y, y11, cm, sums, the partials, the results
    assert list(host(st.iters)) == [0] and list(host(st.active)) == [1]


# ---- B. the bf16 C8 mirror of the updated map (fp32 only) ------------------------------------------------------
# (classes, chunks of y8): exactly ceil(C / 8) chunks, and for 11 classes also the 4 the entry point allows at
# most; each at one geometry of the table with a ragged last block, and the class counts on either side of the
# C <= 16 switch at the second one as well
MIRROR_CASES = [(C, (C + 7) // 8, GEOMETRIES[3 if k % 2 == 0 else 5], FAMILIES[k % 2])
                for k, C in enumerate((1, 8, 9, 11, 16, 17, 21, 32))] + \
               [(11, 4, GEOMETRIES[3], 'negative'), (16, 2, GEOMETRIES[3], 'negative'), (17, 3, GEOMETRIES[5], 'randn')]


@pytest.mark.parametrize('C,chunks,geom,fam', MIRROR_CASES,
                         ids=['C%d-%dchunks-%dx%d-%s' % (c[0], c[1], c[2][2], c[2][3], c[3]) for c in MIRROR_CASES])
def test_refine_update_c8_mirror_is_the_bf16_of_the_updated_map(ops, C, chunks, geom, fam):
    """The whole y8 tensor -- zero lanes >= C and zero chunks past ceil(C / 8) included, over a non-zero
    prefill -- is bit for bit the bf16 (round to nearest even) of the fp32 y the same call left; for the stopped
    image that is its unchanged y (the next DAE forward reads the mirror of every image of the batch).  Every other
    output is bit-identical to the call without y8."""
    SH, SW, H, W, off = geom
    B, step = 3, 0.5
    rng = np.random.default_rng(200 + 8 * C + chunks)
    score0 = _scores(rng, (B, C, SH, SW), fam)
    y0 = rng.random((B, C, H, W)).astype(np.float32)
    runs = []
    for mirrored in (False, True):
        p = Placed()
        score = p.inp(score0)
        y = p.out((B, C, H, W), torch.float32, y0)
        st = p.state(ops, B, H, W, active=[1, 0, 1])
        y8 = None
        if mirrored:
            y8 = p.out((B, chunks, H, W, 8), torch.bfloat16,
                       torch.full((B, chunks, H, W, 8), 2.5, dtype=torch.bfloat16))
        ops.refine_update(score, y, st, step, off=off, y8=y8)
        partial = host(st.partial).copy()
        ops.refine_finalize(st, EPS)
        runs.append((host(y), partial, host(st.last_norm), host(st.active), host(st.iters)))
        p.check()
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    got_y = runs[1][0]
    assert np.array_equal(got_y[1], y0[1]) and not np.array_equal(got_y[0], y0[0])
    assert np.abs(got_y - R.refine_step(score0, y0, [1, 0, 1], step, off)[0]).max() <= MAP_TOL['f32']
    want = R.to_c8_bf16(got_y, chunks)
    got8 = y8.cpu()
    assert got8.shape == want.shape
    assert torch.equal(got8.view(torch.int16), want.view(torch.int16))


# ---- C. refine_finalize on synthetic partials ------------------------------------------------------------------
@pytest.mark.parametrize('nblk', [1, 63, 64, 65, 200])
def test_refine_finalize_sums_every_partial_and_stops_below_eps_only(ops, nblk):
    """One wave per image: lane l adds partials l, l + 64, ...  Partials are small integers (every summation order
    gives the same double).  HW = 16 and eps = 0.5: image 0 sums to 8, its norm EQUALS eps and it stays active;
    image 1 was stopped before and keeps its state; image 2 sums to the double below 8 and stops.  A second
    round on random integers pins the sum itself."""
    B, H, W, eps = 3, 4, 4, 0.5
    rng = np.random.default_rng(nblk)
    part = np.zeros((B, nblk))
    spread = sorted({0, nblk // 2, min(64, nblk - 1), nblk - 1})
    part[0, spread] = 1
    part[0, nblk - 1] += 8 - part[0].sum()
    part[1] = rng.integers(0, 6, size=nblk)
    part[2, nblk - 1] = np.nextafter(8.0, 0.0)                            # (one term: no order to depend on)
    assert part[0].sum() == 8.0
    rounds = ((part, ([1, 0, 1], [3, 5, 0], [7.25, 6.5, 9.0])),
              (rng.integers(0, 6, size=(B, nblk)).astype(np.float64), ([1, 1, 0], [0, 2, 4], [1.0, 2.0, 3.0])))
    for part, state0 in rounds:
        p = Placed()
        st = p.state(ops, B, H, W, *state0, npartial=nblk)
        st.partial.copy_(torch.from_numpy(part.reshape(-1)))
        kept = st.partial.clone()
        ops.refine_finalize(st, eps, nblk=nblk)
        active, iters, last = host(st.active), host(st.iters), host(st.last_norm)
        p.check()
        assert torch.equal(st.partial, kept)
        a_ref, it_ref, last_ref = R.finalize(part.sum(axis=1), *state0, H * W, eps)
        assert list(active) == list(a_ref) and list(iters) == list(it_ref)
        assert np.array_equal(last, last_ref)                            # sum / HW exactly
    # (the first round, spelled out)
    a_ref, it_ref, last_ref = R.finalize([8.0, 0.0, np.nextafter(8.0, 0.0)], [1, 0, 1], [3, 5, 0],
                                         [7.25, 6.5, 9.0], 16, eps)
    assert list(a_ref) == [1, 0, 0] and list(it_ref) == [4, 5, 1]
    assert list(last_ref) == [0.5, 6.5, np.nextafter(0.5, 0.0)]


# ---- D. ctx_tail shares tail_math.h and promises the same bits -------------------------------------------------
@pytest.mark.parametrize('H,W', [(5, 7), (16, 64), (17, 65)], ids=['5x7', '16x64-one-tile', '17x65'])
@pytest.mark.parametrize('C', [9, 11, 16])
def test_ctx_tail_is_bit_identical_to_the_separate_launches(ops, C, H, W):
    """conv6 + conv7 + softmax + update as one launch against conv7(conv6(x)) followed by refine_update, on copies
    of the same inputs: y bit for bit, iters and active after finalize; last_norm to rtol 1e-9 (the partials are
    summed per 16 x 64 tile instead of per 256 pixels; the bound of test_contextmod_fused_tail_is_bit_identical).
    Image 1 is stopped beforehand; image 2 starts at the softmax of its scores and stops in this step."""
    rng = np.random.default_rng(300 + C + H)
    B, step, eps = 3, 0.5, 1e-3
    conv6 = ops.Conv((rng.standard_normal((C, C, 3, 3)) / np.sqrt(C)).astype(np.float32),
                     rng.standard_normal(C).astype(np.float32), pad=0, relu=True, mma='f32')
    conv7 = ops.Conv(rng.standard_normal((C, C, 1, 1)).astype(np.float32), rng.standard_normal(C).astype(np.float32),
                     pad=0, relu=False, mma='f32')
    x0 = rng.standard_normal((B, C, H + 2, W + 2)).astype(np.float32)
    y0 = rng.random((B, C, H, W)).astype(np.float32)
    y0[2] = R.crop_softmax(host(conv7(conv6(dev(x0)))), H, W)[2].astype(np.float32)
    assert ops.ctx_tail_supported(conv6, conv7, dev(y0))
    runs = []
    for fused in (False, True):
        p = Placed()
        x = p.inp(x0)
        y = p.out((B, C, H, W), torch.float32, y0)
        st = p.state(ops, B, H, W, active=[1, 0, 1])
        if fused:
            nblk = ops.ctx_tail(conv6, conv7, x, y, st, step)
            assert nblk == -(-H // 16) * -(-W // 64)
        else:
            nblk = None
            ops.refine_update(conv7(conv6(x)), y, st, step, off=(0, 0))
        ops.refine_finalize(st, eps, nblk=nblk)
        runs.append((host(y), host(st.iters), host(st.active), host(st.last_norm)))
        p.check()
    (ya, ita, aca, lna), (yb, itb, acb, lnb) = runs
    assert np.array_equal(ya, yb), np.abs(ya - yb).max()
    assert np.array_equal(ya[1], y0[1]) and not np.array_equal(ya[0], y0[0])
    assert list(ita) == list(itb) == [1, 0, 1] and list(aca) == list(acb) == [1, 0, 0]
    assert np.allclose(lna, lnb, rtol=1e-9, atol=0)


# ---- E. the confusion matrix -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _confusion_data(C, HW):
    """Predictions (float32-exact probabilities) and one-hot targets with the void plane last, B = 3, with
    hand-placed pixels: the ties of the prediction, a void pixel, a class that only the last pixel of a map has,
    and one target that is not one-hot -- class 0 tied with void, the only way to tell `>` from `>=` in the
    void test.  The references with and without image 1 switched off."""
    B = 3
    rng = np.random.default_rng(400 + 64 * C + HW)
    y = rng.random((B, C, 1, HW)).astype(np.float32)
    y = (y / y.sum(1, keepdims=True)).astype(np.float32)
    # class C - 1 is kept for the last pixel of every map: a dropped ragged pixel changes a count
    labels = rng.choice(np.r_[np.arange(C - 1), C], size=(B, 1, HW))
    labels[:, 0, HW - 1] = C - 1
    tie = np.zeros(C, np.float32)
    tie[[1, C - 1] if C >= 3 else []] = 0.5                               # two non-zero classes tied: the lower wins
    if HW >= 4:
        y[0, :, 0, 0] = np.float32(1.0 / C)                               # every class tied: index 0
        if C >= 3:
            y[0, :, 0, 1] = tie
        labels[0, 0, 2] = C                                               # a void pixel
    else:                                                                 # one pixel per image: one image each
        y[0, :, 0, 0] = np.float32(1.0 / C)
        if C >= 3:
            y[1, :, 0, 0] = tie
        labels[1, 0, 0] = C
    t = np.zeros((B, C + 1, 1, HW), np.float32)
    np.put_along_axis(t, labels[:, None], 1.0, axis=1)
    if HW >= 4:
        t[0, :, 0, 3] = 0
        t[0, [0, C], 0, 3] = 0.5                                          # class 0 tied with void: the class wins
    refs = {None: R.confusion(y, t), (1, 0, 1): R.confusion(y, t, active=(1, 0, 1))}
    cm = refs[None][0]
    assert cm[0].sum() >= 1 and cm[:, C].sum() >= 1 and cm[:, C - 1].sum() >= 2
    for a in (y, t):
        a.setflags(write=False)
    return y, t, refs


@both_dtypes
@pytest.mark.parametrize('HW', [1, 255, 2048, 2049, 5000])
@pytest.mark.parametrize('C', [1, 11, 15, 16, 21, 31])
def test_confusion_counts_are_exact(ops, C, HW, dt):
    """One block covers 8 x 256 pixels; C + 1 <= 16 runs the 16-plane instantiation, 15 classes its last.
    Counts equal the restatement exactly, accumulate (a second pass doubles them), and skip a switched-off image;
    the two sums to 1e-6 relative (fp32 squares and channel mean, double accumulation) / 1e-12 (float64)."""
    T = DTYPES[dt]
    y0, t0, refs = _confusion_data(C, HW)
    for active, (cm_ref, sums_ref) in refs.items():
        p = Placed()
        y, t = p.inp(y0, T), p.inp(t0, T)
        act = None if active is None else p.inp(torch.tensor(active, dtype=torch.int32))
        cm = p.out((C * (C + 1),), torch.int64, np.zeros(C * (C + 1), np.int64))
        sums = p.out((2,), torch.float64, np.zeros(2))
        for n in (1, 2):
            ops.confusion_accumulate(y, t, cm, sums, active=act)
            got_cm, got_sums = host(cm).reshape(C, C + 1), host(sums)
            assert np.array_equal(got_cm, n * cm_ref), (active, n)
            err = np.abs(got_sums - n * sums_ref)
            assert (err <= (1e-6 if dt == 'f32' else 1e-12) * n * sums_ref).all(), (active, n, err, sums_ref)
        p.check()
    assert refs[None][0].sum() == 3 * HW and refs[(1, 0, 1)][0].sum() == 2 * HW


@both_dtypes
def test_confusion_refuses_32_classes(ops, dt):
    T, p = DTYPES[dt], Placed()
    C = 32
    cm, sums = p.out((C * (C + 1),), torch.int64), p.out((2,), torch.float64)
    with pytest.raises(RuntimeError, match=r'no kernel variant.*iiseg_status -5'):
        ops.confusion_accumulate(p.inp(np.zeros((1, C, 2, 3)), T), p.inp(np.zeros((1, C + 1, 2, 3)), T), cm, sums)
    p.check()
    assert p.nothing_written()


# ---- F. the pool adjoints --------------------------------------------------------------------------------------
def _win(a):
    B, C, H, W = a.shape
    return a[:, :, :H // 2 * 2, :W // 2 * 2].reshape(B, C, H // 2, 2, W // 2, 2)


@functools.lru_cache(maxsize=None)
def _pool_data(shape, variant):
    """Integer data: gradients in [-3, 3], pre = relu of integers in [-2, 3]: every sum of four terms is exact.
    The 2 x 2 map has one window; it comes as the tied window and as the all-zero window."""
    B, C, H, W = shape
    rng = np.random.default_rng(sum(shape))
    pre = np.maximum(rng.integers(-2, 4, size=shape), 0).astype(np.float64)
    if variant == 'tie':
        pre[...] = [[3, 1], [0, 3]]
    elif variant == 'zero':
        pre[...] = 0
    pooled = onn.maxpool2(pre)
    d = dict(pre=pre, pooled=pooled, gout=rng.integers(-3, 4, size=shape).astype(np.float64),
             gpool=rng.integers(-3, 4, size=pooled.shape).astype(np.float64))
    if variant != 'random':
        d['gout'][...] = [[1, 2], [3, -3]]
        d['gpool'][...] = -2
    for v in d.values():
        v.setflags(write=False)
    win = _win(pre)
    tied = ((win == pooled[:, :, :, None, :, None]).sum(axis=(3, 5)) >= 2) & (pooled > 0)
    zero = ~win.any(axis=(3, 5))
    if variant != 'zero':
        assert tied.any(), 'no window with tied positive maxima'
    if variant != 'tie':
        assert zero.any(), 'no all-zero window'
    return d


POOL_CASES = [((1, 1, 2, 2), 'tie'), ((1, 1, 2, 2), 'zero'), ((2, 3, 9, 7), 'random'), ((1, 5, 211, 13), 'random'),
              ((3, 2, 16, 64), 'random')]
pool_cases = pytest.mark.parametrize('shape,variant', POOL_CASES,
                                     ids=['%dx%dx%dx%d-%s' % (c[0] + (c[1],)) for c in POOL_CASES])


def _pool_relu_bwd(ops, d, T):
    p = Placed()
    gpool, pre, pooled = p.inp(d['gpool'], T), p.inp(d['pre'], T), p.inp(d['pooled'], T)
    with p.allocations():
        gz = ops.pool_relu_bwd(gpool, pre, pooled)
    got = host(gz)
    p.check()
    assert len(p.flats) == 1
    ref = R.pool_relu_bwd(d['gpool'], d['pre'], d['pooled'])
    assert got.shape == ref.shape and np.array_equal(got, ref)
    H, W = ref.shape[2:]
    assert not got[:, :, H // 2 * 2:].any() and not got[:, :, :, W // 2 * 2:].any()     # an odd last row / column
    return ref


def _depool_bwd(ops, d, T):
    p = Placed()
    gout, pre, pooled = p.inp(d['gout'], T), p.inp(d['pre'], T), p.inp(d['pooled'], T)
    with p.allocations():
        gup = ops.depool_bwd(gout, pre, pooled)
    got = host(gup)
    p.check()
    assert len(p.flats) == 1
    ref = R.depool_bwd(d['gout'], d['pre'], d['pooled'])
    assert got.shape == ref.shape and np.array_equal(got, ref)
    return ref


@both_dtypes
@pool_cases
def test_pool_relu_bwd_ties_zero_windows_and_odd_edges(ops, shape, variant, dt):
    d = _pool_data(shape, variant)
    ref = _pool_relu_bwd(ops, d, DTYPES[dt])
    if variant == 'tie':
        assert np.array_equal(ref[0, 0], [[-2, 0], [0, -2]])
    if variant == 'zero':
        assert not ref.any()


@both_dtypes
@pool_cases
def test_depool_bwd_ties_zero_windows_and_odd_edges(ops, shape, variant, dt):
    d = _pool_data(shape, variant)
    ref = _depool_bwd(ops, d, DTYPES[dt])
    if variant == 'tie':
        assert ref[0, 0, 0, 0] == 1 + -3
    if variant == 'zero':
        assert ref[0, 0, 0, 0] == 1 + 2 + 3 + -3                        # all four tied at 0: all four counted


@both_dtypes
def test_pool_relu_bwd_past_one_pass_of_the_capped_grid(ops, dt):
    """9 planes of 484 x 484 = 2 108 304 elements, more than the 8192 x 256 one pass of the grid covers."""
    shape = (1, 9, 484, 484)
    assert np.prod(shape) > 8192 * 256
    _pool_relu_bwd(ops, _pool_data(shape, 'random'), DTYPES[dt])


@both_dtypes
def test_depool_bwd_past_one_pass_of_the_capped_grid(ops, dt):
    """The count is over pooled elements here: 9 planes of 968 x 968 pool to 9 x 484 x 484."""
    shape = (1, 9, 968, 968)
    assert np.prod(shape) // 4 > 8192 * 256
    _depool_bwd(ops, _pool_data(shape, 'random'), DTYPES[dt])


# ---- G. element-wise helpers -----------------------------------------------------------------------------------
NONFINITE_STRIDE = 4096 * 256           # elements one pass of count_nonfinite's capped grid covers
EW_STRIDE = 16384 * 256                 # ... of add_noise's and dropout_apply's


@both_dtypes
@pytest.mark.parametrize('n', [1, 255, 257, NONFINITE_STRIDE + 513])
def test_count_nonfinite_counts_every_nan_and_inf_once(ops, n, dt):
    """NaN, -NaN, +Inf and -Inf at element 0, at the last element and (the large case) at the first element of
    the second pass of the grid; the largest finite values and a denormal are not counted; the counter
    accumulates over calls."""
    T, p = DTYPES[dt], Placed()
    npt = np.float32 if dt == 'f32' else np.float64
    fi = np.finfo(npt)
    rng = np.random.default_rng(n)
    base = rng.standard_normal(n).astype(npt)
    spots = sorted({0, n - 1} | ({NONFINITE_STRIDE} if n > NONFINITE_STRIDE else set()))
    if n >= 255:
        base[[1, 2, n - 2, 64]] = [fi.max, -fi.max, fi.smallest_subnormal, -fi.smallest_subnormal]
    specials = [npt(np.nan), npt(np.copysign(np.nan, -1)), npt(np.inf), npt(-np.inf)]
    assert np.signbit(specials[1]) and np.isnan(specials[1])
    counter = p.out((1,), torch.int32, np.zeros(1, np.int32))
    want = 0
    for call in range(4):                                                # every special visits every spot
        x = base.copy()
        for k, s in enumerate(spots):
            x[s] = specials[(call + k) % 4]
        ops.count_nonfinite(p.inp(torch.from_numpy(x)), counter)
        want += len(spots)
        assert int(host(counter)[0]) == want
    if n == 1:                                                           # (no room next to the special above)
        for v in (fi.max, -fi.max, fi.smallest_subnormal, 0.0):
            ops.count_nonfinite(p.inp(torch.from_numpy(np.array([v], npt))), counter)
    else:
        ops.count_nonfinite(p.inp(torch.from_numpy(base)), counter)
    assert int(host(counter)[0]) == want
    p.check()


@both_dtypes
@pytest.mark.parametrize('n', [1, 257, EW_STRIDE + 257])
def test_add_noise(ops, n, dt):
    """Small integers and sigma = 0.5: exact with or without FMA contraction.  Random data: fp32 within
    1e-6 (1 + |ref|), the element-wise rule of test_gpu_ops.py tightened; float64 within 1e-15 (1 + |ref|): one
    rounding of sigma * eps (|sigma eps| < 2.2) and one of the sum, 1.1e-16 relative each."""
    T = DTYPES[dt]
    rng = np.random.default_rng(n)
    for exact in (True, False):
        p = Placed()
        if exact:
            x0, e0 = (rng.integers(-4, 5, size=n).astype(np.float64) for _ in range(2))
            sigma = 0.5
        else:
            x0, e0 = (np.clip(rng.standard_normal(n), -6, 6).astype(np.float32).astype(np.float64) for _ in range(2))
            sigma = float(np.float32(0.37))
        x, e = p.inp(x0, T), p.inp(e0, T)
        with p.allocations():
            out = ops.add_noise(x, e, sigma)
        got = host(out)
        p.check()
        ref = x0 + sigma * e0
        assert len(p.flats) == 1 and got.shape == ref.shape
        if exact:
            assert np.array_equal(got, ref)
        else:
            assert (np.abs(got - ref) <= (1e-6 if dt == 'f32' else 1e-15) * (1 + np.abs(ref))).all()


@both_dtypes
@pytest.mark.parametrize('n', [1, 257, EW_STRIDE + 257])
def test_dropout_apply(ops, n, dt):
    """In place x * keep / (1 - p).  Integers with p in {0, 0.5} (scale 1 and 2): exact.  Random data, p = 0.3:
    the same element-wise rule (three roundings: 1 - p, the reciprocal, the product)."""
    T = DTYPES[dt]
    rng = np.random.default_rng(n + 1)
    keep0 = rng.integers(0, 2, size=n).astype(np.float64)
    for prob in (0.0, 0.5, 0.3):
        p = Placed()
        if prob != 0.3:
            x0 = rng.integers(-4, 5, size=n).astype(np.float64)
        else:
            x0 = rng.standard_normal(n).astype(np.float32).astype(np.float64)
        pk = float(np.float32(prob)) if dt == 'f32' else prob              # (the probability the kernel is handed)
        keep = p.inp(keep0, T)
        x = p.out((n,), T, dev(x0, T))
        assert ops.dropout_apply(x, keep, prob) is x
        got = host(x)
        p.check()
        ref = x0 * keep0 / (1.0 - pk)
        if prob != 0.3:
            assert np.array_equal(got, ref)
        else:
            assert (np.abs(got - ref) <= (1e-6 if dt == 'f32' else 1e-15) * (1 + np.abs(ref))).all()
