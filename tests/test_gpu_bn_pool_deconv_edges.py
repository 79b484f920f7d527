"""The host networks' small kernels at their edges, against the float64 restatements of tests/bn_pool_ref.py
(pinned to the oracle and to torch CPU float64 by tests/test_bn_pool_ref.py): BatchNorm statistics, bn_relu and
bn_affine (csrc/bn.hip), the forward 2x2 max-pool / DePool2D kernels with their window and mask-byte forms
(csrc/pool_unpool.hip), the transposed convolution in its gather and output-phase forms (csrc/deconv.hip,
csrc/deconv_phase.hip), the NCHW <-> bf16 C8 slice converters (csrc/conv_c8_bf16.hip) and the C8 statistics and
BatchNorm fold (csrc/conv_c8_m16.hip).

Placement: every tensor a kernel writes lies between GUARD sentinel elements, which must be unchanged afterwards,
as must every read-only input; a refused request must leave nothing but sentinels.

NOT covered: the 64-bit index branch of maxpool2x2_window_kernel (2^31 and more window elements) and the
65536-block grid cap of the C8 converters (over 0.5 GB of input): neither fits a test of a few seconds.

Tolerances and where they come from (the largest errors seen on an MI355X follow):
  A. bn_stats, relative to the math.fsum two-pass reference of the same stored data.  float64: 1e-12, the suite's
     strict-parity tolerance, on every family, the large-offset ones included (bn_stats subtracts a per-channel
     pivot before it accumulates; the one-pass form on the raw values missed this bound by up to seven orders of
     magnitude on an MI355X).  fp32: one float32 ulp -- the kernel rounds a double whose own error is far below that.
  B. bn_relu / bn_affine, element-wise: 4 u (|x - m| |gamma inv_std| + |beta|), u = 2^-24 / 2^-53 -- one rounding
     each for the subtraction, the scale product, the multiply and the add.  Integer-valued parameters: the bits.
  C. pool / unpool / mask bytes: the bits (compare and select only).
  D. deconv: integer data the bits of the float64 restatement; random data the suite's conv_tol(ref, taps Cin)
     (tests/test_gpu_ops.py: 2e-6 sqrt(n) (1 + max |ref|)) and, float64, 1e-12 (1 + max |ref|); phase and gather
     forms the same bits wherever both run.
  E. C8 converters: the bits (bf16 round-to-nearest-even).  bn_stats_c8: two float32 ulps against the fsum
     reference of the STORED bf16 values, for channels with m^2 / (var + eps) <= 1e7.  That kernel keeps the
     one-pass form ss / n - m^2 in double: its relative error in var + eps is about 2^-53 m^2 / (var + eps), 1e-9
     at that limit, far below a float32 ulp -- and far above it past 1e14, which no bf16 activation of the
     FC-DenseNet stack reaches.  bn_fold: a the float32 product's bits, b within 2 u (|beta| + |m a|).
  F. refusals: a RuntimeError and nothing but sentinels.

Largest errors measured on an MI355X (each test prints its own), fp32 / float64:
  bn_stats mean 0.49 ulp / 1.8e-13; inv_std 0.50 ulp / 2.8e-15 (per family, float64: 0.5 +- 2 2.4e-15, 30 +- 0.05
  2.0e-15, 100 +- 0.01 2.8e-15, 1000 +- 1 1.7e-15, 1e4 +- 1 8.9e-16, constant 0; the kernel before the pivot:
  1.6e-12, 2.8e-10, 4.3e-8, 2.8e-7, 3.6e-5, 1.4e-13, and 0.77 ulp in fp32)
  bn_relu 5.2e-7 / 8.9e-16 and bn_affine 2.1e-6 / 8.9e-16, at most 0.47 / 0.50 of the element's bound
  pool, unpool, mask bytes, C8 converters: 0 (bits)
  deconv, random data: phase 8.8e-6 / 1.8e-14, gather 6.9e-6 / 1.4e-14 (the bounds: 1e-4 and more / 2e-11 and more)
  bn_stats_c8 mean 0.44, inv_std 0.50 float32 ulps; bn_fold b 4.0e-7, 0.45 of its bound
Wall time of the file on an MI355X: 4 s for the 243 tests (22 s with the library build in the first test's setup).

Each of these changes to a kernel makes tests of this file fail (tried, one at a time; none removes a bounds
guard):
  unbiased (n - 1) variance in bn_stats_finalize_kernel: test_bn_stats, 28 of 36 cases: all but the six of one
    element and the two whose only channel is the constant one;
  `per` rounded down in bn_stats_kernel: test_bn_stats, 22 of 36 cases: B HW no multiple of 64, except one element (nothing
    is summed, and mean = pivot, var = 0 is right) and the two whose only channel is the constant one;
  y0 and x0 swapped in bn_affine_window_kernel (clamped to the plane): test_bn_affine_windows, 8 of 12 cases: every window
    but the full plane and (100, 100, 30, 29), whose y0 equals its x0;
  mask bits 2 and 4 swapped in maxpool2x2_window_kernel: test_mask_bytes_of_special_windows, the fp32 cases of
    test_maxpool_forms (9 of 10; the 1 x 2 x 2 tie map is all-equal) and of test_pool_and_unpool_past_the_grid_cap;
  column flip dropped in deconv_gather_kernel (tap = (K - 1 - a) K + bb): all of test_deconv_gather, all of
    test_deconv_phase (the phase / gather comparison or the gather form itself), the capped-grid case;
  dy and dx swapped in deconv_phase_pack_kernel: 74 of the 86 cases of test_deconv_phase: all that run the phase
    kernel (eight fall to the gather kernel) but the four last-partial-period windows, which only the dy = dx = 1
    tap reaches;
  channels past C not zeroed in nchw_to_c8_kernel: test_c8_slice_converters for C in {1, 7, 9, 21} (8 of 12:
    8 and 16 have no padded lane);
  b = beta + mean s in bn_fold_kernel: all three cases of test_bn_fold."""
import functools

import numpy as np
import pytest
import torch

import bn_pool_ref as R
from _parity_helpers import GUARD, SENTINEL, Placed, host, same_bits

pytestmark = pytest.mark.gpu

DTYPES = {'f32': torch.float32, 'f64': torch.float64}
NPT = {'f32': np.float32, 'f64': np.float64}
U = {'f32': 2.0 ** -24, 'f64': 2.0 ** -53}
both_dtypes = pytest.mark.parametrize('dt', ['f32', 'f64'])


@pytest.fixture(scope='module')
def ops(built_lib):
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from iterative_inference_segm_amd import ops as _ops
    return _ops


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def stored(a, dt):
    """`a` as the kernel of that dtype is handed it, and the float64 values of that."""
    s = np.ascontiguousarray(a, dtype=NPT[dt])
    return s, s.astype(np.float64)


# ---- A. BatchNorm statistics -----------------------------------------------------------------------------------
FAMILIES = (('std', 0.5, 2.0), ('const', 0.1, 0.0), ('m30', 30.0, 0.05), ('m100', 100.0, 0.01),
            ('m1000', 1000.0, 1.0), ('m1e4', 1e4, 1.0))
BHW = ((1, 1, 1), (3, 3, 7), (2, 4, 8), (5, 1, 13), (1, 1, 257), (5, 29, 113))    # B, H, W: B HW = 1, 63, 64, 65, 257, 64 256 + 1
assert [b * h * w for b, h, w in BHW] == [1, 63, 64, 65, 257, 64 * 256 + 1]
STATS_C0 = 3


@functools.lru_cache(maxsize=None)
def _stats_case(k, n, dt):
    """A stack (B, c0 + n + 2, H, W) whose channel c0 + j is of family (j + k) mod 6, as stored in `dt`, and the
    fsum statistics of the stored values."""
    B, H, W = BHW[k]
    rng = np.random.default_rng(100 * k + n)
    x = rng.standard_normal((B, STATS_C0 + n + 2, H, W))
    fam = [FAMILIES[(j + k) % len(FAMILIES)] for j in range(n)]
    for j, (_, m, s) in enumerate(fam):
        x[:, STATS_C0 + j] = m + s * x[:, STATS_C0 + j]
    xs, x64 = stored(x, dt)
    # (the float32 entry point is handed eps as a C float)
    mean, inv_std = R.bn_stats(x64, STATS_C0, n, eps=float(np.float32(1e-4)) if dt == 'f32' else 1e-4)
    for a in (xs, mean, inv_std):
        a.setflags(write=False)
    return xs, [f[0] for f in fam], mean, inv_std


def _ulps(got, ref):
    """|got - ref| in float32 ulps of ref."""
    return np.abs(got.astype(np.float64) - ref) / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


@both_dtypes
@pytest.mark.parametrize('n', [1, 64, 65])
@pytest.mark.parametrize('k', range(len(BHW)), ids=['BHW%d' % (b * h * w) for b, h, w in BHW])
def test_bn_stats(ops, k, n, dt):
    """Channels [c0, c0 + n) of a wider stack (bstride > C HW): one element (var 0, inv_std = 1 / sqrt(eps)), fewer
    elements than chunks, a ragged last chunk, a second trip of the stage-1 loop; a second workgroup of the finalize
    (n = 65); a constant channel (the var < 0 clamp) and the four large-offset families."""
    xs, fam, mean_ref, inv_ref = _stats_case(k, n, dt)
    T, p = DTYPES[dt], Placed()
    x = p.inp(xs, T)
    ctot = x.shape[1]
    mean, inv_std = p.out((ctot,), T), p.out((ctot,), T)
    ops.bn_stats(x, STATS_C0, n, mean, inv_std)
    gm, gi = host(mean), host(inv_std)
    p.check()
    sl = slice(STATS_C0, STATS_C0 + n)
    outside = np.ones(ctot, bool)
    outside[sl] = False
    assert (gm[outside] == SENTINEL).all() and (gi[outside] == SENTINEL).all()
    if dt == 'f64':
        em = np.abs(gm[sl] - mean_ref) / np.abs(mean_ref)
        ei = np.abs(gi[sl] - inv_ref) / inv_ref
        bound, unit = 1e-12, 'relative'
    else:
        em, ei = _ulps(gm[sl], mean_ref), _ulps(gi[sl], inv_ref)
        bound, unit = 1.0, 'float32 ulps'
    for f in sorted(set(fam)):
        on = np.array([g == f for g in fam])
        print('bn_stats %s B HW %d n %d family %s: mean %.3e, inv_std %.3e %s (bound %g)'
              % (dt, xs.shape[0] * xs.shape[2] * xs.shape[3], n, f, em[on].max(), ei[on].max(), unit, bound))
    assert em.max() <= bound and ei.max() <= bound
    if xs.shape[0] * xs.shape[2] * xs.shape[3] == 1:
        assert same(gm[sl], xs[0, sl, 0, 0])                            # one element: the mean is that element
    for j, f in enumerate(fam):
        if f == 'const':                                                 # var is exactly 0, not a clamped negative
            assert gm[STATS_C0 + j] == xs[0, STATS_C0 + j, 0, 0] and abs(gi[STATS_C0 + j] - 100.0) <= 1e-5


# ---- B. bn_relu, bn_affine -------------------------------------------------------------------------------------
PLANES = ((1, 1), (15, 17), (16, 16), (1, 257), (129, 128))          # HW = 1, 255, 256, 257, 129 128 (> 64 blocks)


def _bn_params(rng, x64, dt):
    """Four channels: random with a negative gamma; normalised values all <= 0 (mean = the channel's maximum,
    beta 0); integer-valued everything (inv_std 0.5); random with a positive gamma.  As stored in `dt`."""
    beta = np.array([0.3, 0.0, -2.0, rng.standard_normal()])
    gamma = np.array([-1.7, 1.3, 3.0, 0.8])
    mean = np.array([0.4, x64[:, 1].max(), 1.0, rng.standard_normal()])
    inv_std = np.array([0.9, 2.1, 0.5, 1.0 + rng.random()])
    return [stored(v, dt) for v in (beta, gamma, mean, inv_std)]


def _bn_data(rng, shape, dt):
    x = rng.standard_normal(shape)
    x[:, 2] = rng.integers(-6, 7, size=x[:, 2].shape)
    return stored(x, dt)


def _bn_bound(x64, prm64, dt):
    beta, gamma, mean, inv_std = (v[None, :x64.shape[1], None, None] for v in prm64)
    return 4 * U[dt] * (np.abs(x64 - mean) * np.abs(gamma * inv_std) + np.abs(beta))


@both_dtypes
@pytest.mark.parametrize('H,W', PLANES)
def test_bn_relu(ops, H, W, dt):
    """The first 4 channels of a 6-channel stack into a dense output."""
    T, p = DTYPES[dt], Placed()
    rng = np.random.default_rng(H * W)
    xs, x64 = _bn_data(rng, (2, 6, H, W), dt)
    prm = _bn_params(rng, x64, dt)
    # (parameter vectors as long as the stack: the kernel reads entries [0, n) only)
    dv = [p.inp(np.concatenate([v[0], [7, 7]]).astype(NPT[dt]), T) for v in prm]
    out = ops.bn_relu(p.inp(xs, T), 4, *dv, out=p.out((2, 4, H, W), T))
    got = host(out)
    p.check()
    ref = R.bn_relu(x64, 4, *[v[1] for v in prm])
    err = np.abs(got - ref)
    bound = _bn_bound(x64[:, :4], [v[1] for v in prm], dt)
    print('bn_relu %s %dx%d: max |err| %.3e, max err / bound %.3f' % (dt, H, W, err.max(), (err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    assert not bits(got[:, 1]).any()                                  # exact +0.0, never -0.0
    assert same(got[:, 2], ref[:, 2].astype(NPT[dt]))
    assert H * W == 1 or ((got[:, 0] > 0).any() and (got[:, 0] == 0).any())


AFFINE_WINDOWS = (None, (7, 5, 1, 1), (129, 0, 1, 129), (0, 128, 130, 1), (100, 100, 30, 29), (1, 0, 129, 128))


def _run_affine(ops, H, W, window, dt):
    T, p = DTYPES[dt], Placed()
    rng = np.random.default_rng(H * W + (0 if window is None else sum(window)))
    xs, x64 = _bn_data(rng, (2, 4, H, W), dt)
    prm = _bn_params(rng, x64, dt)
    x = p.out((2, 4, H, W), T, xs)
    assert ops.bn_affine(x, tuple(p.inp(v[0], T) for v in prm), window=window) is x
    got = host(x)
    p.check()
    ref = R.bn_affine(x64, tuple(v[1] for v in prm), window)
    y0, x0, wh, ww = window if window is not None else (0, 0, H, W)
    outside = np.ones((H, W), bool)
    outside[y0:y0 + wh, x0:x0 + ww] = False
    assert np.array_equal(bits(got)[:, :, outside], bits(xs)[:, :, outside]), 'wrote outside the window'
    win = (slice(None), slice(None), slice(y0, y0 + wh), slice(x0, x0 + ww))
    err = np.abs(got - ref)[win]
    bound = _bn_bound(x64, [v[1] for v in prm], dt)[win]
    print('bn_affine %s %dx%d window %s: max |err| %.3e, max err / bound %.3f'
          % (dt, H, W, window, err.max(), (err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    assert same(got[:, 2], ref[:, 2].astype(NPT[dt]))
    assert (got[win][:, 1] <= 0).all()


@both_dtypes
@pytest.mark.parametrize('H,W', PLANES)
def test_bn_affine_planes(ops, H, W, dt):
    _run_affine(ops, H, W, None, dt)


@both_dtypes
@pytest.mark.parametrize('window', AFFINE_WINDOWS, ids=lambda w: 'full' if w is None else '%d_%d_%dx%d' % w)
def test_bn_affine_windows(ops, window, dt):
    """Full, one pixel, one row, one column, ending at the last row and column, and more than 16384 elements, of
    a 130 x 129 plane: the plane outside the window keeps its bits."""
    _run_affine(ops, 130, 129, window, dt)


# ---- C. pool and unpool forward --------------------------------------------------------------------------------
POOL_SHAPES = ((1, 2, 2), (3, 3, 3), (2, 2, 301), (5, 301, 2), (7, 9, 7))       # BC, H, W
POOL_BIG = (2, 2050, 2050)            # 2 x 1025 x 1025 outputs: one block past the 8192-block grid cap
UNPOOL_BIG = (1, 1449, 1449)          # 1449^2 outputs: one block past the cap, odd on both axes
assert 8192 < -(-POOL_BIG[0] * (POOL_BIG[1] // 2) * (POOL_BIG[2] // 2) // 256) < 8192 + 32
assert 8192 < -(-UNPOOL_BIG[1] * UNPOOL_BIG[2] // 256) < 8192 + 32


@functools.lru_cache(maxsize=None)
def _pool_data(shape, fam):
    """A float32-exact map (so the same values serve both dtypes), its pooled map and mask bytes, an `up`."""
    BC, H, W = shape
    rng = np.random.default_rng(BC * 1000 + H + W)
    if fam == 'ties':
        x = rng.integers(-2, 3, (1, BC, H, W)).astype(np.float32)
        up = rng.integers(-2, 3, (1, BC, H // 2, W // 2)).astype(np.float32)       # negative values, exact zeros
    else:
        x = rng.standard_normal((1, BC, H, W)).astype(np.float32)
        up = rng.standard_normal((1, BC, H // 2, W // 2)).astype(np.float32)
    pooled, mask = R.maxpool2x2(x, mask=np.zeros(up.shape, np.uint8))
    for a in (x, up, pooled, mask):
        a.setflags(write=False)
    return x, up, pooled, mask


def _pool_windows(h, w):
    wins = [(0, 0, h, w), (h - 1, w - 1, 1, 1), (h - 1, 0, 1, w), (0, w - 1, h, 1)]
    if h >= 3 and w >= 3:
        wins.append((1, 1, h - 2, w - 2))
    elif w >= 3:
        wins.append((0, 1, h, w - 2))
    elif h >= 3:
        wins.append((1, 0, h - 2, w))
    return sorted(set(wins))


def _unpool_windows(H, W):
    h2, w2 = H // 2 * 2, W // 2 * 2
    wins = [(0, 0, H, W), (H - 1, 0, 1, W), (0, W - 1, H, 1), (H - 1, W - 1, 1, 1)]      # (odd sizes: the border only)
    if H >= 3 and W >= 3:
        wins += [(h2 - 1 - (h2 == H), w2 - 1 - (w2 == W), 2, 2), (1, 1, H - 2, W - 2)]    # (odd: straddles 2h, 2w)
    return sorted(set(wins))


@both_dtypes
@pytest.mark.parametrize('fam', ['ties', 'random'])
@pytest.mark.parametrize('shape', POOL_SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_maxpool_forms(ops, shape, fam, dt):
    """maxpool2x2, its window form and (float32) its mask-byte form: the bits of the restatement inside the window,
    sentinels outside, in `out` and in `mask`."""
    x0, up0, pooled0, mask0 = _pool_data(shape, fam)
    T, nt = DTYPES[dt], NPT[dt]
    BC, H, W = shape
    h, w = H // 2, W // 2
    p = Placed()
    x = p.inp(x0, T)
    got = host(ops.maxpool2x2(x, out=p.out((1, BC, h, w), T)))
    assert same(got, pooled0.astype(nt))
    for win in _pool_windows(h, w):
        out = p.out((1, BC, h, w), T)
        ops.maxpool2x2(x, out=out, window=win)
        exp = R.maxpool2x2(x0.astype(nt), out=np.full((1, BC, h, w), SENTINEL, nt), window=win)
        assert same(host(out), exp), win
        if dt == 'f32':
            out, mask = p.out((1, BC, h, w), T), p.out((1, BC, h, w), torch.uint8)
            ops.maxpool2x2(x, out=out, window=win, mask=mask)
            expm = R.maxpool2x2(x0, out=np.full((1, BC, h, w), SENTINEL, nt), window=win,
                                mask=np.full((1, BC, h, w), SENTINEL & 0xFF, np.uint8))[1]
            assert same(host(out), exp) and same(host(mask), expm), win
    p.check()
    print('maxpool2x2 %s %s %s: bit-exact (max |err| 0)' % (dt, shape, fam))


@both_dtypes
@pytest.mark.parametrize('fam', ['ties', 'random'])
@pytest.mark.parametrize('shape', POOL_SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_unpool_forms(ops, shape, fam, dt):
    """unpool_eqmask and its window form: an odd last row and column are written as 0, `up` holds negative values
    and exact zeros, windows straddle the 2h / 2w border or are the border row alone."""
    x0, up0, pooled0, mask0 = _pool_data(shape, fam)
    T, nt = DTYPES[dt], NPT[dt]
    BC, H, W = shape
    p = Placed()
    up, pre, pooled = p.inp(up0, T), p.inp(x0, T), p.inp(pooled0, T)
    full = R.unpool_eqmask(up0, x0, pooled0).astype(nt)
    got = host(ops.unpool_eqmask(up, pre, pooled, out=p.out((1, BC, H, W), T)))
    assert same(got, full)
    assert not bits(got[:, :, H // 2 * 2:]).any() and not bits(got[:, :, :, W // 2 * 2:]).any()
    for win in _unpool_windows(H, W):
        out = p.out((1, BC, H, W), T)
        ops.unpool_eqmask(up, pre, pooled, out=out, window=win)
        exp = R.unpool_eqmask(up0.astype(nt), x0.astype(nt), pooled0.astype(nt),
                              out=np.full((1, BC, H, W), SENTINEL, nt), window=win)
        assert same(host(out), exp), win
    p.check()
    print('unpool_eqmask %s %s %s: bit-exact (max |err| 0)' % (dt, shape, fam))


@both_dtypes
def test_pool_and_unpool_past_the_grid_cap(ops, dt):
    T, nt = DTYPES[dt], NPT[dt]
    p = Placed()
    x0, up0, pooled0, mask0 = _pool_data(POOL_BIG, 'ties')
    BC, H, W = POOL_BIG
    x = p.inp(x0, T)
    assert same(host(ops.maxpool2x2(x, out=p.out(pooled0.shape, T))), pooled0.astype(nt))
    out = p.out(pooled0.shape, T)
    ops.maxpool2x2(x, out=out, window=(0, 0, H // 2, W // 2))
    assert same(host(out), pooled0.astype(nt))
    if dt == 'f32':
        out, mask = p.out(pooled0.shape, T), p.out(pooled0.shape, torch.uint8)
        ops.maxpool2x2(x, out=out, mask=mask)
        assert same(host(out), pooled0) and same(host(mask), mask0)
    p.check()
    del x, out, p
    p = Placed()
    x0, up0, pooled0, mask0 = _pool_data(UNPOOL_BIG, 'ties')
    BC, H, W = UNPOOL_BIG
    full = R.unpool_eqmask(up0, x0, pooled0).astype(nt)
    up, pre, pooled = p.inp(up0, T), p.inp(x0, T), p.inp(pooled0, T)
    assert same(host(ops.unpool_eqmask(up, pre, pooled, out=p.out(x0.shape, T))), full)
    out = p.out(x0.shape, T)
    ops.unpool_eqmask(up, pre, pooled, out=out, window=(0, 0, H, W))
    assert same(host(out), full)
    p.check()


def test_mask_bytes_of_special_windows(ops):
    """An all-equal window gives 15; a unique maximum in each of the four positions gives 1, 2, 4, 8; a map of
    negative values only; -0.0 against +0.0, which compare equal: both bits are set."""
    x = np.zeros((1, 7, 2, 2), np.float32)
    for k in range(4):
        x[0, k, k >> 1, k & 1] = 1.0
    x[0, 4] = 2.5
    x[0, 5] = [[-3.0, -1.0], [-1.0, -7.0]]
    x[0, 6] = [[-0.0, 0.0], [-1.0, -0.0]]
    p = Placed()
    out, mask = p.out((1, 7, 1, 1), torch.float32), p.out((1, 7, 1, 1), torch.uint8)
    ops.maxpool2x2(p.inp(x), out=out, mask=mask)
    got, gm = host(out), host(mask)
    p.check()
    assert list(gm.ravel()) == [1, 2, 4, 8, 15, 0b0110, 0b1011]
    ref, refm = R.maxpool2x2(x, mask=np.zeros((1, 7, 1, 1), np.uint8))
    assert same(gm, refm) and np.array_equal(got, ref) and list(got.ravel()) == [1, 1, 1, 1, 2.5, -1, 0]
    rng = np.random.default_rng(6)
    neg = -1.0 - rng.integers(0, 3, (2, 3, 9, 7)).astype(np.float32)
    p = Placed()
    out, mask = p.out((2, 3, 4, 3), torch.float32), p.out((2, 3, 4, 3), torch.uint8)
    ops.maxpool2x2(p.inp(neg), out=out, mask=mask)
    ref, refm = R.maxpool2x2(neg, mask=np.zeros((2, 3, 4, 3), np.uint8))
    assert same(host(out), ref) and same(host(mask), refm) and ref.max() < 0
    p.check()


# ---- D. transposed convolution ---------------------------------------------------------------------------------
def conv_tol(ref, K):
    return 2e-6 * np.sqrt(K) * (1.0 + np.abs(ref).max())        # (tests/test_gpu_ops.py)


def D(K, s, Cin, Cout, H, W, window=None, add=None, bias=True, form='phase', B=2, both=True):
    """add = (extra rows, extra columns, ay0, ax0): the skip tensor is the window's size plus the extras."""
    return dict(K=K, s=s, Cin=Cin, Cout=Cout, H=H, W=W, window=window, add=add, bias=bias, form=form, B=B, both=both)


def _did(c):
    return 'k%ds%d-%dto%d-%dx%d-%s%s%s-%s' % (c['K'], c['s'], c['Cin'], c['Cout'], c['H'], c['W'],
                                             'full' if c['window'] is None else 'w%d_%d_%dx%d' % c['window'],
                                             '-add' if c['add'] else '', '' if c['bias'] else '-nobias', c['form'])


PHASE_CASES = (
    # the CP = 12 / 16 switch at Cout 12 / 13, one channel on either side, both strides
    [D(2 * s, s, ci, co, 3, 4) for s in (2, 8) for ci, co in ((1, 1), (1, 12), (16, 13), (16, 16), (3, 12), (11, 5))]
    # inputs of one pixel, one row, one column
    + [D(2 * s, s, 3, 5, h, w) for s in (2, 8) for h, w in ((1, 1), (1, 9), (9, 1))]
    # ni nj = (H + 1) (W + 1) = 63, 64, 65 input positions: a wave short of one, full, and one over
    + [D(2 * s, s, 2, 3, h, w, B=1) for s in (2, 8) for h, w in ((6, 8), (7, 7), (4, 12))]
    # one-pixel windows at every phase of a period (s = 2), at the corner phases and an interior one (s = 8)
    + [D(4, 2, 3, 5, 4, 5, window=(4 + py, 6 + px, 1, 1)) for py in (0, 1) for px in (0, 1)]
    + [D(16, 8, 3, 5, 3, 4, window=(8 + py, 16 + px, 1, 1)) for py, px in ((0, 0), (0, 7), (7, 0), (7, 7), (3, 5))]
    # the last partial period only
    + [D(4, 2, 3, 5, 4, 5, window=(9, 11, 1, 1)), D(16, 8, 3, 5, 3, 4, window=(29, 35, 3, 5))]
    + [D(4, 2, 5, 11, 4, 5, bias=False), D(16, 8, 5, 11, 2, 3, bias=False)]
    # s = 2 with a skip tensor larger than the window at a non-zero offset; s = 8 with one runs the gather kernel
    + [D(4, 2, 11, 11, 7, 9, window=(3, 1, 7, 6), add=(3, 4, 2, 3)), D(4, 2, 16, 13, 5, 4, add=(1, 0, 1, 0)),
       D(16, 8, 4, 5, 3, 3, window=(5, 9, 17, 12), add=(3, 4, 2, 3), form='gather')]
    + [D(4, 2, 17, 5, 3, 4, form='gather'), D(4, 2, 5, 17, 3, 4, form='gather'), D(16, 8, 17, 3, 2, 2, form='gather')]
)
GATHER_CASES = (
    # both instantiations and the channel counts around their switch, with a window and an add
    [D(4, 2, 3, co, 5, 4, window=(1, 2, 9, 7), add=(2, 3, 1, 2), form='forced') for co in (1, 16, 17, 32)]
    # K not a multiple of the stride; K = s
    + [D(3, 2, 3, 5, 4, 5, form='gather'), D(5, 2, 2, 17, 3, 4, form='gather'), D(2, 2, 3, 5, 4, 3, form='gather'),
       D(3, 2, 2, 3, 4, 5, window=(2, 3, 6, 7), add=(1, 1, 0, 1), form='gather'),
       D(5, 2, 2, 3, 1, 1, form='gather'), D(3, 2, 4, 6, 5, 4, bias=False, form='gather'),
       D(4, 2, 3, 21, 4, 3, bias=False, form='forced')]
)


def _deconv_inputs(c, integer, dt):
    K, s, B, Cin, Cout, H, W = (c[k] for k in ('K', 's', 'B', 'Cin', 'Cout', 'H', 'W'))
    rng = np.random.default_rng(K * 1000 + Cin * 37 + Cout + H * 5 + W + integer)
    fh, fw = (H - 1) * s + K, (W - 1) * s + K
    oy0, ox0, oh, ow = c['window'] if c['window'] is not None else (0, 0, fh, fw)
    gen = (lambda lo, hi, shape: rng.integers(lo, hi + 1, shape).astype(np.float64)) if integer else \
        (lambda lo, hi, shape: rng.standard_normal(shape))
    x, Wt = gen(-3, 3, (B, Cin, H, W)), gen(-2, 2, (Cin, Cout, K, K))
    b = gen(-2, 2, (Cout,)) if c['bias'] else None
    other = gen(-5, 5, (B, Cout, oh + c['add'][0], ow + c['add'][1])) if c['add'] else None
    return [None if a is None else stored(a, dt) for a in (x, Wt, b, other)], (oy0, ox0, oh, ow)


def _run_deconv(ops, c, dt, monkeypatch):
    T = DTYPES[dt]
    worst = 0.0
    for integer in (True, False):
        (x, Wt, b, other), win = _deconv_inputs(c, integer, dt)
        oh, ow = win[2:]
        d = ops.Deconv(Wt[0], None if b is None else b[0], c['s'], dtype=T)
        kw = dict(window=win)
        p = Placed()
        if other is not None:
            kw.update(add=p.inp(other[0], T), add_off=c['add'][2:])
        xd = p.inp(x[0], T)
        monkeypatch.setattr(ops, 'DECONV_PHASE', c['form'] != 'forced')
        got = host(d(xd, out=p.out((c['B'], c['Cout'], oh, ow), T), **kw))
        assert d.last_form == ('gather' if c['form'] == 'forced' else c['form'])
        if c['form'] == 'phase' and c['both']:
            monkeypatch.setattr(ops, 'DECONV_PHASE', False)
            gather = host(d(xd, out=p.out((c['B'], c['Cout'], oh, ow), T), **kw))
            assert d.last_form == 'gather'
            assert same(got, gather), 'phase and gather forms differ: %g' % np.abs(got - gather).max()
        monkeypatch.setattr(ops, 'DECONV_PHASE', True)
        p.check()
        ref = R.deconv(x[1], Wt[1], None if b is None else b[1], c['s'], add=None if other is None else other[1],
                       add_off=(c['add'] or (0, 0, 0, 0))[2:], window=win)
        assert got.shape == ref.shape
        if integer:
            assert same(got.astype(np.float64), ref)
        else:
            taps = (-(-c['K'] // c['s'])) ** 2
            err = np.abs(got - ref).max()
            worst = max(worst, err)
            assert err <= conv_tol(ref, taps * c['Cin'])
            if dt == 'f64':
                assert err <= 1e-12 * (1.0 + np.abs(ref).max())
    print('deconv %s %s: integer data exact, random data max |err| %.3e' % (_did(c), dt, worst))


@both_dtypes
@pytest.mark.parametrize('c', PHASE_CASES, ids=_did)
def test_deconv_phase(ops, c, dt, monkeypatch):
    _run_deconv(ops, c, dt, monkeypatch)


@both_dtypes
@pytest.mark.parametrize('c', GATHER_CASES, ids=_did)
def test_deconv_gather(ops, c, dt, monkeypatch):
    _run_deconv(ops, c, dt, monkeypatch)


def test_deconv_gather_past_the_grid_cap(ops):
    """2048 x 2050 output pixels of one channel: 16 blocks more than the 16384 of the capped grid."""
    H, W = 1024, 1025
    assert -(-(2 * H) * (2 * W) // 256) == 16384 + 16
    rng = np.random.default_rng(12)
    x = rng.integers(-3, 4, (1, 1, H, W)).astype(np.float32)
    Wt = np.array([[[[1, -2], [3, 2]]]], np.float32)
    p = Placed()
    d = ops.Deconv(Wt, np.array([-1], np.float32), 2)
    got = host(d(p.inp(x), out=p.out((1, 1, 2 * H, 2 * W), torch.float32)))
    p.check()
    assert d.last_form == 'gather'
    assert same(got.astype(np.float64), R.deconv(x, Wt, [-1.0], 2))


# ---- E. C8 helpers ---------------------------------------------------------------------------------------------
C8TOT = 5


def _c8_np(t):
    return host(t.float())


@pytest.mark.parametrize('H,W', [(3, 5), (17, 19)])
@pytest.mark.parametrize('C', [1, 7, 8, 9, 16, 21])
def test_c8_slice_converters(ops, C, H, W):
    """Into / out of chunk plane c8_0 in {0, 1, last} of a 5-plane tensor: bf16 round-to-nearest-even of the input
    (half-way cases among them), zero lanes past C in the last written chunk, the other planes' bits unchanged; the
    reverse direction writes C channels and nothing behind them."""
    rng = np.random.default_rng(C * 100 + H)
    x0 = rng.standard_normal((2, C, H, W)).astype(np.float32)
    x0[0, 0, 0, :5] = [1.00390625, 1.01171875, -1.00390625, 1.0 + 2.0 ** -9, -0.0]     # (ties to even: 1, 1.015625, -1)
    n8 = (C + 7) // 8
    init = rng.standard_normal((2, C8TOT, H, W, 8)).astype(np.float32)
    init = R.bf16_round(init)
    for c8_0 in sorted({0, 1, C8TOT - n8}):
        p = Placed()
        out8 = p.out((2, C8TOT, H, W, 8), torch.bfloat16, torch.from_numpy(init).to(torch.bfloat16))
        assert ops.nchw_to_c8_slice(p.inp(x0), out8, c8_0 * 8) is out8
        got = _c8_np(out8)
        p.check()
        ref = R.nchw_to_c8_slice(x0, init, c8_0 * 8)
        assert same(got, ref), (C, c8_0)
        assert got[0, c8_0, 0, 0, 0] == 1.0 and got[0, c8_0, 0, 1, 0] == 1.015625 and got[0, c8_0, 0, 2, 0] == -1.0
        # the reverse direction from the tensor just written (whose other planes hold random bf16 values)
        src = p.inp(out8.clone())
        back = ops.c8_slice_to_nchw(src, c8_0 * 8, C, out=p.out((2, C, H, W), torch.float32))
        gb = host(back)
        p.check()
        assert same(gb, R.c8_slice_to_nchw(ref, c8_0 * 8, C)) and same(gb, R.bf16_round(x0))


C8_STATS = ((1, 1, 1), (1, 15, 17), (3, 3, 3641))        # B, H, W: B HW = 1, 255, 256 128 + 1
assert [b * h * w for b, h, w in C8_STATS] == [1, 255, 256 * 128 + 1]


@pytest.mark.parametrize('B,H,W', C8_STATS)
@pytest.mark.parametrize('c0,n', [(8, 8), (16, 16)])
def test_bn_stats_c8(ops, B, H, W, c0, n):
    """Channels [c0, c0 + n), c0 > 0, of a 4-plane C8 tensor against the fsum statistics of the STORED bf16 values:
    two float32 ulps for the channels with m^2 / (var + eps) <= 1e7.  bn_stats_c8 keeps the one-pass variance in
    double (relative error about 2^-53 m^2 / (var + eps)), so past that limit -- a channel of mean 100 and spread
    0.01 -- nothing is claimed; the families here (0.5 +- 2, 30 +- 0.05, 1000 +- 1, a constant) are all below it."""
    rng = np.random.default_rng(B * H * W + c0)
    fam = ((0.5, 2.0), (30.0, 0.05), (1000.0, 1.0), (0.75, 0.0))
    x = rng.standard_normal((B, 32, H, W))
    for c in range(32):
        m, s = fam[c % 4]
        x[:, c] = m + s * x[:, c]
    x8 = R.bf16_round(x.astype(np.float32)).reshape(B, 4, 8, H, W).transpose(0, 1, 3, 4, 2)
    mean_ref, inv_ref = R.bn_stats_c8(x8, c0, n)
    ratio = mean_ref ** 2 * inv_ref ** 2
    ok = ratio <= 1e7
    assert ok.sum() >= n // 2 and (ok.all() or B * H * W == 1)      # (one element: var 0, and 1000^2 / eps is 1e10)
    p = Placed()
    # (copied into a fresh tensor: a 1 x 1 map from numpy carries strides that c8_ctot does not take for contiguous)
    buf = p.inp(torch.empty(x8.shape, dtype=torch.bfloat16).copy_(torch.from_numpy(np.ascontiguousarray(x8))))
    assert same(_c8_np(buf), np.ascontiguousarray(x8))
    mean, inv_std = p.out((32,), torch.float32), p.out((32,), torch.float32)
    ops.bn_stats_c8(buf, c0, n, mean, inv_std)
    gm, gi = host(mean), host(inv_std)
    p.check()
    outside = np.ones(32, bool)
    outside[c0:c0 + n] = False
    assert (gm[outside] == SENTINEL).all() and (gi[outside] == SENTINEL).all()
    em, ei = _ulps(gm[c0:c0 + n], mean_ref)[ok], _ulps(gi[c0:c0 + n], inv_ref)[ok]
    print('bn_stats_c8 B HW %d c0 %d n %d: mean %.3f, inv_std %.3f float32 ulps (bound 2), largest m^2/(var+eps) %.2e'
          % (B * H * W, c0, n, em.max(), ei.max(), ratio[ok].max()))
    assert em.max() <= 2 and ei.max() <= 2


@pytest.mark.parametrize('n', [1, 256, 257])
def test_bn_fold(ops, n):
    rng = np.random.default_rng(n)
    beta, gamma, mean = (rng.standard_normal(n + 3).astype(np.float32) for _ in range(3))
    mean += np.float32(0.5) * np.sign(mean)                                # (|mean| >= 0.5: its sign matters)
    inv_std = (0.5 + rng.random(n + 3)).astype(np.float32)
    p = Placed()
    a, b = p.out((n + 3,), torch.float32), p.out((n + 3,), torch.float32)
    ops.bn_fold(p.inp(beta), p.inp(gamma), p.inp(mean), p.inp(inv_std), n, a=a, b=b)
    ga, gb = host(a), host(b)
    p.check()
    assert (ga[n:] == SENTINEL).all() and (gb[n:] == SENTINEL).all()
    assert same(ga[:n], (gamma * inv_std)[:n])
    ref = beta[:n].astype(np.float64) - mean[:n].astype(np.float64) * ga[:n].astype(np.float64)
    bound = 2 * U['f32'] * (np.abs(beta[:n]) + np.abs(mean[:n].astype(np.float64) * ga[:n]))
    err = np.abs(gb[:n] - ref)
    print('bn_fold n %d: max |err| of b %.3e, max err / bound %.3f' % (n, err.max(), (err / bound).max()))
    assert (err <= bound).all()
    ra, rb = R.bn_fold(beta, gamma, mean, inv_std, n)
    assert np.abs(ga[:n] - ra).max() <= 1e-6 and np.abs(gb[:n] - rb).max() <= 1e-6


# ---- F. refusals -----------------------------------------------------------------------------------------------
@both_dtypes
def test_out_of_range_requests_are_refused(ops, dt):
    """One out-of-range request per entry point: a RuntimeError (the IISEG_ERR_* of the C ABI), nothing written."""
    T = DTYPES[dt]
    p = Placed()
    rng = np.random.default_rng(1)
    x = p.inp(rng.standard_normal((2, 3, 6, 8)), T)
    vec = lambda n=3: p.inp(rng.standard_normal(n), T)
    refused = []

    def refuse(what, fn):
        with pytest.raises(RuntimeError, match='iiseg_status'):
            fn()
        refused.append(what)
        assert p.nothing_written(), what

    pooled, up = p.inp(rng.standard_normal((2, 3, 3, 4)), T), p.inp(rng.standard_normal((2, 3, 3, 4)), T)
    refuse('maxpool window', lambda: ops.maxpool2x2(x, out=p.out((2, 3, 3, 4), T), window=(1, 2, 3, 2)))
    refuse('maxpool window', lambda: ops.maxpool2x2(x, out=p.out((2, 3, 3, 4), T), window=(0, 3, 1, 2)))
    if dt == 'f32':
        refuse('mask window', lambda: ops.maxpool2x2(x, out=p.out((2, 3, 3, 4), T), window=(3, 0, 1, 1),
                                                     mask=p.out((2, 3, 3, 4), torch.uint8)))
    refuse('unpool window', lambda: ops.unpool_eqmask(up, x, pooled, out=p.out((2, 3, 6, 8), T), window=(5, 0, 2, 8)))
    refuse('bn_affine window', lambda: ops.bn_affine(p.out((2, 3, 6, 8), T), (vec(), vec(), vec(), vec()),
                                                     window=(0, 7, 6, 2)))
    # bstride = Ctot HW < C HW: more channels asked for than the stack has
    refuse('bn_stats bstride', lambda: ops.bn_stats(x, 0, 4, p.out((8,), T), p.out((8,), T)))
    refuse('bn_relu bstride', lambda: ops.bn_relu(x, 4, vec(4), vec(4), vec(4), vec(4), out=p.out((2, 4, 6, 8), T)))
    for K, s, form in ((4, 2, 'phase'), (3, 2, 'gather')):
        d = ops.Deconv(rng.standard_normal((3, 5, K, K)), rng.standard_normal(5), s, dtype=T)
        fh, fw = d.out_hw(6, 8)
        refuse('deconv window', lambda: d(x, window=(1, 0, fh, fw), out=p.out((2, 5, fh, fw), T)))
        refuse('deconv window', lambda: d(x, window=(0, fw - 3, 4, 4), out=p.out((2, 5, 4, 4), T)))
        add = p.inp(rng.standard_normal((2, 5, 6, 7)), T)
        refuse('deconv add', lambda: d(x, window=(2, 3, 5, 6), add=add, add_off=(2, 1), out=p.out((2, 5, 5, 6), T)))
        refuse('deconv add', lambda: d(x, window=(2, 3, 5, 6), add=add, add_off=(0, 2), out=p.out((2, 5, 5, 6), T)))
        assert d.last_form is None                                         # (neither kernel ran)
    if dt == 'f32':
        c8 = lambda planes: p.out((2, planes, 6, 8, 8), torch.bfloat16)
        src8 = p.inp(torch.zeros((2, 3, 6, 8, 8), dtype=torch.bfloat16))
        x9 = p.inp(rng.standard_normal((2, 9, 6, 8)), T)
        refuse('nchw_to_c8_slice', lambda: ops.nchw_to_c8_slice(x9, c8(3), 16))         # planes 2, 3 of 3
        refuse('c8_slice_to_nchw', lambda: ops.c8_slice_to_nchw(src8, 16, 9, out=p.out((2, 9, 6, 8), T)))
        refuse('bn_stats_c8', lambda: ops.bn_stats_c8(src8, 16, 16, p.out((32,), T), p.out((32,), T)))
        refuse('bn_fold', lambda: ops.bn_fold(vec(), vec(), vec(), vec(), 0, a=p.out((3,), T), b=p.out((3,), T)))
    p.check()
    print('refused (%s): %s' % (dt, ', '.join(refused)))
