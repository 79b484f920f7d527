"""The float64 restatements of tests/bn_pool_ref.py against the oracle and against torch CPU float64, to 1e-12:
what makes them trustworthy as the reference of tests/test_gpu_bn_pool_deconv_edges.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_pool_ref as R
from oracle import dae as odae
from oracle import densenet as oden
from oracle import nn as onn

TOL = 1e-12


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / (1.0 + np.abs(np.asarray(b)).max()))


# ---- BatchNorm -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,c0,n', [((3, 10, 9, 7), 0, 10), ((2, 7, 5, 3), 2, 4), ((1, 3, 1, 1), 1, 1)])
def test_bn_stats_and_bn_relu_are_the_oracle_batchnorm(shape, c0, n):
    rng = np.random.default_rng(sum(shape))
    x = 0.5 + 2 * rng.standard_normal(shape)
    beta, gamma = rng.standard_normal(n), rng.standard_normal(n)            # (negative gammas among them)
    mean, inv_std = R.bn_stats(x, c0, n)
    sl = x[:, c0:c0 + n]
    assert _rel(mean, sl.mean(axis=(0, 2, 3))) <= TOL
    assert _rel(inv_std, 1.0 / np.sqrt(sl.var(axis=(0, 2, 3)) + 1e-4)) <= TOL
    got = R.bn_relu(sl, n, beta, gamma, mean, inv_std)
    assert _rel(got, oden._bn_relu(sl, beta, gamma)) <= TOL
    assert _rel(got, np.maximum(onn.batchnorm_batchstats(sl, beta, gamma), 0)) <= TOL
    if sl[:, 0].size > 1:                                  # (torch refuses batch statistics of one value)
        ref = F.relu(F.batch_norm(_t(sl), None, None, _t(gamma), _t(beta), training=True, eps=1e-4)).numpy()
        assert _rel(got, ref) <= TOL
    # the first n channels of a wider stack, longer parameter vectors
    pad = lambda v: np.concatenate([v, [7.0, 7.0]])
    wide = np.concatenate([sl, rng.standard_normal((shape[0], 2) + shape[2:])], axis=1)
    assert np.array_equal(R.bn_relu(wide, n, pad(beta), pad(gamma), pad(mean), pad(inv_std)), got)


def test_bn_stats_is_shift_invariant_where_one_pass_is_not():
    """The families of the GPU test: the fsum two-pass form agrees with numpy's two-pass var to 1e-12 and gives the
    exact answers for a constant channel and a single element."""
    rng = np.random.default_rng(5)
    for m, s in ((30, 0.05), (100, 0.01), (1000, 1), (1e4, 1)):
        x = (m + s * rng.standard_normal((2, 1, 64, 129)))
        mean, inv_std = R.bn_stats(x, 0, 1)
        ref = 1.0 / np.sqrt(x.var() + 1e-4)
        assert abs(inv_std[0] - ref) <= TOL * ref and abs(mean[0] - x.mean()) <= TOL * m
    mean, inv_std = R.bn_stats(np.full((2, 1, 5, 3), 0.1), 0, 1)
    assert mean[0] == 0.1 and inv_std[0] == 1.0 / np.sqrt(1e-4)
    mean, inv_std = R.bn_stats(np.full((1, 1, 1, 1), -3.25), 0, 1, eps=0.25)
    assert mean[0] == -3.25 and inv_std[0] == 2.0


@pytest.mark.parametrize('window', [None, (0, 0, 6, 5), (2, 3, 1, 1), (5, 0, 1, 5), (0, 4, 6, 1), (3, 2, 3, 3)])
def test_bn_affine_is_the_oracle_stored_average_batchnorm_on_its_window(window):
    rng = np.random.default_rng(8)
    x = rng.standard_normal((2, 3, 6, 5))
    bnp = tuple(rng.standard_normal(3) for _ in range(3)) + (rng.random(3) + 0.5,)
    got = R.bn_affine(x, bnp, window)
    y0, x0, h, w = window or (0, 0, 6, 5)
    ref = x.copy()
    ref[:, :, y0:y0 + h, x0:x0 + w] = odae._bn_avg(x, bnp)[:, :, y0:y0 + h, x0:x0 + w]
    assert _rel(got, ref) <= TOL
    outside = np.ones(x.shape, bool)
    outside[:, :, y0:y0 + h, x0:x0 + w] = False
    assert np.array_equal(got[outside], x[outside])
    beta, gamma, mean, inv_std = bnp
    t = F.batch_norm(_t(x), _t(mean), _t(1.0 / inv_std ** 2 - 1e-4), _t(gamma), _t(beta), training=False, eps=1e-4).numpy()
    assert _rel(got[:, :, y0:y0 + h, x0:x0 + w], t[:, :, y0:y0 + h, x0:x0 + w]) <= TOL


def test_bn_fold_gives_bn_relu():
    rng = np.random.default_rng(9)
    x = rng.standard_normal((2, 5, 4, 3))
    beta, gamma, mean = (rng.standard_normal(7) for _ in range(3))
    inv_std = rng.random(7) + 0.5
    a, b = R.bn_fold(beta, gamma, mean, inv_std, 5)
    assert a.shape == b.shape == (5,)
    got = np.maximum(a[None, :, None, None] * x + b[None, :, None, None], 0)
    assert _rel(got, R.bn_relu(x, 5, beta, gamma, mean, inv_std)) <= TOL


# ---- pool / unpool ---------------------------------------------------------------------------------------------
def _eq_bits(pre, pooled):
    """The byte form of the DePool2D mask as tests/test_gpu_ops.py and tests/test_gpu_f64.py build it from host
    arrays (restated here: one test module does not import another)."""
    B, Cc, H, W = pre.shape
    h2, w2 = H // 2, W // 2
    m = np.zeros((B, Cc, h2, w2), np.uint8)
    for dy in (0, 1):
        for dx in (0, 1):
            eq = pre[:, :, dy:2 * h2:2, dx:2 * w2:2] == pooled
            m |= (eq.astype(np.uint8) << (dy * 2 + dx))
    return m


@pytest.mark.parametrize('shape', [(1, 1, 2, 2), (2, 3, 3, 3), (1, 2, 2, 9), (2, 2, 7, 4), (3, 2, 9, 7)])
def test_maxpool_and_mask_bytes_on_forced_ties(shape):
    rng = np.random.default_rng(sum(shape))
    x = rng.integers(-2, 3, shape).astype(np.float64)                  # five values: most windows hold a tie
    ref = onn.maxpool2(x)
    assert np.array_equal(R.maxpool2x2(x), ref)
    assert np.array_equal(R.maxpool2x2(x), F.max_pool2d(_t(x), 2).numpy())
    out, mask = R.maxpool2x2(x, mask=np.zeros(ref.shape, np.uint8))
    assert np.array_equal(out, ref) and np.array_equal(mask, _eq_bits(x, ref))
    assert mask.min() >= 1 and (np.unpackbits(mask[..., None], axis=-1).sum(-1) > 1).any()        # ties are there
    # the byte mask says what the materialised DePool2D multiplies with
    up = rng.standard_normal(ref.shape)
    un = R.unpool_eqmask(up, x, ref)
    assert np.array_equal(un, onn.depool_eqmask(up, x, ref))
    h, w = ref.shape[2:]
    for k in range(4):
        dy, dx = k >> 1, k & 1
        assert np.array_equal(un[:, :, dy:2 * h:2, dx:2 * w:2], np.where((mask >> k) & 1, up, 0.0))
    assert not un[:, :, 2 * h:].any() and not un[:, :, :, 2 * w:].any()


def test_mask_bit_positions_and_signed_zeros():
    x = np.zeros((1, 4, 2, 2))
    for k in range(4):
        x[0, k, k >> 1, k & 1] = 1.0                                   # a unique maximum in each of the positions
    _, mask = R.maxpool2x2(x, mask=np.zeros((1, 4, 1, 1), np.uint8))
    assert list(mask.ravel()) == [1, 2, 4, 8]
    _, mask = R.maxpool2x2(np.full((1, 1, 2, 2), -3.0), mask=np.zeros((1, 1, 1, 1), np.uint8))
    assert mask.item() == 15
    _, mask = R.maxpool2x2(np.array([[[[-0.0, 0.0], [-1.0, -0.0]]]]), mask=np.zeros((1, 1, 1, 1), np.uint8))
    assert mask.item() == 0b1011


def test_pool_and_unpool_windows_write_their_window_only():
    rng = np.random.default_rng(3)
    x = rng.integers(-3, 4, (2, 2, 9, 7)).astype(np.float64)
    full, fmask = R.maxpool2x2(x, mask=np.zeros((2, 2, 4, 3), np.uint8))
    for win in [(0, 0, 4, 3), (1, 2, 1, 1), (3, 0, 1, 3), (0, 2, 4, 1), (1, 1, 2, 1)]:
        y0, x0, h, w = win
        out, mask = R.maxpool2x2(x, out=np.full(full.shape, -9.0), window=win, mask=np.full(full.shape, 0xAA, np.uint8))
        exp, expm = np.full(full.shape, -9.0), np.full(full.shape, 0xAA, np.uint8)
        exp[:, :, y0:y0 + h, x0:x0 + w] = full[:, :, y0:y0 + h, x0:x0 + w]
        expm[:, :, y0:y0 + h, x0:x0 + w] = fmask[:, :, y0:y0 + h, x0:x0 + w]
        assert np.array_equal(out, exp) and np.array_equal(mask, expm)
        assert np.array_equal(R.maxpool2x2(x, out=np.full(full.shape, -9.0), window=win), exp)
    up = rng.standard_normal(full.shape)
    un = onn.depool_eqmask(up, x, full)
    for win in [(0, 0, 9, 7), (8, 0, 1, 7), (7, 5, 2, 2), (0, 6, 9, 1), (3, 2, 4, 3)]:
        y0, x0, h, w = win
        got = R.unpool_eqmask(up, x, full, out=np.full(x.shape, -9.0), window=win)
        exp = np.full(x.shape, -9.0)
        exp[:, :, y0:y0 + h, x0:x0 + w] = un[:, :, y0:y0 + h, x0:x0 + w]
        assert np.array_equal(got, exp)


# ---- transposed convolution ------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,s,Cin,Cout,H,W', [(4, 2, 3, 5, 4, 3), (16, 8, 2, 3, 2, 3), (3, 2, 2, 2, 3, 4), (5, 2, 1, 2, 3, 2),
                                               (2, 2, 2, 1, 3, 3), (4, 2, 1, 1, 1, 1), (4, 2, 2, 17, 1, 5)])
def test_deconv_is_the_oracle_and_the_flipped_conv_transpose(K, s, Cin, Cout, H, W):
    rng = np.random.default_rng(K * 10 + s + Cout)
    x, Wt, b = rng.standard_normal((2, Cin, H, W)), rng.standard_normal((Cin, Cout, K, K)), rng.standard_normal(Cout)
    ref = onn.deconv2d(x, Wt, b, stride=s)
    got = R.deconv(x, Wt, b, s)
    assert got.shape == ref.shape and _rel(got, ref) <= TOL
    t = F.conv_transpose2d(_t(x), _t(Wt[:, :, ::-1, ::-1]), _t(b), stride=s).numpy()
    assert _rel(got, t) <= TOL
    assert _rel(R.deconv(x, Wt, None, s), onn.deconv2d(x, Wt, None, stride=s)) <= TOL
    # the centre-cropped sum of the FCN-8 skips: a window, and an add larger than the window at an offset
    fh, fw = ref.shape[2:]
    oh, ow = max(fh - 3, 1), max(fw - 2, 1)
    other = rng.standard_normal((2, Cout, fh + 4, fw + 1))
    ref2 = onn.center_crop(ref, oh, ow) + onn.center_crop(other, oh, ow)
    got2 = R.deconv(x, Wt, b, s, add=other, add_off=((fh + 4 - oh) // 2, (fw + 1 - ow) // 2),
                    window=((fh - oh) // 2, (fw - ow) // 2, oh, ow))
    assert _rel(got2, ref2) <= TOL
    assert _rel(R.deconv(x, Wt, b, s, window=(fh - 1, fw - 1, 1, 1)), ref[:, :, -1:, -1:]) <= TOL


# ---- bf16 C8 ---------------------------------------------------------------------------------------------------
def test_bf16_round_is_round_to_nearest_even():
    rng = np.random.default_rng(4)
    x = np.concatenate([rng.standard_normal(4096).astype(np.float32) * 50,
                        np.array([1.00390625, 1.01171875, -1.00390625, 1.0, 0.0, -0.0, 3.3895314e38, 1e-40],
                                 np.float32)])
    ref = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
    got = R.bf16_round(x)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    # the half-way cases: 1 + 2^-8 lies between 1 and 1 + 2^-7 and goes to the even 1; 1 + 3 * 2^-8 goes up
    assert got[4096] == 1.0 and got[4097] == 1.015625 and got[4098] == -1.0


@pytest.mark.parametrize('C', [1, 7, 8, 9, 16, 21])
def test_c8_slices_round_trip(C):
    rng = np.random.default_rng(C)
    x = rng.standard_normal((2, C, 3, 5)).astype(np.float32)
    n8 = (C + 7) // 8
    for c8_0 in (0, 1, 5 - n8):
        wide = np.full((2, 5, 3, 5, 8), 7.0, np.float32)
        got = R.nchw_to_c8_slice(x, wide, c8_0 * 8)
        xb = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
        for c in range(n8 * 8):
            plane = got[:, c8_0 + c // 8, :, :, c % 8]
            assert np.array_equal(plane, xb[:, c] if c < C else np.zeros_like(plane))
        untouched = [p for p in range(5) if not c8_0 <= p < c8_0 + n8]
        assert (got[:, untouched] == 7.0).all()
        back = R.c8_slice_to_nchw(got, c8_0 * 8, C)
        assert back.shape == x.shape and np.array_equal(back, xb)
        m, i = R.bn_stats_c8(got, c8_0 * 8, n8 * 8)
        m2, i2 = R.bn_stats(np.concatenate([xb, np.zeros((2, n8 * 8 - C, 3, 5))], axis=1), 0, n8 * 8)
        assert np.array_equal(m, m2) and np.array_equal(i, i2)
