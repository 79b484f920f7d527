"""The float64 restatements of tests/tail_ref.py against the oracle and against torch float64 autograd on the
CPU, to 1e-12: what makes them trustworthy as the reference of tests/test_gpu_tail_edges.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tail_ref as R
from oracle import metrics as ometrics
from oracle import nn as onn
from oracle import torch_cpu as otc

TOL = 1e-12


def _t(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).requires_grad_(grad)


@pytest.mark.parametrize('C', [1, 2, 11, 17, 32])
def test_crop_softmax_is_the_oracle_softmax_of_the_centre_crop(C):
    rng = np.random.default_rng(C)
    score = 5 * rng.standard_normal((2, C, 30, 29))
    y = rng.random((2, C, 24, 20))
    ref = onn.softmax_channels(onn.center_crop(score, 24, 20))
    assert np.abs(R.crop_softmax(score, 24, 20) - ref).max() <= TOL
    assert np.abs(R.crop_softmax(score, 24, 20, off=(3, 4)) - ref).max() <= TOL      # = (30-24)//2, (29-20)//2
    assert np.abs(R.crop_softmax(score, 24, 20, minuend=y) - (y - ref)).max() <= TOL
    # an explicit offset is the window that starts there
    ref = onn.softmax_channels(score[:, :, 6:30, 0:20])
    assert np.abs(R.crop_softmax(score, 24, 20, off=(6, 0)) - ref).max() <= TOL


def test_refine_step_and_grad_step_follow_their_definitions():
    rng = np.random.default_rng(2)
    B, C, H, W = 3, 5, 6, 7
    score = 3 * rng.standard_normal((B, C, H + 2, W + 3))
    y = rng.random((B, C, H, W))
    gt = rng.uniform(-1, 1, (B, C, H, W))
    r = onn.softmax_channels(onn.center_crop(score, H, W))
    active = np.array([1, 0, 1])
    new, norms = R.refine_step(score, y, active, 0.3)
    de = y - r
    assert np.abs(new[[0, 2]] - np.clip(y - 0.3 * de, 0, 1)[[0, 2]]).max() <= TOL
    assert np.array_equal(new[1], y[1])                                  # stopped: unchanged ...
    assert np.abs(norms - np.linalg.norm(de, axis=1).mean(axis=(1, 2))).max() <= TOL     # ... its norm still there
    new, norms = R.grad_step(score, gt, y, active, 0.5)
    g = gt - 2 * (r - y)
    assert np.abs(new[[0, 2]] - np.clip(y - 0.5 * g, 0, 1)[[0, 2]]).max() <= TOL
    assert np.array_equal(new[1], y[1])
    assert np.abs(norms - np.linalg.norm(g, axis=1).mean(axis=(1, 2))).max() <= TOL
    assert new.min() >= 0 and new.max() <= 1 and (new == 0).any() and (new == 1).any()     # the clip is reached


@pytest.mark.parametrize('C', [1, 2, 11, 21])
def test_sqerr_softmax_bwd_against_autograd(C):
    rng = np.random.default_rng(30 + C)
    score = 4 * rng.standard_normal((2, C, 9, 8))
    y = rng.random((2, C, 5, 6))
    s = _t(score, grad=True)
    ((torch.softmax(s[:, :, 1:6, 2:8], dim=1) - _t(y)) ** 2).sum().backward()
    ref = s.grad.numpy()
    got = R.sqerr_softmax_bwd(score, y, off=(1, 2))
    assert np.abs(got - ref[:, :, 1:6, 2:8]).max() <= TOL
    ref[:, :, 1:6, 2:8] = 0
    assert not ref.any()                                                 # (nothing outside the window)


def test_finalize():
    act, it, last = R.finalize([6.0, 99.0, 1.0, 2.0], [1, 0, 1, 1], [4, 7, 0, 2], [9.0, 8.0, 7.0, 6.0], 4, 0.5)
    assert list(act) == [1, 0, 0, 1]                   # 1.5 >= eps; stopped before; 0.25 < eps; 0.5 == eps stays
    assert list(it) == [5, 7, 1, 3]
    assert list(last) == [1.5, 8.0, 0.25, 0.5]


@pytest.mark.parametrize('C', [1, 11, 16])
def test_confusion_against_val_fn(C):
    rng = np.random.default_rng(40 + C)
    B, H, W = 2, 9, 13
    y = rng.random((B, C, H, W))
    y /= y.sum(1, keepdims=True)
    y[0, :, 0, 0] = 1.0 / C                            # all tied: index 0
    if C > 2:
        y[0, :, 0, 1] = 0.0
        y[0, [1, 2], 0, 1] = 0.5                       # two tied non-zero classes: the lower index
    labels = rng.integers(0, C + 1, size=(B, H, W))
    t = np.zeros((B, C + 1, H, W))
    np.put_along_axis(t, labels[:, None], 1.0, axis=1)
    acc_ref, jacc_ref, mse_ref = ometrics.val_fn(y, t, C, [C])
    cm, sums = R.confusion(y, t)
    assert cm.shape == (C, C + 1) and cm.dtype == np.int64 and cm.sum() == B * H * W
    assert cm[:, C].sum() == (labels == C).sum()
    nonvoid = cm[:, :C].astype(np.float64)
    tp = np.diag(nonvoid)
    assert np.array_equal(np.stack([tp, nonvoid.sum(1) + nonvoid.sum(0) - tp]), jacc_ref)
    assert abs(tp.sum() / nonvoid.sum() - acc_ref) <= TOL
    assert abs(sums[0] / sums[1] - mse_ref) <= TOL
    # `active` switches whole images off
    cm1, sums1 = R.confusion(y, t, active=[0, 1])
    cm_b, sums_b = R.confusion(y[1:], t[1:])
    assert np.array_equal(cm1, cm_b) and np.array_equal(sums1, sums_b)


@pytest.mark.parametrize('shape', [(1, 1, 2, 2), (2, 3, 9, 7), (1, 2, 6, 11)])
@pytest.mark.parametrize('ties', [False, True])
@pytest.mark.parametrize('depool', [onn.depool_eqmask, otc.depool_eqmask], ids=['numpy', 'torch'])
def test_depool_bwd_against_autograd(shape, ties, depool):
    """g_up of sum(g_out * DePool2D(up)); with integer `pre` the windows have tied maxima, and each tied
    position hands its g_out on (the oracle's mask keeps every one of them)."""
    rng = np.random.default_rng(sum(shape) + ties)
    pre = rng.integers(0, 3, size=shape).astype(np.float64) if ties else rng.standard_normal(shape)
    pooled = onn.maxpool2(pre)
    gout = rng.standard_normal(shape)
    up = _t(rng.standard_normal(pooled.shape), grad=True)
    if depool is otc.depool_eqmask:
        out = depool(up, _t(pre), _t(pooled))
    else:
        # (the numpy oracle is linear in `up`: out = mask * repeat(up); its mask is read off with up = 1)
        mask = _t(depool(np.ones_like(pooled), pre, pooled))
        rep = up.repeat_interleave(2, 2).repeat_interleave(2, 3)
        out = F.pad(rep, (0, shape[3] - rep.shape[3], 0, shape[2] - rep.shape[2])) * mask
    (out * _t(gout)).sum().backward()
    assert np.abs(R.depool_bwd(gout, pre, pooled) - up.grad.numpy()).max() <= TOL
    if ties:
        assert ((_win(pre) == pooled[:, :, :, None, :, None]).sum(axis=(3, 5)) >= 2).any()


def _win(a):
    B, C, H, W = a.shape
    return a[:, :, :H // 2 * 2, :W // 2 * 2].reshape(B, C, H // 2, 2, W // 2, 2)


@pytest.mark.parametrize('shape', [(1, 1, 2, 2), (2, 3, 9, 7), (1, 2, 6, 11)])
def test_pool_relu_bwd_against_autograd_on_tie_free_data(shape):
    rng = np.random.default_rng(sum(shape))
    z = rng.standard_normal(shape)
    gpool = rng.standard_normal((shape[0], shape[1], shape[2] // 2, shape[3] // 2))
    zt = _t(z, grad=True)
    (F.max_pool2d(F.relu(zt), 2) * _t(gpool)).sum().backward()
    pre = np.maximum(z, 0)
    # (a window without a positive value is all zero after the ReLU: four tied zeros there, and autograd's
    # relu'(0) = 0 gives 0 whichever of them max_pool2d picks)
    got = R.pool_relu_bwd(gpool, pre, onn.maxpool2(pre))
    assert np.abs(got - zt.grad.numpy()).max() <= TOL
    assert not got[:, :, shape[2] // 2 * 2:].any() and not got[:, :, :, shape[3] // 2 * 2:].any()


def test_pool_relu_bwd_tie_and_zero_rules_by_hand():
    # 2 x 2: the two tied maxima both receive the gradient, the smaller values nothing
    pre = np.array([[[[3., 1.], [0., 3.]]]])
    got = R.pool_relu_bwd(np.array([[[[5.]]]]), pre, np.array([[[[3.]]]]))
    assert np.array_equal(got, [[[[5., 0.], [0., 5.]]]])
    # 2 x 2 all zero: every position equals the maximum, relu'(0) = 0 lets nothing through
    got = R.pool_relu_bwd(np.array([[[[5.]]]]), np.zeros((1, 1, 2, 2)), np.zeros((1, 1, 1, 1)))
    assert np.array_equal(got, np.zeros((1, 1, 2, 2)))
    # 3 x 3: one window; the odd last row and column belong to none, even where they hold the maximum's value
    pre = np.array([[[[2., 2., 2.], [0., 1., 9.], [2., 9., 2.]]]])
    got = R.pool_relu_bwd(np.array([[[[-4.]]]]), pre, onn.maxpool2(pre))
    assert np.array_equal(got, [[[[-4., -4., 0.], [0., 0., 0.], [0., 0., 0.]]]])


def test_depool_bwd_tie_rule_by_hand():
    pre = np.array([[[[3., 1., 7.], [0., 3., 7.], [3., 3., 3.]]]])
    gout = np.array([[[[1., 10., 100.], [1000., -4., 100.], [9., 9., 9.]]]])
    assert np.array_equal(R.depool_bwd(gout, pre, np.array([[[[3.]]]])), [[[[-3.]]]])
    # an all-zero window: all four tied, all four counted (no ReLU in this adjoint)
    assert np.array_equal(R.depool_bwd(gout[:, :, :2, :2], np.zeros((1, 1, 2, 2)), np.zeros((1, 1, 1, 1))),
                          [[[[1007.]]]])


def test_to_c8_bf16_layout():
    rng = np.random.default_rng(8)
    y = rng.random((2, 11, 3, 5)).astype(np.float32)
    m = R.to_c8_bf16(y)
    assert tuple(m.shape) == (2, 2, 3, 5, 8) and m.dtype == torch.bfloat16
    back = m.float().numpy().transpose(0, 1, 4, 2, 3).reshape(2, 16, 3, 5)
    assert np.array_equal(back[:, :11], torch.from_numpy(y).to(torch.bfloat16).float().numpy())
    assert not back[:, 11:].any()
    assert np.abs(back[:, :11] - y).max() <= 2.0 ** -9                   # bf16: 8 significant bits, y < 1
    m4 = R.to_c8_bf16(y, chunks=4)
    assert tuple(m4.shape) == (2, 4, 3, 5, 8) and torch.equal(m4[:, :2], m) and not m4[:, 2:].float().any()
