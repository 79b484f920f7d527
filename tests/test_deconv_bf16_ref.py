"""CPU: tests/deconv_bf16_ref.py, the float64 statement the deconv='bf16' kernels are checked against (DESIGN.md
section 23), equals the project's restatement of the transposed convolution's backward and is the adjoint of
oracle.nn's transposed convolution."""
import numpy as np
import pytest
import torch

import deconv_bf16_ref as D
import densenet_train_ref as R
from oracle import nn


def _windows(H, W):
    return [None, (0, 0, 2 * H, 2 * W), (1, 2, 2 * H - 1, 2 * W - 2), (3, 2, 3, 5)]


def _case(B, Cin, Cout, H, W, window, seed):
    rng = np.random.default_rng(seed)
    win = D.full_window(H, W) if window is None else window
    x = rng.standard_normal((B, Cin, H, W))
    Wt = rng.standard_normal((Cin, Cout, 3, 3))
    g = rng.standard_normal((B, Cout, win[2], win[3]))
    return x, g, Wt, win


CASES = [(2, 5, 3, 4, 6, w) for w in _windows(4, 6)] + [(1, 1, 1, 1, 1, None)]


@pytest.mark.parametrize('B,Cin,Cout,H,W,window', CASES)
def test_grads_equal_the_restatement(B, Cin, Cout, H, W, window):
    x, g, Wt, win = _case(B, Cin, Cout, H, W, window, 11)
    dW, gx, db = D.grads(x, g, Wt, window)
    gx_r, dW_r, db_r = R.deconv_bwd(x, Wt, g, 2, win)
    for got, want in ((dW, dW_r), (gx, gx_r), (db, db_r)):
        assert got.dtype == np.float64 and got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize('B,Cin,Cout,H,W,window', CASES)
def test_grads_are_the_adjoint_of_the_oracle_forward(B, Cin, Cout, H, W, window):
    x, g, Wt, win = _case(B, Cin, Cout, H, W, window, 12)
    dW, gx, db = D.grads(x, g, Wt, window)
    oy, ox, OH, OW = win
    crop = lambda full: full[:, :, oy:oy + OH, ox:ox + OW]
    bias = np.random.default_rng(13).standard_normal(Cout)
    out = crop(nn.deconv2d(x, Wt, np.zeros(Cout), stride=2))
    rhs = float((g * out).sum())
    assert abs(float((gx * x).sum()) - rhs) <= 1e-12 * np.abs(g * out).sum()       # <gx, x> = <g, window(deconv x)>
    assert abs(float((dW * Wt).sum()) - rhs) <= 1e-12 * np.abs(g * out).sum()      # linear in W too
    with_b = crop(nn.deconv2d(x, Wt, bias, stride=2))
    assert abs(float((g * (with_b - out)).sum()) - float(db @ bias)) <= 1e-12 * (np.abs(g).sum() * np.abs(bias).max())


def test_mags_bound_grads_and_rounded_is_bf16():
    x, g, Wt, win = _case(2, 5, 3, 4, 6, (1, 2, 7, 10), 14)
    got, mag = D.grads(x, g, Wt, win), D.mags(x, g, Wt, win)
    for a, m in zip(got, mag):
        assert (np.abs(a) <= m * (1 + 1e-12)).all() and (m >= 0).all()
    v = torch.tensor([1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8, -(1 + 2.0 ** -8 + 2.0 ** -10)], dtype=torch.float32)
    assert D.rounded(v).tolist() == [1.0, 1 + 2.0 ** -6, -(1 + 2.0 ** -7)]
    assert D.rounded(v.numpy()).dtype == np.float64
