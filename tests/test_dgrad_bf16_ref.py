"""CPU: tests/dgrad_bf16_ref.py -- with rounding off it IS the two existing restatements; with rounding on, the
arrays no rounded data gradient reaches do not move and the others do."""
import numpy as np
import pytest

import dgrad_bf16_ref as D
import fcn8_train_ref as RF
import std_train_ref as R

MODELS = {'small': R.SMALL, 'second': R.SECOND}
FCN8_3X3 = [n for names in RF.BLOCKS for n in names]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_rounding_is_to_nearest_even_through_float32():
    vals = np.array([1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -10, -(1 + 2.0 ** -8 + 2.0 ** -10),
                     1 + 2.0 ** -7 - 2.0 ** -10, 0.0, -2.0])
    want = [1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, -(1 + 2.0 ** -7), 1 + 2.0 ** -7, 0.0, -2.0]
    assert D.bf16(vals).tolist() == want and D.bf16(vals).dtype == np.float64


@pytest.mark.parametrize('which', ['small', 'second'])
def test_standard_dae_chain(which):
    cfg = MODELS[which][3]
    params, hs, y, T = R.make_case(MODELS[which])
    net = R.forward(params, hs, y, cfg)
    _, _, _, g, _ = R.loss_and_grad(net['score'], T, ('crossentropy',), 1.0)
    base = R.backward(params, hs, net, g, cfg)
    off, on = D.std_backward(params, hs, net, g, cfg), D.std_backward(params, hs, net, g, cfg, rounded=True)
    assert sorted(off) == sorted(base) and all(_same(off[n], base[n]) for n in base)
    assert R._conv_bwd_data is __import__('oracle.dae_grad', fromlist=['x'])._conv_bwd_data     # put back
    assert _same(on['up_conv1'], base['up_conv1'])               # before the first data gradient
    moved = [n for n in base if not _same(on[n], base[n])]
    assert sorted(moved) == sorted(n for n in base if n != 'up_conv1'), moved
    cos = D.cosines(on, base)
    print('standard DAE (%s), float64 chain with rounded data gradients: 1 - cosine per layer %s'
          % (which, {n: '%.3g' % (1 - c) for n, c in cos.items()}))
    assert min(cos.values()) > 0.99


def test_fcn8_chain():
    params, x, T, k6, k7 = RF.make_case(3, 26, 30, seed=5)
    s = RF.forward(params, x, k6, k7)
    _, _, _, g, _ = RF.loss_and_grad(s['score'], T)
    base = RF.backward(params, s, g)
    off, on = D.fcn8_backward(params, s, g), D.fcn8_backward(params, s, g, rounded=True)
    assert all(_same(off[n], base[n]) for n in base)
    stay = [n for n in base if n not in FCN8_3X3] + ['conv5_3']
    assert len(stay) == 9
    for n in stay:
        assert _same(on[n], base[n]), n
    assert any(not _same(on[n], base[n]) for n in FCN8_3X3)
    cos = D.cosines(on, base)
    print('FCN-8, float64 chain with rounded data gradients: 1 - cosine per layer %s'
          % {n: '%.3g' % (1 - c) for n, c in cos.items() if n in FCN8_3X3})
    assert all(np.isfinite(c) for c in cos.values())
