"""CPU: tests/kxk_bf16_ref.py -- with rounding off it IS tests/fcn8_train_ref.backward; with rounding on, the arrays
no rounded operand reaches do not move, and the others move by something of bf16's size."""
import numpy as np

import fcn8_train_ref as RF
import kxk_bf16_ref as K

FCN8_3X3 = [n for names in RF.BLOCKS for n in names]
STAY = ['upsample', 'score4', 'score_pool3', 'score2', 'score_pool4', 'score_fr']
_CASE = {}


def _case():
    if not _CASE:
        params, x, T, k6, k7 = RF.make_case(3, 26, 30, seed=5)
        s = RF.forward(params, x, k6, k7)
        _, _, _, g, _ = RF.loss_and_grad(s['score'], T)
        _CASE.update(params=params, s=s, g=g, base=RF.backward(params, s, g),
                     on=K.fcn8_backward(params, s, g, rounded=True))
    return _CASE


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_rounding_is_to_nearest_even_through_float32():
    vals = np.array([1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -10, -(1 + 2.0 ** -8 + 2.0 ** -10),
                     1 + 2.0 ** -7 - 2.0 ** -10, 0.0, -2.0])
    want = [1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, -(1 + 2.0 ** -7), 1 + 2.0 ** -7, 0.0, -2.0]
    assert K.bf16(vals).tolist() == want and K.bf16(vals).dtype == np.float64


def test_the_plain_statements_are_the_restatements_own():
    rng = np.random.default_rng(3)
    x, gz = rng.standard_normal((2, 5, 9, 8)), rng.standard_normal((2, 4, 3, 2))
    W = rng.standard_normal((4, 5, 7, 7))
    assert np.abs(K.wgrad_kxk(x, gz) - RF.wgrad(x, gz, 7)[0]).max() <= 1e-12
    assert np.abs(K.dgrad_kxk(gz, W) - RF.conv_bwd_data(gz, W, 0, (9, 8))).max() <= 1e-12
    x1, W1 = rng.standard_normal((2, 5, 3, 2)), rng.standard_normal((4, 5, 1, 1))
    assert np.abs(K.wgrad_kxk(x1, gz) - RF.wgrad(x1, gz, 1)[0]).max() <= 1e-12
    assert np.abs(K.dgrad_kxk(gz, W1) - RF.conv_bwd_data(gz, W1, 0, (3, 2))).max() <= 1e-12


def test_with_rounding_off_it_is_the_restatement():
    c = _case()
    off = K.fcn8_backward(c['params'], c['s'], c['g'])
    assert sorted(off) == sorted(c['base'])
    for n in c['base']:
        for a, b in zip(off[n], c['base'][n]):
            assert np.abs(a - b).max() <= 1e-12, n
    # the swapped functions have been put back
    on_again = K.fcn8_backward(c['params'], c['s'], c['g'], rounded=True)
    assert all(_same(on_again[n], c['on'][n]) for n in c['on'])
    assert all(_same(RF.backward(c['params'], c['s'], c['g'])[n], c['base'][n]) for n in c['base'])


def test_with_rounding_on_only_what_fc6_and_fc7_reach_moves():
    c = _case()
    base, on = c['base'], c['on']
    for n in STAY:
        assert _same(on[n], base[n]), n
    # fc7's g_z comes from score_fr's fp32 data gradient: db keeps its bits, dW does not
    assert np.array_equal(on['fc7'][1], base['fc7'][1]) and not np.array_equal(on['fc7'][0], base['fc7'][0])
    assert not np.array_equal(on['fc6'][0], base['fc6'][0])
    for n in FCN8_3X3:                                           # downstream of fc6's rounded data gradient
        assert not _same(on[n], base[n]), n


def test_the_move_is_of_bf16s_size():
    """1 - cosine of a gradient whose operands carry independent relative errors of at most 2^-9 each is about half
    the mean squared relative error of a product: between (2^-9)^2 / 100 and (2 * 2^-8)^2 / 2 for every array -- two
    orders below the worst case on one side, the worst case of two operands rounded twice over on the other.  The
    values of this case (printed) lie between 8.4e-8 (conv1_2) and 6.1e-6 (conv5_2, fc6)."""
    c = _case()
    cos = K.cosines({n: c['on'][n] for n in ['fc6', 'fc7'] + FCN8_3X3}, {n: c['base'][n] for n in ['fc6', 'fc7'] + FCN8_3X3})
    print('FCN-8, float64 chain with fc6 / fc7 rounded: 1 - cosine per array %s' % {n: '%.3g' % (1 - v) for n, v in cos.items()})
    lo, hi = (2.0 ** -9) ** 2 / 100, (2 * 2.0 ** -8) ** 2 / 2
    for n, v in cos.items():
        assert lo <= 1 - v <= hi, (n, 1 - v, lo, hi)
