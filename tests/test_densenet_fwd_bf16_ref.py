"""CPU: tests/densenet_fwd_bf16_ref.py pinned -- without rounding it IS densenet_train_ref.forward; with rounding only
the 'brc' layers move; one layer equals the forward's own layer; and the bound discriminates: the sum over unrounded
operands lies far outside it."""
import numpy as np

import densenet_fwd_bf16_ref as F
import densenet_train_ref as RD
from kxk_bf16_ref import bf16


def _same(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


def test_unrounded_forward_is_the_training_reference():
    for cfg in (RD.THIN, RD.WIDE):
        params, x, T, keeps = RD.make_case(cfg)
        for kp in (None, keeps):
            a, b = F.forward(params, x, cfg, kp, 0.2, rounded=False), RD.forward(params, x, cfg, kp, 0.2)
            assert np.array_equal(a['score'], b['score'])
            for k in ('stacks', 'mean', 'inv_std', 'td_pre', 'td_pooled', 'gates'):
                _same(a[k], b[k])
            assert a['win'] == b['win']


def test_rounding_moves_the_dense_block_layers_and_nothing_before_them():
    cfg = RD.THIN
    params, x, T, keeps = RD.make_case(cfg)
    a, b = F.forward(params, x, cfg, keeps, 0.2, rounded=True), RD.forward(params, x, cfg, keeps, 0.2)
    n0 = cfg['n_first']
    assert np.array_equal(a['stacks'][0][:, :n0], b['stacks'][0][:, :n0])           # the first convolution
    assert not np.array_equal(a['stacks'][0][:, n0:], b['stacks'][0][:, n0:])
    d = np.abs(a['score'] - b['score']).max() / np.abs(b['score']).max()
    assert 0 < d < 0.05, d
    # the first 'brc' layer of the rounded pass is `layer` on the (shared) first stack
    e = [e for e in RD.program(cfg)[0] if e['kind'] == 'brc'][0]
    q = params[e['li']]
    t = F.bn_relu(b['stacks'][0][:, :n0], q['beta'], q['gamma'], b['mean'][0], b['inv_std'][0])
    z = F.layer(q['W'], q['b'], t, rounded=True) * keeps[e['ki']] / (1.0 - 0.2)
    g = cfg['growth']
    assert np.allclose(a['stacks'][0][:, n0:n0 + g], z, rtol=1e-12, atol=1e-12)


def test_layer_is_the_plain_statement_and_the_mask_factor_is_float32s():
    rng = np.random.default_rng(0)
    W, b, t = rng.standard_normal((3, 2, 3, 3)), rng.standard_normal(3), np.abs(rng.standard_normal((1, 2, 4, 5)))
    z = F.layer(W, b, t, rounded=False)
    tp = np.pad(t, ((0, 0), (0, 0), (1, 1), (1, 1)))
    ref = np.zeros((1, 3, 4, 5))
    for co in range(3):
        for i in range(4):
            for j in range(5):
                ref[0, co, i, j] = (W[co] * tp[0, :, i:i + 3, j:j + 3]).sum() + b[co]
    assert np.allclose(z, ref, rtol=1e-13, atol=1e-13)
    keep = (rng.random(z.shape) > 0.3).astype(np.float64)
    assert np.array_equal(F.layer(W, b, t, keep, 0.2, rounded=False), z * keep * F.scale_of(0.2))
    assert F.scale_of(0.5) == 2.0 and F.scale_of(0.3) == float(np.float32(1) / (np.float32(1) - np.float32(0.3)))
    assert F.scale_of(0.3) != 1.0 / 0.7                                   # (float32's quotient, not float64's)
    assert np.array_equal(F.layer(W, b, t), F.layer(bf16(W), b, bf16(t), rounded=False))
    assert np.array_equal(F.bn_relu(t, [0, 0], [1, 1], [0, 0], [1, 1]), t)


def test_bound_discriminates_on_17_to_16_channels():
    """The sum over unrounded operands lies outside the bound for more than 0.9 of the entries (seeded normal data,
    He-scaled W, 17 -> 16 channels at 7 x 9, B = 2), the sum over rounded ones inside by construction."""
    W, b, x, beta, gamma, mean, inv_std = F.rounding_case()
    assert x.shape == (2, 17, 7, 9) and W.shape == (16, 17, 3, 3)
    t = F.bn_relu(x, beta, gamma, mean, inv_std)
    zr, zu, bd = F.layer(W, b, t), F.layer(W, b, t, rounded=False), F.bound(W, b, t)
    assert bd.shape == zr.shape and (bd > 0).all()
    diff = np.abs(zu - zr)
    outside = float((diff > bd).mean())
    ratio = float(np.median(diff / bd))
    print('outside %.3f, median difference / bound %.1f' % (outside, ratio))
    assert outside > 0.9, outside
    assert ratio > 8, ratio
    # ... and an fp32 accumulation of the rounded operands stays inside it
    z32 = np.zeros(zr.shape, np.float32)
    tp = np.pad(bf16(t), ((0, 0), (0, 0), (1, 1), (1, 1))).astype(np.float32)
    Wr = bf16(W).astype(np.float32)
    for c in range(17):
        for ky in range(3):
            for kx in range(3):
                z32 += Wr[None, :, c, ky, kx, None, None] * tp[:, c, None, ky:ky + 7, kx:kx + 9]
    z32 += b.astype(np.float32)[None, :, None, None]
    assert (np.abs(z32.astype(np.float64) - zr) <= bd).all()


def test_one_minus_cosines_leaves_the_dead_arrays_out():
    cfg = RD.THIN
    params, x, T, keeps = RD.make_case(cfg)
    _, grads, _ = RD.loss_and_param_grads(params, x, T, cfg, keeps)
    d = F.one_minus_cosines(grads, grads, cfg)
    assert all(abs(v) < 1e-12 for v in d.values())
    assert not set(RD.dead_arrays(cfg)) & set(d) and len(d) == len(RD.arrays(grads)) - len(RD.dead_arrays(cfg))
