"""CPU: tests/std_fwd_bf16_ref.py -- with rounding off it IS tests/std_train_ref (loss and gradients to 1e-12 on both
models); with rounding on every layer is the single-layer statement on the maps of that same forward and the backward
is the unrounded one on those maps; its bf16 helper rounds to nearest, ties to even, in both directions."""
import numpy as np
import pytest
import torch

import std_fwd_bf16_ref as F
import std_train_ref as R
from fwd_bf16_ref import TIES

MODELS = {'small': R.SMALL, 'second': R.SECOND}
_CASES = {}


def _case(which):
    if which not in _CASES:
        params, hs, y, T = R.make_case(MODELS[which])
        cfg = MODELS[which][3]
        _CASES[which] = dict(params=params, hs=hs, y=y, T=T, cfg=cfg,
                             base=R.loss_and_param_grads(params, hs, y, T, cfg),
                             on=F.loss_and_param_grads(params, hs, y, T, cfg, rounded=True))
    return _CASES[which]


@pytest.mark.parametrize('which', list(MODELS))
def test_with_rounding_off_it_is_the_restatement(which):
    c = _case(which)
    loss, grads, net = F.loss_and_param_grads(c['params'], c['hs'], c['y'], c['T'], c['cfg'])
    loss0, grads0, net0 = c['base']
    assert abs(loss - loss0) <= 1e-12 * abs(loss0)
    assert sorted(grads) == sorted(grads0) == sorted(R.order_of(c['cfg']))
    for n in grads0:
        for a, b in zip(grads[n], grads0[n]):
            assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), n
    assert np.array_equal(net['score'], net0['score'])
    # the swapped function has been put back
    from oracle import nn
    assert nn.conv2d.__module__ == 'oracle.nn'
    assert np.array_equal(R.forward(c['params'], c['hs'], c['y'], c['cfg'])['score'], net0['score'])


@pytest.mark.parametrize('which', list(MODELS))
def test_with_rounding_on_every_layer_moves_and_is_the_single_layer_statement(which):
    c = _case(which)
    loss, grads, net = c['on']
    base = c['base'][2]
    calls = F.layer_calls(net, c['hs'], c['cfg'])
    assert sorted(calls) == sorted(R.order_of(c['cfg']))
    for n, (x, pad, relu, other, out) in calls.items():
        W, b = c['params'][n]
        assert np.array_equal(F.layer(W, b, x, pad, relu, other), net[out]), n
        assert not np.array_equal(net[out], base[out]), n
        assert F.bound(W, b, x, pad, other).shape == net[out].shape and (F.bound(W, b, x, pad, other) >= 0).all()
    # nothing else is rounded: the pools, and the backward on these maps with the parameters as they are
    total = len(calls) // 2
    from oracle import nn
    for p in range(1, total + 1):
        assert np.array_equal(net['pool%d' % p], nn.maxpool2(net['pre%d' % p]))
    g = R.loss_and_grad(net['score'], c['T'], ('crossentropy',), 1.0)[3]
    again = R.backward(c['params'], c['hs'], net, g, c['cfg'])
    assert all(np.array_equal(a, b) for n in grads for a, b in zip(grads[n], again[n]))
    cos = F.cosines(grads, c['base'][1])
    print('%s: 1 - cosine of the rounded forward\'s gradients to the unrounded: %s'
          % (which, {n: '%.3g' % (1 - v) for n, v in cos.items()}))
    assert min(cos.values()) > 0.9 and loss != c['base'][0]


def test_the_rounding_helper_on_ties_in_both_directions():
    t = TIES.astype(np.float64)
    # exactly between two bf16 neighbours: down to the even one, up to the even one, both signs; just off a tie: to
    # the nearer neighbour on either side
    assert F.bf16(t).tolist() == [1.0, 1 + 2.0 ** -6, -1.0, -(1 + 2.0 ** -6), 1 + 2.0 ** -7, 1.0, -(1 + 2.0 ** -6),
                                  3.0]
    assert not (F.bf16(t) == t).any()
    rng = np.random.default_rng(0)
    vals = np.concatenate([t, rng.standard_normal(4096), [0.0, -0.0, 2.0 ** -130, 65504.0]]).astype(np.float32)
    want = torch.from_numpy(vals).to(torch.bfloat16).to(torch.float64).numpy()
    assert np.array_equal(F.bf16(vals), want) and F.bf16(vals).dtype == np.float64
    # values bf16 holds pass unchanged
    held = np.array([1.0, -1.5, 2.0 ** -6, 3.0, -2.0, 0.0])
    assert np.array_equal(F.bf16(held), held)
