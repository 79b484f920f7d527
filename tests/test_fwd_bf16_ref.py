"""CPU: tests/fwd_bf16_ref.py -- with rounding off it IS tests/fcn8_train_ref.forward; its bf16 helper is torch's
round-to-nearest-even, ties included; and the precondition of the GPU rounding test (tests/test_gpu_fwd_bf16.py):
on those very arrays the float64 sum over the UNROUNDED operands leaves the bound on at least half of the entries,
while the restatement, computed a second way, stays inside on all of them."""
import numpy as np
import pytest
import torch

import fcn8_train_ref as RF
import fwd_bf16_ref as F

_CASE = {}


def _case():
    if not _CASE:
        params, x, T, k6, k7 = RF.make_case(2, 26, 30, seed=5)
        _CASE.update(params=params, x=x, k6=k6, k7=k7, base=RF.forward(params, x, k6, k7),
                     on=F.forward(params, x, k6, k7, rounded=True))
    return _CASE


def test_with_rounding_off_it_is_the_restatement_exactly():
    c = _case()
    off = F.forward(c['params'], c['x'], c['k6'], c['k7'])
    assert sorted(off) == sorted(c['base'])
    for k, v in c['base'].items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(off[k], v), k
    # the swapped function has been put back
    again = RF.forward(c['params'], c['x'], c['k6'], c['k7'])
    assert all(np.array_equal(again[k], v) for k, v in c['base'].items() if isinstance(v, np.ndarray))


def test_with_rounding_on_the_fifteen_layers_move_and_each_is_the_single_layer_statement():
    c = _case()
    inputs = {n: 'in_' + n for n in F.LAYERS}
    inputs['fc7'] = 'drop6'
    for n in F.LAYERS:
        assert not np.array_equal(c['on'][n], c['base'][n]), n
        W, b = c['params'][n]
        assert np.array_equal(F.layer(W, b, c['on'][inputs[n]], F.pad_of(n)), c['on'][n]), n
    assert np.array_equal(c['on']['pool5'], RF.maxpool2(c['on']['conv5_3']))


def test_the_bf16_helper_is_torchs_nearest_even_ties_included():
    rng = np.random.default_rng(0)
    vals = np.concatenate([F.TIES.astype(np.float64), rng.standard_normal(4096), [0.0, -0.0, 2.0 ** -130, 65504.0]])
    vals = vals.astype(np.float32)
    want = torch.from_numpy(vals).to(torch.bfloat16).to(torch.float64).numpy()
    assert np.array_equal(F.bf16(vals), want) and F.bf16(vals).dtype == np.float64
    t = F.TIES.astype(np.float64)
    assert F.bf16(t).tolist() == [1.0, 1 + 2.0 ** -6, -1.0, -(1 + 2.0 ** -6), 1 + 2.0 ** -7, 1.0, -(1 + 2.0 ** -6),
                                  3.0]
    # every one of them is a value bf16 does not hold
    assert not (F.bf16(t) == t).any()


def _slow_sum(W, b, x, pad):
    """The sum over rounded operands a second way: tap by tap with einsum, not the oracle's C kernel."""
    W, x = F.bf16(W), F.bf16(x)
    if pad:
        x = np.pad(x, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    K = W.shape[2]
    OH, OW = x.shape[2] - K + 1, x.shape[3] - K + 1
    out = np.zeros((x.shape[0], W.shape[0], OH, OW))
    for ky in range(K):
        for kx in range(K):
            out += np.einsum('oi,bihw->bohw', W[:, :, ky, kx], x[:, :, ky:ky + OH, kx:kx + OW])
    return out + b[None, :, None, None]


@pytest.mark.parametrize('name', sorted(F.ROUNDING_CASES))
def test_precondition_of_the_rounding_test(name):
    W, b, x, pad = F.rounding_case(name)
    assert np.array_equal(W, W.astype(np.float32)) and np.array_equal(x, x.astype(np.float32))
    ref = F.layer(W, b, x, pad, relu=False)
    bnd = F.bound(W, b, x, pad)
    plain = F.layer(W, b, x, pad, relu=False, rounded=False)
    out = float((np.abs(plain - ref) > bnd).mean())
    print('%s: the unrounded sum leaves the bound on %.3f of the entries' % (name, out))
    assert out >= 0.5
    assert (np.abs(_slow_sum(W, b, x, pad) - ref) <= bnd).all()
