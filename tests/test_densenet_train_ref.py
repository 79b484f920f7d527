"""CPU: the float64 restatement of FC-DenseNet's training backward (tests/densenet_train_ref.py) against central
finite differences of its own forward + loss, with the protocol of tests/test_fcn8_train_ref.py: per parameter array
the largest entry of the gradient, ten random entries and one random direction, eps 1e-6, with weight decay off and on
and with the dropout masks all-ones and drawn.  A probe whose +-eps forwards take another ReLU / max-pool decision
than the base point is skipped; at most 1 probe in 10 may be.

Case 'thin': layers [2, 3, 2, 3, 2], 2 pools, growth 4, 8 first filters, 4 classes + void, B = 2 on 3 x 13 x 18 -- odd
sizes: the first pool drops a row (13 -> 6), the second a column (9 -> 4), and the two TransitionUps crop 7 -> 6 rows
and 9 -> 9, 13 -> 13 and 19 -> 18.  Every BatchNorm input channel's batch variance is at least 0.05 (asserted), so
that inv_std <= 4.5 and the float64 bound of the GPU test means what it says.
"""
import numpy as np
import pytest

import densenet_train_ref as R

EPS = 1e-6
SEED = 3
CFG = R.THIN


def test_program_is_the_layer_plan():
    steps, caps = R.program(CFG)
    plan = R.plan_of(CFG)
    assert [e['kind'] for e in steps] == [k for k, _, _ in plan] and [e['li'] for e in steps] == list(range(len(plan)))
    for e, (kind, cin, cout) in zip(steps, plan):
        if kind in ('brc', 'td', 'softmax'):
            assert e['n'] == cin
        if kind == 'tu':
            assert e['n'] - e['block0'] == cin and e['keep'] == cout
    assert len(caps) == 2 * CFG['n_pool'] + 1
    assert R.n_keeps(CFG) == sum(CFG['nlpb']) + CFG['n_pool']


def test_forward_is_the_oracles_forward():
    """The restatement's deterministic forward is oracle/densenet.py's."""
    from oracle import nn
    from oracle.densenet import densenet_forward
    params, x, T, keeps = R.make_case(CFG, seed=SEED)
    s = R.forward(params, x, CFG)
    hidden, probs = densenet_forward(params, x, layer=('pool1',), n_layers_per_block=CFG['nlpb'], n_pool=CFG['n_pool'],
                                     growth=CFG['growth'])
    assert np.abs(nn.softmax_channels(s['score']) - probs).max() <= 1e-12
    assert np.abs(s['td_pooled'][0] - hidden).max() <= 1e-12
    assert s['stacks'][0].shape[2:] == (13, 18) and s['stacks'][1].shape[2:] == (6, 9) and s['stacks'][2].shape[2:] == (3, 4)
    assert sorted(s['win'].values()) == [(0, 0, 6, 9), (0, 0, 13, 18)]
    odd = np.random.default_rng(0).standard_normal((2, 3, 7, 9))
    assert np.array_equal(R.maxpool2(odd), nn.maxpool2(odd))


def test_batch_variances_are_bounded_below():
    params, x, T, keeps = R.make_case(CFG, seed=SEED)
    for k in (None, keeps):
        v = R.min_variance(R.forward(params, x, CFG, k), CFG)
        print('smallest batch variance over all BatchNorm inputs (%s): %.4g' % ('drawn masks' if k else 'no dropout', v))
        assert v >= 0.05


@pytest.mark.parametrize('weight_decay,masks', [(0.0, 'ones'), (1e-2, 'drawn')])
def test_restatement_matches_finite_differences(weight_decay, masks):
    params, x, T, keeps = R.make_case(CFG, seed=SEED)
    assert T[:, CFG['n_classes']].sum() > 0                      # void pixels present
    if masks == 'ones':
        keeps = [np.ones_like(k) for k in keeps]
    else:
        assert all(0 < k.sum() < k.size for k in keeps)
    loss, grads, s = R.loss_and_param_grads(params, x, T, CFG, keeps, weight_decay)
    base = R.decisions(s)
    flat, gflat = R.flatten(params), R.flatten(grads)
    assert flat.shape == gflat.shape
    rng = np.random.default_rng(17)
    probes, off = [], 0
    for li, f, a in R.arrays(params):
        idx = off + np.arange(a.size)
        assert np.abs(gflat[idx]).max() > 0, (li, f)             # every array alive
        picks = [idx[np.abs(gflat[idx]).argmax()]] + list(rng.choice(idx, size=min(10, a.size), replace=False))
        for i in picks:
            d = np.zeros_like(flat)
            d[i] = 1.0
            probes.append(((li, f), d))
        d = np.zeros_like(flat)
        d[idx] = rng.standard_normal(a.size)
        probes.append(((li, f), d / np.linalg.norm(d)))
        off += a.size
    skipped, worst = 0, 0.0
    for name, d in probes:
        vals, crossed = [], False
        for sgn in (1.0, -1.0):
            v, s2 = R.loss_of(R.unflatten(flat + sgn * EPS * d, params), x, T, CFG, keeps, weight_decay)
            crossed = crossed or any((a != b).any() for a, b in zip(base, R.decisions(s2)))
            vals.append(v)
        if crossed:
            skipped += 1
            continue
        fd, an = (vals[0] - vals[1]) / (2 * EPS), float(gflat @ d)
        err = abs(fd - an) / max(1.0, abs(an))
        worst = max(worst, err)
        assert err <= 1e-7, (name, fd, an)
    print('finite differences wd %g masks %s: %d probes, %d skipped, worst error %.3g'
          % (weight_decay, masks, len(probes), skipped, worst))
    assert skipped * 10 <= len(probes)


def test_the_one_array_without_a_gradient():
    """The first TransitionUp's bias: its output is read through BatchNorm with batch statistics only, which takes a
    per-channel constant out again.  The restatement's value there is the rounding of a sum that cancels."""
    params, x, T, keeps = R.make_case(CFG, seed=SEED)
    loss, grads, s = R.loss_and_param_grads(params, x, T, CFG, keeps)
    mags = {}
    R.backward(params, s, R.loss_and_grad(s['score'], T)[3], CFG, mags)
    dead = R.dead_arrays(CFG)
    assert dead == [(10, 'b')] and params[10]['kind'] == 'tu'
    for li, q in enumerate(grads):
        for f, a in q.items():
            if (li, f) in dead:
                assert np.abs(a).max() <= 1e-13 * mags[li].max()
            else:
                assert np.abs(a).max() > 1e-6 * max(np.abs(v).max() for v in q.values()), (li, f)
