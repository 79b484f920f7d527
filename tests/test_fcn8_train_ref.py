"""CPU: the float64 restatement of FCN-8's training backward (tests/fcn8_train_ref.py) against central finite
differences of its own forward + loss (the protocol of tests/test_std_train_ref.py): per
parameter array the largest entry of the gradient, ten random entries and one random direction, with weight decay
off and on and with the dropout masks all-ones and drawn.  A probe whose +-eps forwards take another ReLU /
max-pool decision than the base point is skipped; at most 1 probe in 10 may be.

The small net (width_div 16, fc 32, 4 classes) at B = 2, pad 100, input 26 x 30: the smallest input at which fc6
is valid (pool5 is 7 x 7).  conv1_1's bias is made non-positive: with a positive bias the pad-100 border rests at
relu(b) > 0, whole pooling windows tie at that value, and the convention (gradient to EVERY position equal to the
window maximum) counts each tied position, which is by design not the derivative there.  FCN-8 has two or three
convolutions in front of each pool and the border is most of every map at this input size, so the same holds for
the other twelve block convolutions: behind a dead conv1_1 border, conv1_2's border rests at relu(b_1_2), pool1's
windows tie there, and so on down to pool4 (measured: with only conv1_1's bias non-positive every array of blocks
1 to 4 misses finite differences by factors of 2 to 100, block 5 and everything behind it agree to 1e-9).  So the
case makes all thirteen biases non-positive (make_case(dead_border=True)): the border is zero on every map, its
ties carry no gradient under either reading (relu'(0) = 0), and the image's cone keeps every layer alive.  The GPU
tests keep the positive biases: there the tie convention is what is compared.
"""
import numpy as np
import pytest

import fcn8_train_ref as R

EPS = 1e-6
SEED = 5


@pytest.mark.parametrize('weight_decay,masks', [(0.0, 'ones'), (1e-2, 'drawn')])
def test_restatement_matches_finite_differences(weight_decay, masks):
    params, x, T, keep6, keep7 = R.make_case(2, 26, 30, seed=SEED, dead_border=True)
    C = R.SMALL['n_classes']
    assert T[:, C].sum() > 0                                     # void pixels present
    assert R.fc6_hw(26, 30) == (1, 1)
    if masks == 'ones':
        keep6, keep7 = np.ones_like(keep6), np.ones_like(keep7)
    else:
        assert 0 < keep6.sum() < keep6.size and 0 < keep7.sum() < keep7.size
    loss, grads, net = R.loss_and_param_grads(params, x, T, keep6, keep7, weight_decay)
    assert sorted(grads) == sorted(R.PARAM_ORDER) and len(grads) == 21
    base = R.decisions(net)
    flat, gflat = R.flatten(params), R.flatten(grads)
    rng = np.random.default_rng(17)
    probes, off = [], 0
    for n in R.PARAM_ORDER:
        for a in params[n]:
            idx = off + np.arange(a.size)
            picks = [idx[np.abs(gflat[idx]).argmax()]] + list(rng.choice(idx, size=min(10, a.size), replace=False))
            for i in picks:
                d = np.zeros_like(flat)
                d[i] = 1.0
                probes.append((n, d))
            d = np.zeros_like(flat)
            d[idx] = rng.standard_normal(a.size)
            probes.append((n, d / np.linalg.norm(d)))
            off += a.size
    skipped, worst = 0, 0.0
    for n, d in probes:
        vals, crossed = [], False
        for s in (1.0, -1.0):
            p = R.unflatten(flat + s * EPS * d, params)
            v, net_s = R.loss_of(p, x, T, keep6, keep7, weight_decay, reuse=net, first=n)
            crossed = crossed or any((a != b).any() for a, b in zip(base, R.decisions(net_s)))
            vals.append(v)
        if crossed:
            skipped += 1
            continue
        fd, an = (vals[0] - vals[1]) / (2 * EPS), float(gflat @ d)
        err = abs(fd - an) / max(1.0, abs(an))
        worst = max(worst, err)
        assert err <= 1e-7, (n, fd, an)
    print('finite differences wd %g masks %s: %d probes, %d skipped, worst error %.3g'
          % (weight_decay, masks, len(probes), skipped, worst))
    assert skipped * 10 <= len(probes)
    assert np.abs(gflat).max() > 0


def test_reused_forward_is_the_full_forward():
    """The probes recompute only from the perturbed layer on: the same maps as a forward from the input."""
    params, x, T, keep6, keep7 = R.make_case(2, 26, 30, seed=SEED, dead_border=True)
    net = R.forward(params, x, keep6, keep7)
    p2 = dict(params)
    p2['conv4_2'] = (params['conv4_2'][0] * 1.01, params['conv4_2'][1])
    full = R.forward(p2, x, keep6, keep7)
    part = R.forward(p2, x, keep6, keep7, reuse=net, first='conv4_2')
    assert (full['score'] == part['score']).all() and not (full['score'] == net['score']).all()


def test_forward_is_the_oracles_forward():
    """The restatement's deterministic forward is oracle/fcn8.py's, bit for bit (its own max-pool included)."""
    from oracle import nn
    from oracle.fcn8 import fcn8_forward
    params, x, T, keep6, keep7 = R.make_case(2, 26, 30, seed=SEED)
    net = R.forward(params, x)
    score, pool3 = fcn8_forward(params, x, layer=('score', 'pool3'))
    assert np.array_equal(net['score'], score) and np.array_equal(net['pool3'], pool3)
    odd = np.random.default_rng(0).standard_normal((2, 3, 7, 9))
    assert np.array_equal(R.maxpool2(odd), nn.maxpool2(odd))
