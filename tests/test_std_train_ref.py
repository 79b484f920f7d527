"""CPU: the float64 restatement of the standard DAE's training backward (tests/std_train_ref.py) against central
finite differences of its own forward + loss: per parameter array the largest entry of the gradient, ten random
entries and one random direction, for both losses and their sum.  A probe whose +-eps forwards take another ReLU /
max-pool decision than the base point is skipped; at most 1 probe in 10 may be.

The first layer's bias is made non-positive here.  With a positive bias the zero-padding border of that layer
rests at relu(b) > 0, whole pooling windows tie at that value, and the convention (gradient to EVERY position equal
to the window maximum) counts each tied position: by design that is not the derivative there, so finite
differences cannot pin it.  At zero the tie carries no gradient under either reading (relu'(0) = 0)."""
import numpy as np
import pytest

import std_train_ref as R

EPS = 1e-6
SEED = 5


@pytest.mark.parametrize('losses', [('crossentropy',), ('squared_error',), ('crossentropy', 'squared_error')])
def test_restatement_matches_finite_differences(losses):
    C, hc, yshape, cfg = R.SMALL
    params, hs, y, T = R.make_case(R.SMALL, seed=SEED)
    assert T[:, C].sum() > 0                                     # void pixels present
    params['conv1_1'] = (params['conv1_1'][0], -np.abs(params['conv1_1'][1]))
    order = R.order_of(cfg)
    total = len(order) // 2
    loss, grads, net = R.loss_and_param_grads(params, hs, y, T, cfg, losses, 0.7)
    base = R.decisions(net, total)
    flat, gflat = R.flatten(params, order), R.flatten(grads, order)
    rng = np.random.default_rng(17)
    probes, off = [], 0
    for n in order:
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
            p = R.unflatten(flat + s * EPS * d, params, order)
            net_s = R.forward(p, hs, y, cfg)
            crossed = crossed or any((a != b).any() for a, b in zip(base, R.decisions(net_s, total)))
            vals.append(R.loss_and_grad(net_s['score'], T, losses, 0.7)[0])
        if crossed:
            skipped += 1
            continue
        fd, an = (vals[0] - vals[1]) / (2 * EPS), float(gflat @ d)
        err = abs(fd - an) / max(1.0, abs(an))
        worst = max(worst, err)
        assert err <= 1e-7, (n, fd, an)
    print('finite differences %s: %d probes, %d skipped, worst error %.3g' % (losses, len(probes), skipped, worst))
    assert skipped * 10 <= len(probes)
    assert np.abs(gflat).max() > 0
