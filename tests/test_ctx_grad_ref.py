"""CPU: tests/ctx_grad_ref.py -- the float64 restatement the true-gradient refinement of the context-module DAE
is checked against -- is pinned by central finite differences (the bound of tests/test_oracle_grad.py)."""
import numpy as np

import ctx_grad_ref as G
import ctx_train_ref as R
from iterative_inference_segm_amd import synthetic as S


def _pre_activations(params, h, y):
    """The pre-ReLU maps of the seven rectified layers (the forward of ctx_train_ref with relu off per layer)."""
    cat, outs = R.forward(params, h, y)
    H, W = y.shape[2:]
    pad32 = np.zeros(outs[0].shape[:2] + (H + 64, W + 64))
    pad32[:, :, 32:-32, 32:-32] = outs[0]
    ins = [cat, pad32] + outs[1:6]
    pre = [R._valid(cat, *params['conv1'], 1, False)]
    for i, d in enumerate(R.DILATIONS):
        Wd, bd = params['dilconv%d' % (i + 1)]
        pre.append(R._valid(ins[i + 1], np.transpose(Wd, (1, 0, 2, 3)), bd, d, False))
    return pre


def _case():
    # the seed is chosen HERE, on the CPU: the first one for which no ReLU input lies within 1e-5 of zero (a
    # central difference of 1e-6 must not cross a kink)
    B, C, Hh, Ww = 1, 11, 12, 10
    for seed in range(3, 40):
        rng = np.random.default_rng(seed)
        params = R.to64(S.make_contextmod_params(C, 3, seed=seed))
        h = rng.random((B, 3, Hh, Ww))
        y = rng.random((B, C, Hh, Ww))
        y /= y.sum(1, keepdims=True)
        if min(float(np.abs(p).min()) for p in _pre_activations(params, h, y)) > 1e-5:
            return seed, rng, params, h, y
    raise AssertionError('no seed keeps the ReLU inputs away from zero')


def test_sqerr_gradient_matches_central_differences():
    seed, rng, params, h, y = _case()
    g, r = G.ctx_sqerr_grad(params, h, y)
    assert g.shape == y.shape and r.shape == y.shape
    assert np.abs(g).max() > 1e-2                            # not a vanishing gradient
    assert np.allclose(r.sum(axis=1), 1.0)
    e = 1e-6

    def fd_entry(idx):
        yp, ym = y.copy(), y.copy()
        yp[idx] += e
        ym[idx] -= e
        return (G.sqerr(params, h, yp) - G.sqerr(params, h, ym)) / (2 * e)

    big = np.unravel_index(np.abs(g).argmax(), g.shape)
    for idx in [big] + [tuple(rng.integers(0, s) for s in y.shape) for _ in range(10)]:
        fd = fd_entry(idx)
        assert abs(fd - g[idx]) <= 1e-6 * (1 + abs(fd)), (seed, idx, fd, g[idx])
    # one random direction over the whole map
    v = rng.standard_normal(y.shape)
    v /= np.linalg.norm(v)
    fd = (G.sqerr(params, h, y + e * v) - G.sqerr(params, h, y - e * v)) / (2 * e)
    assert abs(fd - float((g * v).sum())) <= 1e-6 * (1 + abs(fd)), (seed, fd, float((g * v).sum()))


def test_pieces_compose_to_the_whole():
    """head + the chain from dilconv6 = backward_y of the softmax backward (what the HIP path fuses)."""
    _, _, params, h, y = _case()
    _, outs = R.forward(params, h, y)
    gs, r = G.softmax_sqerr_bwd(outs[-1], y)
    g6, gs2 = G.head(outs[-1], y, outs[6], params['dilconv7'][0])
    assert np.array_equal(gs, gs2)
    assert np.array_equal(g6, np.where(outs[6] > 0, R._bwd_data(gs, params['dilconv7'][0], 1), 0.0))
    whole, _ = G.ctx_sqerr_grad(params, h, y)
    assert np.array_equal(G.backward_y(params, outs, gs, 3) - 2.0 * (r - y), whole)
    # two steps of the loop lower the reconstruction error
    yy, last = G.refine_gradient(params, h, y, 0.05, 2)
    assert G.sqerr(params, h, yy) < G.sqerr(params, h, y) and last.shape == (1,)
