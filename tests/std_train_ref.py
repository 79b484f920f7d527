"""Float64 (numpy) restatement of what training the standard DAE computes: forward (oracle/dae.py, imported),
the training losses (tests/ctx_train_ref.py, imported) and the backward pass with the weight gradients, by
hand-written reverse mode in the conventions of oracle/dae_grad.py: max-pool backward to EVERY position equal to
the window maximum, relu'(0) = 0, no gradient through the DePool2D mask.  conv_before_pool = 1, bn = 0,
unpool_type in {trackind, inverse}.  TEST INFRASTRUCTURE: pinned by central finite differences
(tests/test_std_train_ref.py); the HIP path is checked against it.  `backward` runs in the dtype of what it is
handed (float32 arrays give the numpy-float32 reference error of tests/test_gpu_std_train.py).
"""
import numpy as np

from ctx_train_ref import adam_step, loss_and_grad, rmsprop_step, to64   # noqa: F401 (re-exported)
from oracle import nn
from oracle.dae import _n_pool, dae_forward, param_order
from oracle.dae_grad import _center, _conv_bwd_data


def order_of(cfg):
    return param_order(cfg['concat_h'], 1, cfg['additional_pool'], cfg.get('unpool_type', 'trackind'), 0)


def forward(params, h_list, y, cfg):
    """The net dict of oracle.dae.dae_forward (score map under 'score'; 'input', 'pre%d', 'pool%d',
    'fused_up%d' are what `backward` reads)."""
    return dae_forward(params, h_list, y, out_softmax=False, return_net=True, **cfg)[1]


def wgrad(x, gz, pad):
    """dW[co, ci, ky, kx] = sum gz[b, co, y, x] xpad[b, ci, y + ky, x + kx]; db[co] = sum gz."""
    B, Ci, H, W = x.shape
    OH, OW = gz.shape[2:]
    xp = np.zeros((B, Ci, H + 2 * pad, W + 2 * pad), dtype=x.dtype)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    dW = np.zeros((gz.shape[1], Ci, 3, 3), dtype=x.dtype)
    for ky in range(3):
        for kx in range(3):
            dW[:, :, ky, kx] = np.tensordot(gz, xp[:, :, ky:ky + OH, kx:kx + OW], axes=([0, 2, 3], [0, 2, 3]))
    return dW, gz.sum(axis=(0, 2, 3))


def _eqmask(pre, pooled):
    h2, w2 = pooled.shape[2], pooled.shape[3]
    return pre[:, :, :2 * h2, :2 * w2] == np.repeat(np.repeat(pooled, 2, 2), 2, 3)


def backward(params, h_list, saved, g_score, cfg):
    """{name: (dW, db)} from the maps of a forward pass (`forward`, or another forward's: teacher forcing -- the
    decisions are [pre > 0] and [pre == its window's maximum] of whatever is handed in)."""
    concat_h = list(cfg['concat_h'])
    n_pool, total = _n_pool(concat_h, cfg['additional_pool'])
    skip, padding = cfg.get('skip', True), cfg.get('padding', 100)
    y = saved['input']
    hmap = dict(zip(concat_h, h_list))
    grads, g_pool = {}, {}
    g_f = g_score
    for p in range(1, total + 1):                                  # decoder, output to input
        pre, pooled = saved['pre%d' % p], saved['pool%d' % p]
        other = saved['pool%d' % (p - 1)] if p > 1 else y
        H, Wd = min(pre.shape[2], other.shape[2]), min(pre.shape[3], other.shape[3])
        W = params['up_conv%d' % p][0]
        g_c = np.zeros((pre.shape[0], W.shape[0]) + pre.shape[2:], dtype=g_f.dtype)
        cy, cx = _center(pre.shape[2], H), _center(pre.shape[3], Wd)
        g_c[:, :, cy:cy + H, cx:cx + Wd] = g_f
        if skip and p > 1:
            gp = g_pool.setdefault(p - 1, np.zeros_like(other))
            oy, ox = _center(other.shape[2], H), _center(other.shape[3], Wd)
            gp[:, :, oy:oy + H, ox:ox + Wd] += g_f
        t_in = pooled if p == total else saved['fused_up%d' % (p + 1)]
        grads['up_conv%d' % p] = wgrad(nn.depool_eqmask(t_in, pre, pooled), g_c, 1)
        g_u = _conv_bwd_data(g_c, W, 1, pre.shape[2:])
        h2, w2 = pooled.shape[2], pooled.shape[3]
        gm = np.where(_eqmask(pre, pooled), g_u[:, :, :2 * h2, :2 * w2], 0.0).astype(g_u.dtype)
        g_f = gm.reshape(gm.shape[0], gm.shape[1], h2, 2, w2, 2).sum(axis=(3, 5))
    g_pool[total] = g_pool.get(total, 0) + g_f
    for p in range(total, 0, -1):                                  # encoder, deep to shallow
        pre, pooled = saved['pre%d' % p], saved['pool%d' % p]
        gp = g_pool.get(p)
        if gp is None:
            gp = np.zeros_like(pooled)
        h2, w2 = pooled.shape[2], pooled.shape[3]
        g_a = np.zeros_like(pre)
        g_a[:, :, :2 * h2, :2 * w2] = np.where(_eqmask(pre, pooled), np.repeat(np.repeat(gp, 2, 2), 2, 3), 0.0)
        g_z = np.where(pre > 0, g_a, 0.0).astype(pre.dtype)       # relu'(0) = 0
        name = 'conv%d_1' % p
        pad = padding if (p == 1 and len(concat_h) == 1 and concat_h[-1] != 'input' and padding > 0) else 1
        x = saved['pool%d' % (p - 1)] if p > 1 else y
        at = 'input' if p == 1 else 'pool%d' % (p - 1)
        if at in hmap:                                             # h first (P13)
            x = nn.concat_h_first(hmap[at], x)
        grads[name] = wgrad(x, g_z, pad)
        if p > 1:
            W = params[name][0]
            g_x = _conv_bwd_data(g_z, W, pad, (g_z.shape[2] + 2 - 2 * pad, g_z.shape[3] + 2 - 2 * pad))
            if at in hmap:
                g_x = g_x[:, hmap[at].shape[1]:]
            g_pool[p - 1] = g_pool.get(p - 1, 0) + g_x
    return grads


def decisions(net, total):
    """The ReLU and max-pool decisions of a forward pass, as a list of boolean arrays."""
    out = []
    for p in range(1, total + 1):
        out += [net['pre%d' % p] > 0, _eqmask(net['pre%d' % p], net['pool%d' % p])]
    return out


def loss_of(params, h_list, y, T, cfg, losses=('crossentropy',), lmb=1.0):
    return loss_and_grad(forward(params, h_list, y, cfg)['score'], T, losses, lmb)[0]


def loss_and_param_grads(params, h_list, y, T, cfg, losses=('crossentropy',), lmb=1.0):
    net = forward(params, h_list, y, cfg)
    loss, _, _, g, _ = loss_and_grad(net['score'], T, losses, lmb)
    return loss, backward(params, h_list, net, g, cfg), net


def flatten(d, order):
    """`order`, W then b: the layout of StandardDAE.flat."""
    return np.concatenate([np.asarray(a).ravel() for n in order for a in d[n]])


def unflatten(flat, like, order):
    out, off = {}, 0
    for n in order:
        arrs = []
        for a in like[n]:
            arrs.append(flat[off:off + a.size].reshape(a.shape))
            off += a.size
        out[n] = tuple(arrs)
    return out


# the two models of the tests: (n_classes, h channels, y shape, cfg)
SMALL = (4, 3, (2, 4, 12, 10), dict(concat_h=['pool1'], padding=3, n_filters=4, additional_pool=1, skip=True))
SECOND = (11, 16, (2, 11, 40, 36), dict(concat_h=['pool2'], padding=100, n_filters=8, additional_pool=2, skip=True))


def make_case(model, seed=5):
    """(params float64, [h], y, T) of a model above: seeded synthetic weights, a noisy one-hot y, void pixels."""
    from iterative_inference_segm_amd import synthetic as S
    C, hc, (B, _, H, W), cfg = model
    rng = np.random.default_rng(seed)
    params = to64(S.make_dae_params(C, (hc,), concat_h=cfg['concat_h'], n_filters=cfg['n_filters'],
                                    additional_pool=cfg['additional_pool'], seed=100 + seed))
    T = S.make_labels(B, H, W, n_classes=C, void_frac=0.1, seed=seed + 1, block=4).astype(np.float64)
    y = np.clip(T[:, :C] + 0.1 * rng.standard_normal((B, C, H, W)), 0, 1)
    # h lives on the map behind its pool point
    n = int(cfg['concat_h'][0][-1])
    hh, hw = H + 2 * cfg['padding'] - 2, W + 2 * cfg['padding'] - 2
    for _ in range(n):
        hh, hw = hh // 2, hw // 2
    h = rng.standard_normal((B, hc, hh, hw))
    return params, [h], y, T
