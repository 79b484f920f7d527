"""Float64 (numpy) restatement of what training FCN-8 computes (reference train_fcn8.py:108-127): the forward of
oracle/fcn8.py / oracle/nn.py with the two dropout masks (DropoutLayer p, rescale=True, behind fc6 and fc7), the
masked cross-entropy of tests/ctx_train_ref.py (imported), + weight_decay * sum W^2 over the weight arrays
(regularize_network_params(l2): never the biases), and the backward pass with all 21 (dW, db) by hand-written
reverse mode in the project's conventions: max-pool gradient to EVERY position equal to the window maximum,
relu'(0) = 0.  pool4 and pool3 receive two gradients: the main path's first, then the side branch's (score_pool4 /
score_pool3), placed at the centre window's offset.  TEST INFRASTRUCTURE: pinned by central finite differences
(tests/test_fcn8_train_ref.py); the HIP path is checked against it.  `backward` runs in the dtype of what it is
handed (float32 arrays give the numpy-float32 reference error of tests/test_gpu_fcn8_train.py).
"""
import numpy as np

from ctx_train_ref import adam_step, loss_and_grad, to64   # noqa: F401 (re-exported)
from oracle import nn
from oracle.fcn8 import PARAM_ORDER

BLOCKS = [('conv1_1', 'conv1_2'), ('conv2_1', 'conv2_2'), ('conv3_1', 'conv3_2', 'conv3_3'),
          ('conv4_1', 'conv4_2', 'conv4_3'), ('conv5_1', 'conv5_2', 'conv5_3')]
STRIDES = {'score2': 2, 'score4': 2, 'upsample': 8}


def _center(big, small):
    return (big - small) // 2


def maxpool2(x):
    """oracle.nn.maxpool2 (2x2, stride 2, floor) as the maximum of its four strided slices: the same values, several
    times faster on the wide maps the finite-difference probes walk hundreds of times."""
    h, w = x.shape[2] // 2, x.shape[3] // 2
    v = x[:, :, :2 * h, :2 * w]
    return np.maximum(np.maximum(v[:, :, 0::2, 0::2], v[:, :, 0::2, 1::2]),
                      np.maximum(v[:, :, 1::2, 0::2], v[:, :, 1::2, 1::2]))


def _conv(params, name, t, pad):
    W, b = params[name]
    return nn.conv2d(t, np.ascontiguousarray(W), b, pad=pad, relu=True)


def forward(params, x, keep6=None, keep7=None, p=0.5, pad=100, reuse=None, first=None):
    """Every map `backward` reads, by name: 'in_<conv>' / '<conv>' the input and rectified output of a
    convolution, 'pool%d', 'drop6' / 'drop7', the inputs 'score_fr' / 'fused' / 'final' of the transposed
    convolutions, 'score'.  keep6 / keep7: 0/1 masks (None: the deterministic pass).  reuse / first: the maps of
    an earlier call whose parameters differ only from layer `first` of PARAM_ORDER on -- the layers before it are
    taken from `reuse` (what the finite-difference probes use)."""
    s = {'input': x, 'keep6': keep6, 'keep7': keep7, 'p': p, 'pad': pad}
    k0 = PARAM_ORDER.index(first) if reuse is not None else 0

    def layer(name, fn):
        if PARAM_ORDER.index(name) < k0:
            return reuse[name]
        return fn()

    t = x
    for bi, names in enumerate(BLOCKS):
        for ni, name in enumerate(names):
            s['in_' + name] = t
            t = s[name] = layer(name, lambda: _conv(params, name, t, pad if (bi == 0 and ni == 0) else 1))
        t = s['pool%d' % (bi + 1)] = maxpool2(t)
    s['in_fc6'] = t
    t = s['fc6'] = layer('fc6', lambda: _conv(params, 'fc6', t, 0))
    if keep6 is not None:
        t = t * keep6 / (1.0 - p)
    s['drop6'] = t
    t = s['fc7'] = layer('fc7', lambda: _conv(params, 'fc7', t, 0))
    if keep7 is not None:
        t = t * keep7 / (1.0 - p)
    s['drop7'] = t
    t = s['score_fr'] = layer('score_fr', lambda: _conv(params, 'score_fr', t, 0))
    for dec, side, pool, out in (('score2', 'score_pool4', 'pool4', 'fused'), ('score4', 'score_pool3', 'pool3', 'final')):
        W, b = params[dec]
        up = nn.deconv2d(t, W, b, stride=2)
        pm = s[pool]
        H, Wd = min(up.shape[2], pm.shape[2]), min(up.shape[3], pm.shape[3])
        oy, ox = _center(pm.shape[2], H), _center(pm.shape[3], Wd)
        s['win_' + side] = (oy, ox, H, Wd)
        s['in_' + side] = win = np.ascontiguousarray(pm[:, :, oy:oy + H, ox:ox + Wd])
        sp = s[side] = _conv(params, side, win, 0)                 # 1x1: the crop commutes with it
        s['win_' + dec] = (_center(up.shape[2], H), _center(up.shape[3], Wd), H, Wd)
        t = s[out] = nn.center_crop(up, H, Wd) + sp
    W, b = params['upsample']
    up = nn.deconv2d(t, W, b, stride=8)
    H, Wd = min(up.shape[2], x.shape[2]), min(up.shape[3], x.shape[3])
    s['win_upsample'] = (_center(up.shape[2], H), _center(up.shape[3], Wd), H, Wd)
    s['score'] = np.ascontiguousarray(nn.center_crop(up, H, Wd))
    return s


def wgrad(x, gz, K, pad=0):
    """dW[co, ci, ky, kx] = sum gz[b, co, y, x] xpad[b, ci, y + ky, x + kx]; db[co] = sum gz."""
    B, Ci, H, W = x.shape
    OH, OW = gz.shape[2:]
    xp = x
    if pad:
        xp = np.zeros((B, Ci, H + 2 * pad, W + 2 * pad), dtype=x.dtype)
        xp[:, :, pad:pad + H, pad:pad + W] = x
    dW = np.zeros((gz.shape[1], Ci, K, K), dtype=x.dtype)
    for ky in range(K):
        for kx in range(K):
            dW[:, :, ky, kx] = np.tensordot(gz, xp[:, :, ky:ky + OH, kx:kx + OW], axes=([0, 2, 3], [0, 2, 3]))
    return dW, gz.sum(axis=(0, 2, 3))


def conv_bwd_data(gz, W, pad, in_hw):
    """Adjoint of nn.conv2d(x, W, pad=pad) w.r.t. x: 'full' correlation of gz with the flipped, channel-transposed
    filter, cropped at offset pad."""
    K = W.shape[2]
    Wt = np.ascontiguousarray(np.transpose(W, (1, 0, 2, 3))[:, :, ::-1, ::-1]).astype(gz.dtype)
    full = nn.conv2d(gz, Wt, None, pad=K - 1)
    return full[:, :, pad:pad + in_hw[0], pad:pad + in_hw[1]]


def deconv_bwd(x, W, g, stride, window):
    """(g_x, dW, db) of nn.deconv2d(x, W, b, stride) given g = dL/d(window of its output), zero outside it."""
    B, Ci, H, Wd = x.shape
    K, s = W.shape[2], stride
    oy, ox, OH, OW = window
    gf = np.zeros((B, W.shape[1], (H - 1) * s + K, (Wd - 1) * s + K), dtype=g.dtype)
    gf[:, :, oy:oy + OH, ox:ox + OW] = g
    gx, dW = np.zeros_like(x), np.zeros_like(W, dtype=x.dtype)
    for a in range(K):
        for c in range(K):
            gs = gf[:, :, a:a + (H - 1) * s + 1:s, c:c + (Wd - 1) * s + 1:s]
            dW[:, :, K - 1 - a, K - 1 - c] = np.tensordot(x, gs, axes=([0, 2, 3], [0, 2, 3]))
            gx += np.einsum('io,bohw->bihw', W[:, :, K - 1 - a, K - 1 - c].astype(x.dtype), gs)
    return gx, dW, g.sum(axis=(0, 2, 3))


def _eqmask(pre, pooled):
    h2, w2 = pooled.shape[2], pooled.shape[3]
    return pre[:, :, :2 * h2, :2 * w2] == np.repeat(np.repeat(pooled, 2, 2), 2, 3)


def backward(params, s, g_score):
    """{name: (dW, db)} from the maps of a forward pass (`forward`, or another forward's: teacher forcing -- the
    decisions are [out > 0] and [out == its window's maximum] of whatever is handed in)."""
    grads, side = {}, {}
    dt = g_score.dtype
    p = s['p']
    g, dW, db = deconv_bwd(s['final'], params['upsample'][0], g_score, 8, s['win_upsample'])
    grads['upsample'] = (dW, db)
    for dec, sname, pool, src in (('score4', 'score_pool3', 'pool3', 'fused'), ('score2', 'score_pool4', 'pool4', 'score_fr')):
        # the sum's fan-out: the side 1x1 layer on the pool's centre window, then the transposed convolution
        W = params[sname][0]
        gz = np.where(s[sname] > 0, g, 0.0).astype(dt)
        grads[sname] = wgrad(s['in_' + sname], gz, 1)
        oy, ox, H, Wd = s['win_' + sname]
        gs = np.zeros_like(s[pool])
        gs[:, :, oy:oy + H, ox:ox + Wd] = conv_bwd_data(gz, W, 0, (H, Wd))
        side[pool] = gs
        g, dW, db = deconv_bwd(s[src], params[dec][0], g, 2, s['win_' + dec])
        grads[dec] = (dW, db)
    for name, x, keep in (('score_fr', 'drop7', 'keep7'), ('fc7', 'drop6', 'keep6'), ('fc6', 'in_fc6', None)):
        W = params[name][0]
        gz = np.where(s[name] > 0, g, 0.0).astype(dt)
        grads[name] = wgrad(s[x], gz, W.shape[2])
        g = conv_bwd_data(gz, W, 0, s[x].shape[2:])
        if keep is not None and s[keep] is not None:
            g = (g * s[keep] / (1.0 - p)).astype(dt)               # dropout's adjoint
    for bi in range(4, -1, -1):
        names = BLOCKS[bi]
        pool = 'pool%d' % (bi + 1)
        if pool in side:
            g = g + side[pool]                                     # main path first, then the side branch
        for ni in range(len(names) - 1, -1, -1):
            name = names[ni]
            out, x = s[name], s['in_' + name]
            if ni == len(names) - 1:
                pooled = s[pool]
                h2, w2 = pooled.shape[2], pooled.shape[3]
                ga = np.zeros_like(out)
                ga[:, :, :2 * h2, :2 * w2] = np.where(_eqmask(out, pooled), np.repeat(np.repeat(g, 2, 2), 2, 3), 0.0)
                g = ga
            gz = np.where(out > 0, g, 0.0).astype(dt)              # relu'(0) = 0
            pad = s['pad'] if (bi == 0 and ni == 0) else 1
            grads[name] = wgrad(x, gz, 3, pad)
            if not (bi == 0 and ni == 0):
                g = conv_bwd_data(gz, params[name][0], pad, x.shape[2:])
    return grads


def decisions(s):
    """The ReLU and max-pool decisions of a forward pass, as a list of boolean arrays."""
    out = []
    for bi, names in enumerate(BLOCKS):
        out += [s[n] > 0 for n in names]
        out.append(_eqmask(s[names[-1]], s['pool%d' % (bi + 1)]))
    out += [s[n] > 0 for n in ('fc6', 'fc7', 'score_fr', 'score_pool4', 'score_pool3')]
    return out


def penalty(params):
    return float(sum((np.asarray(params[n][0], np.float64) ** 2).sum() for n in PARAM_ORDER))


def loss_of(params, x, T, keep6=None, keep7=None, weight_decay=0.0, p=0.5, pad=100, reuse=None, first=None):
    s = forward(params, x, keep6, keep7, p, pad, reuse, first)
    return loss_and_grad(s['score'], T)[0] + weight_decay * penalty(params), s


def loss_and_param_grads(params, x, T, keep6=None, keep7=None, weight_decay=0.0, p=0.5, pad=100):
    s = forward(params, x, keep6, keep7, p, pad)
    loss, _, _, g, _ = loss_and_grad(s['score'], T)
    grads = backward(params, s, g)
    if weight_decay:
        grads = {n: (dW + 2.0 * weight_decay * params[n][0], db) for n, (dW, db) in grads.items()}
    return loss + weight_decay * penalty(params), grads, s


def flatten(d):
    """PARAM_ORDER, W then b: the layout of FCN8.flat."""
    return np.concatenate([np.asarray(a).ravel() for n in PARAM_ORDER for a in d[n]])


def unflatten(flat, like):
    out, off = {}, 0
    for n in PARAM_ORDER:
        arrs = []
        for a in like[n]:
            arrs.append(flat[off:off + a.size].reshape(a.shape))
            off += a.size
        out[n] = tuple(arrs)
    return out


SMALL = dict(width_div=16, fc_channels=32, n_classes=4)


def make_case(B, H, W, seed=5, void_frac=0.1, dead_border=False):
    """(params float64, x, T, keep6, keep7) of the small net: seeded synthetic weights with conv1_1's bias made
    non-positive (dead_border: the bias of all thirteen block convolutions; see tests/test_fcn8_train_ref.py), an
    image batch, labels with void pixels, two 0/1 masks."""
    from iterative_inference_segm_amd import synthetic as S
    C = SMALL['n_classes']
    rng = np.random.default_rng(seed)
    params = to64(S.make_fcn8_params(3, C, seed=100 + seed, width_div=SMALL['width_div'],
                                     fc_channels=SMALL['fc_channels']))
    for n in ([n for names in BLOCKS for n in names] if dead_border else ['conv1_1']):
        params[n] = (params[n][0], -np.abs(params[n][1]))
    x = rng.random((B, 3, H, W))
    T = S.make_labels(B, H, W, n_classes=C, void_frac=void_frac, seed=seed + 1, block=4).astype(np.float64)
    fh, fw = fc6_hw(H, W)
    keep6 = (rng.random((B, SMALL['fc_channels'], fh, fw)) < 0.5).astype(np.float64)
    keep7 = (rng.random((B, SMALL['fc_channels'], fh, fw)) < 0.5).astype(np.float64)
    return params, x, T, keep6, keep7


def fc6_hw(H, W, pad=100):
    h, w = H + 2 * pad - 2, W + 2 * pad - 2
    for _ in range(5):
        h, w = h // 2, w // 2
    return h - 6, w - 6
