"""Float64 (numpy) restatement of what training the context-module DAE computes: the two training losses of
the reference (metrics.py:68-91 crossentropy, :144-156 squared_error with an int `void`), the backward pass of
oracle/contextmod.py by hand-written reverse mode, and Lasagne's rmsprop / adam.  TEST INFRASTRUCTURE: pinned
by central finite differences (tests/test_ctx_train_ref.py); the HIP path is checked against it.

Conventions as oracle/dae_grad.py: relu'(0) = 0.  T.clip passes the gradient only inside [1e-7, 1 - 1e-7].
Adam's powers 0.9^t / 0.999^t are running products (one multiplication per step), which pins their rounding.
"""
import numpy as np

from oracle import nn
from oracle.contextmod import DILATIONS, PARAM_ORDER

EPS = 10e-8            # metrics.py _EPSILON


def _valid(x, W_oihw, b, d, relu):
    return nn.conv2d(x, np.ascontiguousarray(W_oihw), b, pad=0, dilation=d, relu=relu)


def forward(params, h, y):
    """Returns (cat, outs): the zero-bordered concat buffer conv1 reads and the eight layer outputs (conv1's
    as its (H, W) map; the dilated layers see it inside PadLayer(32)'s zeros)."""
    B, _, H, W = y.shape
    cat = np.zeros((B, h.shape[1] + y.shape[1], H + 2, W + 2), dtype=y.dtype)
    cat[:, :h.shape[1], 1:-1, 1:-1] = h
    cat[:, h.shape[1]:, 1:-1, 1:-1] = y
    Wc, bc = params['conv1']
    outs = [_valid(cat, Wc, bc, 1, True)]
    t = np.zeros((B, outs[0].shape[1], H + 64, W + 64), dtype=y.dtype)
    t[:, :, 32:-32, 32:-32] = outs[0]
    for i, d in enumerate(DILATIONS):
        Wd, bd = params['dilconv%d' % (i + 1)]
        t = _valid(t, np.transpose(Wd, (1, 0, 2, 3)), bd, d, True)
        outs.append(t)
    W7, b7 = params['dilconv7']
    outs.append(_valid(t, np.transpose(W7, (1, 0, 2, 3)), b7, 1, False))
    return cat, outs


def loss_and_grad(score, T, losses=('crossentropy',), lmb=1.0):
    """(loss, ce, se, g_score, (N_ce, N_se)).  T one-hot (B, C+1, H, W), void channel last."""
    C = score.shape[1]
    r = nn.softmax_channels(score)
    label = T.argmax(axis=1)
    m_ce = (label != C).astype(score.dtype)
    m_se = T[:, :C].sum(axis=1)
    n_ce, n_se = m_ce.sum(), m_se.sum()
    i_ce = 1.0 / n_ce if n_ce > 0 else 0.0
    i_se = 1.0 / n_se if n_se > 0 else 0.0
    lab = np.where(label == C, 0, label)
    rl = np.take_along_axis(r, lab[:, None], axis=1)[:, 0]
    ce = float((-np.log(np.clip(rl, EPS, 1.0 - EPS)) * m_ce).sum() * i_ce)
    diff = r - T[:, :C]
    se = float(((diff ** 2).mean(axis=1) * m_se).sum() * i_se)
    gr = np.zeros_like(r)
    loss = 0.0
    if 'crossentropy' in losses:
        loss += ce
        inside = (rl >= EPS) & (rl <= 1.0 - EPS)
        gl = np.where(inside, -1.0 / rl, 0.0) * m_ce * i_ce
        np.put_along_axis(gr, lab[:, None], gl[:, None], axis=1)
    if 'squared_error' in losses:
        loss += lmb * se
        gr += (lmb * i_se) * m_se[:, None] * 2.0 * diff / C
    g = r * (gr - (r * gr).sum(axis=1, keepdims=True))
    return loss, ce, se, g, (float(n_ce), float(n_se))


def wgrad(x, gz, K, d):
    """dW[ci, co, ky, kx] = sum x[b, ci, y + ky d, x + kx d] gz[b, co, y, x]; db[co] = sum gz."""
    B, Co, OH, OW = gz.shape
    dW = np.zeros((x.shape[1], Co, K, K), dtype=np.float64)
    for ky in range(K):
        for kx in range(K):
            xs = x[:, :, ky * d:ky * d + OH, kx * d:kx * d + OW]
            dW[:, :, ky, kx] = np.tensordot(xs, gz, axes=([0, 2, 3], [0, 2, 3]))
    return dW, gz.sum(axis=(0, 2, 3))


def _bwd_data(gz, W_iohw, d):
    """Adjoint of the 'valid' dilated layer w.r.t. its input: W[in,out,k,k] flipped, read as W[out,in,k,k]."""
    K = W_iohw.shape[2]
    Wadj = np.ascontiguousarray(W_iohw[:, :, ::-1, ::-1])
    return nn.conv2d(gz, Wadj, None, pad=d * (K - 1), dilation=d)


def backward(params, cat, outs, g_score):
    """{name: (dW, db)} in the parameters' own layouts, from the saved layer outputs (`forward`, or another
    forward's: teacher forcing -- the masks are [out > 0] of whatever is handed in)."""
    grads = {}
    H, W = outs[0].shape[2:]
    W7 = params['dilconv7'][0]
    grads['dilconv7'] = wgrad(outs[6], g_score, 1, 1)
    g = _bwd_data(g_score, W7, 1)
    pad32 = np.zeros(outs[0].shape[:2] + (H + 64, W + 64), dtype=np.float64)
    pad32[:, :, 32:-32, 32:-32] = outs[0]
    for L in range(6, 0, -1):
        d = DILATIONS[L - 1]
        x = outs[L - 1] if L > 1 else pad32
        gz = np.where(outs[L] > 0, g, 0.0)
        grads['dilconv%d' % L] = wgrad(x, gz, 3, d)
        g = _bwd_data(gz, params['dilconv%d' % L][0], d)
    g = g[:, :, 32:-32, 32:-32]                              # PadLayer(32)'s adjoint
    gz = np.where(outs[0] > 0, g, 0.0)
    dW, db = wgrad(cat, gz, 3, 1)
    grads['conv1'] = (np.ascontiguousarray(np.transpose(dW, (1, 0, 2, 3))), db)   # W[out,in,k,k]
    return grads


def to64(params):
    return {k: tuple(np.asarray(a, np.float64) for a in v) for k, v in params.items()}


def loss_of(params, h, y, T, losses=('crossentropy',), lmb=1.0):
    _, outs = forward(params, h, y)
    return loss_and_grad(outs[-1], T, losses, lmb)[0]


def loss_and_param_grads(params, h, y, T, losses=('crossentropy',), lmb=1.0):
    cat, outs = forward(params, h, y)
    loss, _, _, g, _ = loss_and_grad(outs[-1], T, losses, lmb)
    return loss, backward(params, cat, outs, g)


def flatten(d):
    """PARAM_ORDER, W then b: the layout of ContextModDAE.flat."""
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


def rmsprop_step(p, g, a, lr, dtype=np.float64):
    """lasagne.updates.rmsprop, rho 0.9, epsilon 1e-6, every operation rounded in `dtype`."""
    t = dtype
    rho, one, eps = t(0.9), t(1), t(1e-6)
    a = rho * a + (one - rho) * (g * g)
    p = p - (t(lr) * g) / np.sqrt(a + eps)
    return p.astype(t), a.astype(t)


def adam_step(p, g, m, v, state, lr, dtype=np.float64):
    """lasagne.updates.adam, beta 0.9 / 0.999, epsilon 1e-8; state = (t, 0.9^t, 0.999^t), start (0, 1, 1)."""
    t = dtype
    b1, b2, one, eps = t(0.9), t(0.999), t(1), t(1e-8)
    state = (state[0] + 1, t(state[1]) * b1, t(state[2]) * b2)
    alpha = (t(lr) * np.sqrt(one - state[2])) / (one - state[1])
    m = b1 * m + (one - b1) * g
    v = b2 * v + (one - b2) * (g * g)
    p = p - (alpha * m) / (np.sqrt(v) + eps)
    return p.astype(t), m.astype(t), v.astype(t), state
