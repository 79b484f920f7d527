"""Float64 (numpy) restatement of what training FC-DenseNet computes: the forward of
oracle/densenet.py on oracle/nn.py's conv2d / deconv2d / maxpool2 / center_crop with a dropout mask (DropoutLayer p,
rescale=True) behind the convolution of every BN_ReLU_Conv and TransitionDown, the masked cross-entropy of
tests/ctx_train_ref.py (imported) + weight_decay * sum p^2 over every W and every gamma (never beta or a bias), and the
backward pass by hand-written reverse mode in the project's conventions: BatchNorm with BATCH statistics (the mean and
variance terms are part of g_x), relu'(0) = 0, max-pool gradient to EVERY position equal to the window maximum and no
ReLU gate behind TransitionDown's pool (it pools a linear map).  A gradient stack mirrors every feature stack; the
layers are walked in reverse creation order (`program`).  TEST INFRASTRUCTURE: pinned by central finite differences
(tests/test_densenet_train_ref.py); the HIP path is checked against it.  `backward` runs in the dtype of what it is
handed (float32 maps give the numpy-float32 reference error of tests/test_gpu_densenet_train.py).
"""
import numpy as np

from ctx_train_ref import loss_and_grad, rmsprop_step   # noqa: F401 (re-exported)
from fcn8_train_ref import conv_bwd_data, deconv_bwd, wgrad
from oracle import nn
from oracle.densenet import layer_plan

BN_EPS = 1e-4
THIN = dict(nlpb=[2, 3, 2, 3, 2], n_pool=2, growth=4, n_first=8, n_classes=4)
WIDE = dict(nlpb=[2, 3, 2, 3, 2], n_pool=2, growth=16, n_first=48, n_classes=4)


def plan_of(cfg):
    return layer_plan(cfg['nlpb'], cfg['n_pool'], cfg['growth'], cfg['n_first'], 3, cfg['n_classes'])


def program(cfg):
    """(steps, caps): the layers in creation order as dicts -- kind, li (index into params), sid (the stack read),
    n (channels read: [0, n), for 'tu' [block0, n)), and where the result goes -- and the channel capacity of every
    stack (down path's, the bottleneck's, up path's, in creation order)."""
    nlpb, n_pool, g = cfg['nlpb'], cfg['n_pool'], cfg['growth']
    steps, caps = [], []
    li = ki = ti = 0
    n = cfg['n_first']
    caps.append(n + g * nlpb[0])
    steps.append(dict(kind='first', li=li, sid=0, cout=n))
    li += 1
    sid, skips = 0, []
    for i in range(n_pool):
        for _ in range(nlpb[i]):
            steps.append(dict(kind='brc', li=li, sid=sid, n=n, ki=ki))
            li, ki, n = li + 1, ki + 1, n + g
        skips.append((sid, n))
        caps.append(n + g * nlpb[i + 1])
        steps.append(dict(kind='td', li=li, sid=sid, n=n, ki=ki, ti=ti, dst=sid + 1))
        li, ki, ti, sid = li + 1, ki + 1, ti + 1, sid + 1
    skips = skips[::-1]
    block0 = n
    for _ in range(nlpb[n_pool]):
        steps.append(dict(kind='brc', li=li, sid=sid, n=n, ki=ki))
        li, ki, n = li + 1, ki + 1, n + g
    for i in range(n_pool):
        keep = g * nlpb[n_pool + i]
        skip_sid, skip_n = skips[i]
        caps.append(keep + skip_n + g * nlpb[n_pool + i + 1])
        steps.append(dict(kind='tu', li=li, sid=sid, block0=block0, n=n, dst=sid + 1, keep=keep, skip_sid=skip_sid,
                          skip_n=skip_n))
        li, sid = li + 1, sid + 1
        n = keep + skip_n
        block0 = n
        for _ in range(nlpb[n_pool + i + 1]):
            steps.append(dict(kind='brc', li=li, sid=sid, n=n, ki=ki))
            li, ki, n = li + 1, ki + 1, n + g
    steps.append(dict(kind='softmax', li=li, sid=sid, n=n))
    return steps, caps


def n_keeps(cfg):
    return sum(1 for e in program(cfg)[0] if e['kind'] in ('brc', 'td'))


def maxpool2(x):
    """oracle.nn.maxpool2 as the maximum of its four strided slices (the same values, faster)."""
    h, w = x.shape[2] // 2, x.shape[3] // 2
    v = x[:, :, :2 * h, :2 * w]
    return np.maximum(np.maximum(v[:, :, 0::2, 0::2], v[:, :, 0::2, 1::2]),
                      np.maximum(v[:, :, 1::2, 0::2], v[:, :, 1::2, 1::2]))


def _eqmask(pre, pooled):
    h2, w2 = pooled.shape[2], pooled.shape[3]
    return pre[:, :, :2 * h2, :2 * w2] == np.repeat(np.repeat(pooled, 2, 2), 2, 3)


def bn_parts(x, q, mean, inv_std):
    """(xhat, y) of one consumer (beta, gamma in q) on the channels x of a stack with the handed-in statistics."""
    n = x.shape[1]
    dt = x.dtype
    m, r = mean[:n].astype(dt)[None, :, None, None], inv_std[:n].astype(dt)[None, :, None, None]
    gamma, beta = q['gamma'].astype(dt)[None, :, None, None], q['beta'].astype(dt)[None, :, None, None]
    d = x - m
    return d * r, d * (gamma * r) + beta


def bn_relu_bwd(x, q, mean, inv_std, g_t):
    """(g_x, dbeta, dgamma) of t = relu(gamma xhat + beta) with batch statistics, per DESIGN.md section 21."""
    xhat, y = bn_parts(x, q, mean, inv_std)
    dt = x.dtype
    N = x.shape[0] * x.shape[2] * x.shape[3]
    g_y = np.where(y > 0, g_t, 0).astype(dt)
    dbeta = g_y.sum(axis=(0, 2, 3))
    dgamma = (g_y * xhat).sum(axis=(0, 2, 3))
    k = (q['gamma'].astype(dt) * inv_std[:x.shape[1]].astype(dt))[None, :, None, None]
    g_x = k * (g_y - dbeta[None, :, None, None] / dt.type(N) - xhat * (dgamma[None, :, None, None] / dt.type(N)))
    return g_x.astype(dt), dbeta, dgamma


def forward(params, x, cfg, keeps=None, p=0.2):
    """The saved maps of a training forward: 'stacks' (every stack whole, (B, cap, H, W)), 'mean' / 'inv_std' (their
    batch statistics, per stack), 'keeps' (the 0/1 masks per brc / td layer in creation order; None: the
    deterministic pass), 'td_pre' / 'td_pooled' (per TransitionDown the post-dropout map and its pool), 'gates'
    (per brc / td the ReLU decisions y > 0), 'win' (per TransitionUp its crop window), 'score'."""
    steps, caps = program(cfg)
    B = x.shape[0]
    dt = x.dtype
    s = dict(x=x, stacks=[None] * len(caps), mean=[np.zeros(c, dt) for c in caps], inv_std=[np.zeros(c, dt) for c in caps],
             keeps=keeps, td_pre=[], td_pooled=[], gates=[], win={}, p=p)

    def put(sid, c0, v):
        if s['stacks'][sid] is None:
            s['stacks'][sid] = np.zeros((B, caps[sid]) + v.shape[2:], dt)
        s['stacks'][sid][:, c0:c0 + v.shape[1]] = v
        s['mean'][sid][c0:c0 + v.shape[1]] = v.mean(axis=(0, 2, 3))
        s['inv_std'][sid][c0:c0 + v.shape[1]] = 1.0 / np.sqrt(v.var(axis=(0, 2, 3)) + BN_EPS)

    def drop(z, ki):
        return z if keeps is None else z * keeps[ki] / (1.0 - p)

    for e in steps:
        q = params[e['li']]
        W = np.ascontiguousarray(q['W'])
        sid = e['sid']
        if e['kind'] == 'first':
            put(0, 0, nn.conv2d(x, W, q['b'], pad=1))
            continue
        stack = s['stacks'][sid]
        if e['kind'] in ('brc', 'td'):
            n = e['n']
            _, y = bn_parts(stack[:, :n], q, s['mean'][sid], s['inv_std'][sid])
            s['gates'].append(y > 0)
            t = np.maximum(y, 0)
            if e['kind'] == 'brc':
                put(sid, n, drop(nn.conv2d(t, W, q['b'], pad=1), e['ki']))
            else:
                pre = drop(nn.conv2d(t, W, q['b'], pad=0), e['ki'])
                pooled = maxpool2(pre)
                s['td_pre'].append(pre)
                s['td_pooled'].append(pooled)
                put(e['dst'], 0, pooled)
        elif e['kind'] == 'tu':
            blk = np.ascontiguousarray(stack[:, e['block0']:e['n']])
            up = nn.deconv2d(blk, W, q['b'], stride=2)
            skip = s['stacks'][e['skip_sid']]
            H, Wd = min(up.shape[2], skip.shape[2]), min(up.shape[3], skip.shape[3])
            assert (H, Wd) == skip.shape[2:]
            s['win'][e['li']] = ((up.shape[2] - H) // 2, (up.shape[3] - Wd) // 2, H, Wd)
            put(e['dst'], 0, nn.center_crop(up, H, Wd))
            put(e['dst'], e['keep'], skip[:, :e['skip_n']])
        else:
            s['score'] = nn.conv2d(np.ascontiguousarray(stack[:, :e['n']]), W, q['b'], pad=0)
    return s


def dead_arrays(cfg):
    """[(li, 'b')]: the arrays whose gradient is ZERO by construction -- the bias of a TransitionUp whose output is read
    through BatchNorm only (every one but the last: no dropout behind it, and batch statistics take a per-channel
    constant out again).  What a backward pass computes there is the rounding of a sum that cancels."""
    steps, caps = program(cfg)
    return [(e['li'], 'b') for e in steps if e['kind'] == 'tu' and e['dst'] != len(caps) - 1]


def backward(params, s, g_score, cfg, mags=None):
    """[{'W', 'b'[, 'gamma', 'beta']}] per layer from the saved maps of a forward (`forward`, or another forward's:
    teacher forcing -- the decisions are taken on whatever is handed in).  mags (a dict): receives per TransitionUp
    {li: sum |g| per channel}, the magnitude of the sum its db is."""
    steps, _ = program(cfg)
    dt = g_score.dtype
    p = s['p']
    c = lambda a: np.ascontiguousarray(a, dtype=dt)
    stacks = [c(a) for a in s['stacks']]
    gst = [np.zeros_like(a) for a in stacks]
    grads = [None] * len(params)
    for e in reversed(steps):
        q = params[e['li']]
        W = c(q['W'])
        sid = e['sid']
        stack = stacks[sid]
        if e['kind'] == 'softmax':
            n = e['n']
            dW, db = wgrad(c(stack[:, :n]), g_score, 1)
            gst[sid][:, :n] += conv_bwd_data(g_score, W, 0, stack.shape[2:])
            grads[e['li']] = dict(W=dW, b=db)
        elif e['kind'] in ('brc', 'td'):
            n = e['n']
            if e['kind'] == 'brc':
                gz = c(gst[sid][:, n:n + W.shape[0]])
            else:
                pre, pooled = c(s['td_pre'][e['ti']]), c(s['td_pooled'][e['ti']])
                h2, w2 = pooled.shape[2:]
                gz = np.zeros_like(pre)
                gpool = gst[e['dst']][:, :n]
                gz[:, :, :2 * h2, :2 * w2] = np.where(_eqmask(pre, pooled), np.repeat(np.repeat(gpool, 2, 2), 2, 3), 0)
            if s['keeps'] is not None:
                gz = (gz * c(s['keeps'][e['ki']]) / dt.type(1.0 - p)).astype(dt)
            x = c(stack[:, :n])
            _, y = bn_parts(x, q, s['mean'][sid], s['inv_std'][sid])
            t = np.maximum(y, 0).astype(dt)
            K = W.shape[2]
            dW, db = wgrad(t, gz, K, K // 2)
            g_t = conv_bwd_data(gz, W, K // 2, x.shape[2:])
            g_x, dbeta, dgamma = bn_relu_bwd(x, q, s['mean'][sid], s['inv_std'][sid], g_t)
            gst[sid][:, :n] += g_x
            grads[e['li']] = dict(W=dW, b=db, gamma=dgamma, beta=dbeta)
        elif e['kind'] == 'tu':
            keep = e['keep']
            g = c(gst[e['dst']][:, :keep])
            blk = c(stack[:, e['block0']:e['n']])
            gx, dW, db = deconv_bwd(blk, W, g, 2, s['win'][e['li']])
            if mags is not None:
                mags[e['li']] = np.abs(g).sum(axis=(0, 2, 3))
            gst[sid][:, e['block0']:e['n']] += gx
            gst[e['skip_sid']][:, :e['skip_n']] += gst[e['dst']][:, keep:keep + e['skip_n']]
            grads[e['li']] = dict(W=dW, b=db)
        else:
            dW, db = wgrad(c(s['x']), c(gst[0][:, :e['cout']]), 3, 1)
            grads[e['li']] = dict(W=dW, b=db)
    return grads


FIELDS = ('gamma', 'beta', 'W', 'b')          # the order of the module's flat buffer, per layer


def arrays(d):
    """The arrays of params / grads in the order of FCDenseNet.flat: per layer gamma, beta (BatchNorm), W, b."""
    return [(li, f, q[f]) for li, q in enumerate(d) for f in FIELDS if f in q]


def flatten(d):
    return np.concatenate([np.asarray(a).ravel() for _, _, a in arrays(d)])


def unflatten(flat, like):
    out, off = [], 0
    for q in like:
        r = {'kind': q['kind']} if 'kind' in q else {}
        for f in FIELDS:
            if f in q:
                r[f] = flat[off:off + q[f].size].reshape(q[f].shape)
                off += q[f].size
        out.append(r)
    return out


def penalty(params):
    return float(sum((np.asarray(q[f], np.float64) ** 2).sum() for q in params for f in ('W', 'gamma') if f in q))


def loss_of(params, x, T, cfg, keeps=None, weight_decay=0.0, p=0.2):
    s = forward(params, x, cfg, keeps, p)
    return loss_and_grad(s['score'], T)[0] + weight_decay * penalty(params), s


def loss_and_param_grads(params, x, T, cfg, keeps=None, weight_decay=0.0, p=0.2):
    s = forward(params, x, cfg, keeps, p)
    loss, _, _, g, _ = loss_and_grad(s['score'], T)
    grads = backward(params, s, g, cfg)
    if weight_decay:
        for q, gq in zip(params, grads):
            for f in ('W', 'gamma'):
                if f in gq:
                    gq[f] = gq[f] + 2.0 * weight_decay * q[f]
    return loss + weight_decay * penalty(params), grads, s


def decisions(s):
    """The ReLU and max-pool decisions of a forward pass, as a list of boolean arrays."""
    return list(s['gates']) + [_eqmask(a, b) for a, b in zip(s['td_pre'], s['td_pooled'])]


def min_variance(s, cfg):
    """The smallest batch variance over every BatchNorm input channel of the forward `s`."""
    steps, _ = program(cfg)
    v = np.inf
    for e in steps:
        if e['kind'] in ('brc', 'td'):
            v = min(v, float(s['stacks'][e['sid']][:, :e['n']].var(axis=(0, 2, 3)).min()))
    return v


def make_params(cfg, seed):
    """He-uniform weights, small biases, gamma in [0.7, 1.3], beta in [-0.2, 0.2]; float64, creation order."""
    rng = np.random.default_rng(seed)
    out = []
    for kind, cin, cout in plan_of(cfg):
        q = {'kind': kind}
        if kind in ('brc', 'td'):
            q['gamma'] = rng.uniform(0.7, 1.3, size=cin)
            q['beta'] = rng.uniform(-0.2, 0.2, size=cin)
        k = 1 if kind in ('td', 'softmax') else 3
        shape, fan = ((cin, cout, 3, 3), cin * 9 / 4.0) if kind == 'tu' else ((cout, cin, k, k), cin * k * k)
        lim = np.sqrt(6.0 / fan)
        q['W'] = rng.uniform(-lim, lim, size=shape)
        q['b'] = rng.uniform(-0.1, 0.1, size=cout)
        out.append(q)
    return out


def make_case(cfg, B=2, H=13, W=18, seed=3, p=0.2, void_frac=0.1):
    """(params float64, x, T one-hot with void last, keeps) of a small net: seeded weights, an image batch, labels with
    void pixels, one drawn 0/1 mask per brc / td layer."""
    from iterative_inference_segm_amd import synthetic as S
    rng = np.random.default_rng(seed)
    params = make_params(cfg, 200 + seed)
    x = rng.random((B, 3, H, W))
    T = S.make_labels(B, H, W, n_classes=cfg['n_classes'], void_frac=void_frac, seed=seed + 1, block=4).astype(np.float64)
    s = forward(params, x, cfg)
    steps, _ = program(cfg)
    keeps = []
    for e in steps:
        if e['kind'] == 'brc':
            shape = (B, cfg['growth']) + s['stacks'][e['sid']].shape[2:]
        elif e['kind'] == 'td':
            shape = s['td_pre'][e['ti']].shape
        else:
            continue
        keeps.append((rng.random(shape) >= p).astype(np.float64))
    return params, x, T, keeps
