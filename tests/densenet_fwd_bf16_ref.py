"""Float64 (numpy) restatement of FC-DenseNet's training forward with the rounding points of fwd='bf16' (DESIGN.md
section 25): tests/densenet_train_ref.forward stated again layer by layer, with W and t = relu(BatchNorm(stack)) of
every 'brc' layer rounded to bf16 (to nearest, ties to even: torch's CPU cast) when `rounded`; BatchNorm, the bias, the
sum, the dropout factor, TransitionDown, TransitionUp, the first and the score layer stay float64 statements of what
they were.  With rounding off it is pinned equal to densenet_train_ref.forward.  Also one layer on its own (what the
teacher-forced GPU test feeds the GPU's saved stacks to) and the bound of one entry.  TEST INFRASTRUCTURE: pinned by
tests/test_densenet_fwd_bf16_ref.py; the HIP path is checked against it (tests/test_gpu_densenet_fwd_bf16.py).
"""
import numpy as np

import densenet_train_ref as RD
from fwd_bf16_ref import TIES                      # noqa: F401 (re-exported)
from kxk_bf16_ref import bf16
from oracle import nn

U = 2.0 ** -24


def bn_relu(x, beta, gamma, mean, inv_std):
    """t = max((x - mean) (gamma inv_std) + beta, 0) per channel of x (B, n, H, W), float64."""
    x = np.asarray(x, np.float64)
    n = x.shape[1]
    v = lambda a: np.asarray(a, np.float64)[:n][None, :, None, None]
    return np.maximum((x - v(mean)) * (v(gamma) * v(inv_std)) + v(beta), 0)


def scale_of(p):
    """dropout_apply's factor as the kernels form it: 1 / (1 - p) in float32."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def layer(W, b, t, keep=None, p=0.0, rounded=True):
    """One 'brc' layer from t on: (sum_{c,ky,kx} W tpad + b) keep s in float64, the operands rounded (or not)."""
    W, t = np.asarray(W, np.float64), np.asarray(t, np.float64)
    if rounded:
        W, t = bf16(W), bf16(t)
    z = nn.conv2d(np.ascontiguousarray(t), np.ascontiguousarray(W), np.asarray(b, np.float64), pad=1, relu=False)
    return z if keep is None else z * np.asarray(keep, np.float64) * scale_of(p)


def bound(W, b, t, keep=None, p=0.0):
    """Per entry: (9 n + 3) 2^-24 (sum |a b| + |b|) s over the ROUNDED operands -- any-order fp32 accumulation of 9 n
    exact products (9 n - 1 roundings), the slabs' sum and the bias (two more), the mask's factor (two more)."""
    n = W.shape[1]
    mag = nn.conv2d(np.ascontiguousarray(np.abs(bf16(t))), np.ascontiguousarray(np.abs(bf16(W))),
                    np.abs(np.asarray(b, np.float64)), pad=1, relu=False)
    return (9 * n + 3) * U * mag * (1.0 if keep is None else scale_of(p))


def forward(params, x, cfg, keeps=None, p=0.2, rounded=False):
    """densenet_train_ref.forward's saved maps; rounded=True: W and t of every 'brc' layer rounded to bf16."""
    steps, caps = RD.program(cfg)
    B, dt = x.shape[0], x.dtype
    s = dict(x=x, stacks=[None] * len(caps), mean=[np.zeros(c, dt) for c in caps],
             inv_std=[np.zeros(c, dt) for c in caps], keeps=keeps, td_pre=[], td_pooled=[], gates=[], win={}, p=p)

    def put(sid, c0, v):
        if s['stacks'][sid] is None:
            s['stacks'][sid] = np.zeros((B, caps[sid]) + v.shape[2:], dt)
        s['stacks'][sid][:, c0:c0 + v.shape[1]] = v
        s['mean'][sid][c0:c0 + v.shape[1]] = v.mean(axis=(0, 2, 3))
        s['inv_std'][sid][c0:c0 + v.shape[1]] = 1.0 / np.sqrt(v.var(axis=(0, 2, 3)) + RD.BN_EPS)

    drop = lambda z, ki: z if keeps is None else z * keeps[ki] / (1.0 - p)
    for e in steps:
        q = params[e['li']]
        W, sid = np.ascontiguousarray(q['W']), e['sid']
        if e['kind'] == 'first':
            put(0, 0, nn.conv2d(x, W, q['b'], pad=1))
            continue
        stack = s['stacks'][sid]
        if e['kind'] in ('brc', 'td'):
            n = e['n']
            _, y = RD.bn_parts(stack[:, :n], q, s['mean'][sid], s['inv_std'][sid])
            s['gates'].append(y > 0)
            t = np.maximum(y, 0)
            if e['kind'] == 'brc':
                if rounded:
                    t, W = bf16(t).astype(dt), bf16(W).astype(dt)
                put(sid, n, drop(nn.conv2d(np.ascontiguousarray(t), W, q['b'], pad=1), e['ki']))
            else:
                pre = drop(nn.conv2d(t, W, q['b'], pad=0), e['ki'])
                pooled = RD.maxpool2(pre)
                s['td_pre'].append(pre)
                s['td_pooled'].append(pooled)
                put(e['dst'], 0, pooled)
        elif e['kind'] == 'tu':
            up = nn.deconv2d(np.ascontiguousarray(stack[:, e['block0']:e['n']]), W, q['b'], stride=2)
            skip = s['stacks'][e['skip_sid']]
            H, Wd = min(up.shape[2], skip.shape[2]), min(up.shape[3], skip.shape[3])
            assert (H, Wd) == skip.shape[2:]
            s['win'][e['li']] = ((up.shape[2] - H) // 2, (up.shape[3] - Wd) // 2, H, Wd)
            put(e['dst'], 0, nn.center_crop(up, H, Wd))
            put(e['dst'], e['keep'], skip[:, :e['skip_n']])
        else:
            s['score'] = nn.conv2d(np.ascontiguousarray(stack[:, :e['n']]), W, q['b'], pad=0)
    return s


def one_minus_cosines(a, b, cfg):
    """{(li, field): 1 - cosine} between two gradient lists (densenet_train_ref.backward's), dead arrays left out."""
    dead = set(RD.dead_arrays(cfg))
    out = {}
    for (li, f, u), (_, _, v) in zip(RD.arrays(a), RD.arrays(b)):
        if (li, f) in dead:
            continue
        u, v = np.asarray(u, np.float64).ravel(), np.asarray(v, np.float64).ravel()
        out[(li, f)] = 1.0 - float(u @ v / (np.linalg.norm(u) * np.linalg.norm(v)))
    return out


def rounding_case(n=17, Cout=16, B=2, H=7, W=9, seed=21):
    """(W, b, x, beta, gamma, mean, inv_std) of the seeded non-integer case: normal x with its own batch statistics,
    He-scaled normal W; float32 values held in float64 arrays."""
    rng = np.random.default_rng(seed)
    f = lambda a: np.asarray(a).astype(np.float32).astype(np.float64)
    x = f(rng.standard_normal((B, n, H, W)) * 1.5 + 0.3)
    Wt = f(rng.standard_normal((Cout, n, 3, 3)) * np.sqrt(2.0 / (9 * n)))
    b = f(rng.uniform(-0.1, 0.1, Cout))
    beta, gamma = f(rng.uniform(-0.2, 0.2, n)), f(rng.uniform(0.7, 1.3, n))
    mean, inv_std = f(x.mean(axis=(0, 2, 3))), f(1.0 / np.sqrt(x.var(axis=(0, 2, 3)) + RD.BN_EPS))
    return Wt, b, x, beta, gamma, mean, inv_std
