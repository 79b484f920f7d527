"""Float64 (numpy) restatement of FCN-8's backward with the rounding points of kxk='bf16' (DESIGN.md section 17):
tests/fcn8_train_ref.backward itself, with the two functions it forms weight and data gradients with (module-level
names) replaced, for the duration of the call, by ones that first round the operands of fc6 and fc7 to bf16 (to
nearest, ties to even: torch's CPU cast) -- x and g_z of their weight gradients (db stays the sum of the unrounded
g_z), W and g_z of their data gradients.  The two layers are recognised by identity: `backward` hands `wgrad` the
saved input map itself and `conv_bwd_data` the parameter itself.  With rounding off the function is called as it
stands.  Also the plain numpy statements of the two ops the GPU tests compare with.  TEST INFRASTRUCTURE: pinned by
tests/test_kxk_bf16_ref.py; the HIP path's chain error is checked against it (tests/test_gpu_kxk_bf16.py).
"""
import contextlib

import numpy as np
import torch

import fcn8_train_ref as RF

LAYERS = ('fc6', 'fc7')
INPUTS = {'fc6': 'in_fc6', 'fc7': 'drop6'}


def bf16(a):
    """`a` rounded to float32 and then to bf16 (nearest, ties to even: torch on the CPU), as float64."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64).numpy()


def wgrad_kxk(x, gz):
    """dW[co, ci, ky, kx] = sum_{b,y,x} gz[b, co, y, x] x[b, ci, y + ky, x + kx] of a 'valid' layer, K from the shapes"""
    K = x.shape[2] - gz.shape[2] + 1
    OH, OW = gz.shape[2:]
    dW = np.zeros((gz.shape[1], x.shape[1], K, K), dtype=np.result_type(x.dtype, gz.dtype))
    for ky in range(K):
        for kx in range(K):
            dW[:, :, ky, kx] = np.tensordot(gz, x[:, :, ky:ky + OH, kx:kx + OW], axes=([0, 2, 3], [0, 2, 3]))
    return dW


def dgrad_kxk(gz, W):
    """gx[b, ci, y, x] = sum_{co,ky,kx} W[co, ci, ky, kx] gz[b, co, y - ky, x - kx], gz zero outside its plane"""
    K = W.shape[2]
    B, Co, OH, OW = gz.shape
    out = np.zeros((B, W.shape[1], OH + K - 1, OW + K - 1), dtype=np.result_type(gz.dtype, W.dtype))
    for ky in range(K):
        for kx in range(K):
            out[:, :, ky:ky + OH, kx:kx + OW] += np.einsum('oi,bohw->bihw', W[:, :, ky, kx], gz)
    return out


@contextlib.contextmanager
def _swapped(module, name, fn):
    old = getattr(module, name)
    setattr(module, name, fn)
    try:
        yield
    finally:
        setattr(module, name, old)


def fcn8_backward(params, s, g_score, rounded=False):
    """fcn8_train_ref.backward; rounded=True: the operands of fc6's and fc7's weight and data gradients rounded."""
    if not rounded:
        return RF.backward(params, s, g_score)
    inner_w, inner_d = RF.wgrad, RF.conv_bwd_data
    xs = [s[INPUTS[n]] for n in LAYERS]
    Ws = [params[n][0] for n in LAYERS]
    seen = {'w': 0, 'd': 0}

    def wgrad(x, gz, K, pad=0):
        if any(x is t for t in xs):
            seen['w'] += 1
            dW, _ = inner_w(bf16(x).astype(x.dtype), bf16(gz).astype(gz.dtype), K, pad)
            return dW, gz.sum(axis=(0, 2, 3))
        return inner_w(x, gz, K, pad)

    def conv_bwd_data(gz, W, pad, in_hw):
        if any(W is t for t in Ws):
            seen['d'] += 1
            gz, W = bf16(gz).astype(gz.dtype), bf16(W).astype(W.dtype)
        return inner_d(gz, W, pad, in_hw)

    with _swapped(RF, 'wgrad', wgrad), _swapped(RF, 'conv_bwd_data', conv_bwd_data):
        out = RF.backward(params, s, g_score)
    assert seen == {'w': 2, 'd': 2}, seen
    return out


def cosines(a, b):
    """{name: cosine of (dW, db) of a to those of b}"""
    cat = lambda v: np.concatenate([np.asarray(t, np.float64).ravel() for t in v])
    return {n: float(cat(a[n]) @ cat(b[n]) / (np.linalg.norm(cat(a[n])) * np.linalg.norm(cat(b[n])))) for n in a}
