"""Float64 (numpy) restatement of the standard DAE's forward and backward with the rounding points of fwd='bf16'
(DESIGN.md section 20): tests/std_train_ref.forward itself -- oracle/dae.py's forward -- with the function it runs a
convolution with (oracle.nn.conv2d) replaced, for the duration of the call, by one that first rounds W and the layer's
input map (after the concatenation, after DePool2D) to bf16 (to nearest, ties to even: tests/fwd_bf16_ref.bf16);
the bias, the sums, ReLU, the pools, the DePool2D masks, the skip sum and the crop stay float64 statements of what they
were, and so does the whole backward (tests/std_train_ref.backward on the maps of that forward and the parameters
themselves).  With rounding off the functions are called as they stand.  Also one layer on its own (what the
teacher-forced GPU test feeds the GPU's saved inputs to) with the bound of one entry.  TEST INFRASTRUCTURE: pinned by
tests/test_std_fwd_bf16_ref.py; the HIP path is checked against it (tests/test_gpu_std_fwd_bf16.py).
"""
import contextlib

import numpy as np

import std_train_ref as R
from fwd_bf16_ref import bf16, cosines   # noqa: F401 (re-exported)
from oracle import nn
from oracle.dae import _n_pool

U = 2.0 ** -24


@contextlib.contextmanager
def _rounding_convs(seen):
    inner = nn.conv2d

    def conv2d(x, W, b=None, **kw):
        seen.append(tuple(W.shape))
        return inner(bf16(x), bf16(W), b, **kw)

    nn.conv2d = conv2d
    try:
        yield
    finally:
        nn.conv2d = inner


def forward(params, h_list, y, cfg, rounded=False):
    """std_train_ref.forward; rounded=True: W and the input of every encoder and decoder layer rounded to bf16."""
    if not rounded:
        return R.forward(params, h_list, y, cfg)
    seen = []
    with _rounding_convs(seen):
        net = R.forward(params, h_list, y, cfg)
    assert seen == [tuple(params[n][0].shape) for n in R.order_of(cfg)], seen     # every layer, once, in order
    return net


def loss_and_param_grads(params, h_list, y, T, cfg, losses=('crossentropy',), lmb=1.0, rounded=False):
    """(loss, {name: (dW, db)}, net): the forward of the mode, then the float64 loss and backward as they are."""
    net = forward(params, h_list, y, cfg, rounded)
    loss, _, _, g, _ = R.loss_and_grad(net['score'], T, losses, lmb)
    return loss, R.backward(params, h_list, net, g, cfg), net


def layer_calls(saved, h_list, cfg):
    """{name: (x, pad, relu, other, output name)} of every layer on the maps of a forward pass (`saved`: 'input',
    'pre%d', 'pool%d', 'fused_up%d'): x the layer's input as the kernel forms it (h first, then the features;
    DePool2D of the level's input under the level's own mask), `other` the map whose center crop the skip sum adds
    (None: no addend), and the name of the saved map the layer's launch wrote."""
    concat_h = list(cfg['concat_h'])
    n_pool, total = _n_pool(concat_h, cfg['additional_pool'])
    skip, padding = cfg.get('skip', True), cfg.get('padding', 100)
    hmap = dict(zip(concat_h, h_list))
    calls = {}
    for p in range(1, total + 1):
        x = saved['pool%d' % (p - 1)] if p > 1 else saved['input']
        at = 'input' if p == 1 else 'pool%d' % (p - 1)
        if at in hmap:
            x = nn.concat_h_first(hmap[at], x)
        pad = padding if (p == 1 and len(concat_h) == 1 and concat_h[-1] != 'input' and padding > 0) else 1
        calls['conv%d_1' % p] = (x, pad, True, None, 'pre%d' % p)
    for p in range(total, 0, -1):
        t_in = saved['pool%d' % total] if p == total else saved['fused_up%d' % (p + 1)]
        x = nn.depool_eqmask(t_in, saved['pre%d' % p], saved['pool%d' % p])
        other = saved['pool%d' % (p - 1)] if p > 1 else saved['input']
        calls['up_conv%d' % p] = (x, 1, False, other, 'fused_up%d' % p) if skip and p > 1 else \
            (x, 1, False, ('crop', other), 'fused_up%d' % p)
    return calls


def _finish(z, other):
    if other is None:
        return z
    if isinstance(other, tuple):                                 # the crop alone (fcn_up.py:104-113)
        return nn.crop_like(other[1], z)
    return nn.crop_sum(z, other)


def layer(W, b, x, pad, relu, other=None, rounded=True):
    """One layer of the mode on its own: the operands rounded (or not), float64 from there on; the skip addend
    (center crop of `other`) is added to the cropped linear result (no ReLU on such a layer)."""
    x, W = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(W, np.float64)
    if rounded:
        W, x = bf16(W), bf16(x)
    return _finish(nn.conv2d(x, W, np.asarray(b, np.float64), pad=pad, relu=relu), other)


def bound(W, b, x, pad, other=None):
    """Per entry: (n + 3) 2^-24 (sum |a b| + |b| + |addend|) over the ROUNDED operands, n = 9 Cin -- fp32
    accumulation of n exact products in any order, the bias and the addend."""
    n = W.shape[1] * W.shape[2] * W.shape[3]
    mag = nn.conv2d(np.abs(bf16(x)), np.abs(bf16(W)), np.abs(np.asarray(b, np.float64)), pad=pad, relu=False)
    if other is not None and not isinstance(other, tuple):
        other = np.abs(other)
    return (n + 3) * U * _finish(mag, other)
