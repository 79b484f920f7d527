"""Float64 (numpy) restatement of FCN-8's training forward with the rounding points of fwd='bf16' (DESIGN.md
section 18): tests/fcn8_train_ref.forward itself, with the function it runs a convolution layer with (a module-level
name) replaced, for the duration of the call, by one that first rounds W and the input map of the fifteen layers of
the mode -- the thirteen 3x3 layers, fc6, fc7 -- to bf16 (to nearest, ties to even: torch's CPU cast); the bias, the
sum, ReLU, the pools, dropout, the score and transposed layers stay float64 statements of what they were.  With
rounding off the function is called as it stands.  Also one layer on its own (what the teacher-forced GPU test feeds
the GPU's saved inputs to), the plain statement of the op, and the bound of one entry.  TEST INFRASTRUCTURE: pinned by
tests/test_fwd_bf16_ref.py; the HIP path is checked against it (tests/test_gpu_fwd_bf16.py).
"""
import numpy as np

import fcn8_train_ref as RF
from kxk_bf16_ref import _swapped, bf16, cosines   # noqa: F401 (re-exported)
from oracle import nn

LAYERS = tuple(n for names in RF.BLOCKS for n in names) + ('fc6', 'fc7')
U = 2.0 ** -24


def conv_valid(x, W, b=None, relu=True, pad=0):
    """z[b, co, y, x] = relu(sum_{ci,ky,kx} W[co, ci, ky, kx] xpad[b, ci, y + ky, x + kx] + b[co]) in float64"""
    x, W = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(W, np.float64)
    return nn.conv2d(x, W, None if b is None else np.asarray(b, np.float64), pad=pad, relu=relu)


def layer(W, b, x, pad=0, relu=True, rounded=True):
    """One layer of the mode on its own: the operands rounded (or not), float64 from there on."""
    if rounded:
        W, x = bf16(W), bf16(x)
    return conv_valid(x, W, b, relu, pad)


def bound(W, b, x, pad=0):
    """Per entry: (n + 2) 2^-24 (sum |a b| + |b|) over the ROUNDED operands, n = K^2 Cin -- any-order fp32
    accumulation of n exact products (n - 1 roundings), the slabs' sum and the bias (two more)."""
    n = W.shape[1] * W.shape[2] * W.shape[3]
    mag = conv_valid(np.abs(bf16(x)), np.abs(bf16(W)), None if b is None else np.abs(b), relu=False, pad=pad)
    return (n + 2) * U * mag


def pad_of(name, pad=100):
    return pad if name == 'conv1_1' else (1 if name in LAYERS[:13] else 0)


def forward(params, x, keep6=None, keep7=None, p=0.5, pad=100, rounded=False):
    """fcn8_train_ref.forward; rounded=True: W and the input of the mode's fifteen layers rounded to bf16."""
    if not rounded:
        return RF.forward(params, x, keep6, keep7, p, pad)
    inner = RF._conv
    seen = []

    def _conv(prm, name, t, pad_):
        if name in LAYERS:
            seen.append(name)
            W, b = prm[name]
            return inner({name: (bf16(W).astype(W.dtype), b)}, name, bf16(t).astype(t.dtype), pad_)
        return inner(prm, name, t, pad_)

    with _swapped(RF, '_conv', _conv):
        s = RF.forward(params, x, keep6, keep7, p, pad)
    assert tuple(seen) == LAYERS, seen
    return s


# Values exactly between two bf16 neighbours, both parities and both signs (the even neighbour is below the first
# and above the second), and values just off a tie on either side; all exact in float32.
TIES = np.array([1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 2.0 ** -7 + 2.0 ** -8),
                 1 + 2.0 ** -8 + 2.0 ** -12, 1 + 2.0 ** -8 - 2.0 ** -12, -(1 + 2.0 ** -7 + 2.0 ** -8 + 2.0 ** -12),
                 3 + 2.0 ** -7], dtype=np.float32)

# name: (Cout, Cin, K, pad, B, h, w, seed) -- reductions short enough (n = K^2 Cin <= 153) for the rounding of the
# operands, about 2^-9 sqrt(n) of a term, to stand far outside the bound, about n 2^-24 of the terms' sum
ROUNDING_CASES = {'k7_3to16_8x9': (16, 3, 7, 0, 2, 8, 9, 11), 'k1_70to33_7x7': (33, 70, 1, 0, 2, 7, 7, 12),
                  '3x3_17to33_9x33': (33, 17, 3, 1, 2, 9, 33, 13)}


def rounding_case(name):
    """(W, b, x, pad) of a seeded non-integer case, float32 values held in float64 arrays."""
    Cout, Cin, K, pad, B, h, w, seed = ROUNDING_CASES[name]
    rng = np.random.default_rng(seed)
    f = lambda a: a.astype(np.float32).astype(np.float64)
    W, b = f(rng.standard_normal((Cout, Cin, K, K))), f(rng.standard_normal(Cout))
    return W, b, f(rng.standard_normal((B, Cin, h, w))), pad
