"""Float64 (torch, CPU) restatement of the context-module DAE's 16-bit leg (ContextModDAE(mma='bf16c8'),
csrc/conv_c8_dil.hip) with the kernel's rounding points:
  * weights of every C8 layer to bf16, round to nearest-even;
  * activations to bf16 (RNE) at every C8 store: y on its way in, conv1's output, dilconv1..6's outputs;
  * the image half of conv1 (W_h * h + b, a float32 map) and every bias in fp32, never in bf16;
  * the score map (dilconv7, 1 x 1) in fp32.
Sums are exact to float64 here; the kernel's differ by fp32 accumulation only.
TEST INFRASTRUCTURE: with the rounding switched off it is oracle/contextmod.py (tests/test_ctx_c8_host.py)."""
import numpy as np
import torch
import torch.nn.functional as F

DILATIONS = [1, 2, 4, 8, 16, 1]


def bf16(t):
    """float64 -> nearest bf16 (ties to even) -> float64."""
    return t.to(torch.bfloat16).to(torch.float64)


def f32(t):
    return t.to(torch.float32).to(torch.float64)


def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


def layer(x, W_oihw, b=None, add=None, dil=1, relu=False):
    """The arithmetic of one conv_c8_dil launch before its store, exact: 'valid' conv of x with W, + b, + add."""
    z = F.conv2d(x, W_oihw, None, dilation=dil)
    if b is not None:
        z = z + b.view(1, -1, 1, 1)
    if add is not None:
        z = z + add
    return torch.relu(z) if relu else z


def abs_sum(x, W_oihw, dil=1):
    """sum |w x| over the terms of every output: what the fp32 accumulation bound scales with."""
    return F.conv2d(x.abs(), W_oihw.abs(), None, dilation=dil)


def forward(params, h, y, rounding=True, layers=False):
    """Score map (B, C, H, W), float64 numpy, of the C8 module for params {name: (W, b)} in the checkpoint's
    layouts (conv1 W[out,in,3,3], dilconv* W[in,out,k,k]); h first in conv1's input channels."""
    rw = bf16 if rounding else (lambda t: t)          # C8 weights and C8 stores
    rf = f32 if rounding else (lambda t: t)           # what is kept as a float32 map
    h, y = _t(h), _t(y)
    ch = h.shape[1]
    W1, b1 = _t(params['conv1'][0]), _t(params['conv1'][1])
    hb = rf(F.conv2d(h, W1[:, :ch], b1, padding=1))                       # the image half, fp32 kernel
    t = rw(layer(F.pad(rw(y), (1, 1, 1, 1)), rw(W1[:, ch:]), None, hb, 1, True))
    outs = [t]
    t = F.pad(t, (32, 32, 32, 32))                                       # PadLayer(32)
    for i, d in enumerate(DILATIONS):
        W, b = params['dilconv%d' % (i + 1)]
        t = rw(layer(t, rw(_t(W).permute(1, 0, 2, 3)), _t(b), None, d, True))
        outs.append(t)
    W, b = params['dilconv7']
    score = rf(layer(t, rw(_t(W).permute(1, 0, 2, 3)), _t(b), None, 1, False))
    outs.append(score)
    return ([o.numpy() for o in outs] if layers else score.numpy())
