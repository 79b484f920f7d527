"""What the GPU tests of the two bf16 3x3 weight-gradient forms share (test_gpu_wgrad_bf16.py: 64 output channels per
workgroup; test_gpu_densenet_wgrad_bf16.py: 16): the numpy reference of dW, the integer cases both kernels must hit
exactly, and the bound on real data.  Plain functions; nothing here touches the GPU but `dev`."""
import numpy as np
import torch

F32 = torch.float32
U = 2.0 ** -24
_REF = {}


def dev(a, dt=F32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda().contiguous()


def taps(g, xp, OH, OW):
    """[co, ci, ky, kx] = sum_{b,y,x} g[b, co, y, x] xp[b, ci, y + ky, x + kx]"""
    return np.stack([np.stack([np.tensordot(g, xp[:, :, ky:ky + OH, kx:kx + OW], axes=([0, 2, 3], [0, 2, 3]))
                               for kx in range(3)], axis=-1) for ky in range(3)], axis=-2)


def pad(x, pad):
    return np.pad(x, ((0, 0), (0, 0), (pad, pad), (pad, pad)))


def int_case(Cin, Cout, B, H, W, pad_, dtype):
    """(x, gz, dW, db) of a layer on small integers, gz as behind a ReLU mask; dW and db summed in `dtype` (np.int64
    or np.float64: both exact) and below 2^24, so that fp32 holds every partial sum in any order.  Computed once."""
    key = (Cin, Cout, B, H, W, pad_, np.dtype(dtype).name)
    if key not in _REF:
        rng = np.random.default_rng(Cin * 1000 + Cout + 7 * B + H + 3 * pad_)
        OH, OW = H + 2 * pad_ - 2, W + 2 * pad_ - 2
        x = rng.integers(-2, 3, size=(B, Cin, H, W))
        gz = rng.integers(-2, 3, size=(B, Cout, OH, OW))
        gz[rng.integers(0, 2, size=gz.shape) == 0] = 0           # as behind a ReLU mask
        dW = taps(gz.astype(dtype), pad(x.astype(dtype), pad_), OH, OW)
        db = gz.astype(dtype).sum(axis=(0, 2, 3))
        assert dW.dtype == dtype and np.abs(dW).max() < 2 ** 24 and np.abs(db).max() < 2 ** 24
        _REF[key] = (x, gz, dW, db)
    return _REF[key]


def rounded(t):
    """float64 numpy of a float32 tensor rounded to bf16 on the CPU"""
    return t.detach().cpu().to(torch.bfloat16).double().numpy()


def bound_check(dW, x, gz, pad_, what=''):
    """dW (Cout, Cin, 3, 3) against the float64 sum over x, gz (float32 tensors) rounded to bf16 on the CPU: every
    entry within (n + 1) 2^-24 sum|a b|, the bound of n fp32 additions of exact products in ANY order, sum|a b|
    per entry from the rounded data.  Returns (worst error / bound, ref, mag)."""
    OH, OW = gz.shape[2:]
    n = gz.shape[0] * OH * OW
    g, xp = rounded(gz), pad(rounded(x), pad_)
    ref, mag = taps(g, xp, OH, OW), taps(np.abs(g), np.abs(xp), OH, OW)
    err = np.abs(dW.detach().cpu().double().numpy() - ref)
    bound = (n + 1) * U * mag
    frac = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    assert (err <= bound).all(), '%s: worst error / bound %.3g over %d terms' % (what, frac, n)
    return frac, ref, mag
