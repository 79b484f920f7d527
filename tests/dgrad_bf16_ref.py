"""Float64 (numpy) restatement of both backward chains with the rounding points of dgrad='bf16' (DESIGN.md section
16): tests/std_train_ref.backward and tests/fcn8_train_ref.backward themselves, with the function each of them
forms its data gradients with (a module-level name in both) replaced, for the duration of the call, by one that
first rounds W and g_z of a 3x3 layer to bf16 (to nearest, ties to even).  With rounding off the two functions are
called as they stand.  TEST INFRASTRUCTURE: pinned by tests/test_dgrad_bf16_ref.py; the HIP path's chain error is
checked against it (tests/test_gpu_dgrad_bf16.py).
"""
import contextlib

import numpy as np
import torch

import fcn8_train_ref as RF
import std_train_ref as R


def bf16(a):
    """`a` rounded to float32 and then to bf16 (nearest, ties to even: torch on the CPU), as float64."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64).numpy()


def rounding(inner):
    """`inner(gz, W, pad, in_hw)` on the rounded operands of a 3x3 layer; other layers as they are."""
    def conv_bwd_data(gz, W, pad, in_hw):
        if tuple(W.shape[2:]) == (3, 3):
            gz, W = bf16(gz).astype(gz.dtype), bf16(W).astype(W.dtype)
        return inner(gz, W, pad, in_hw)
    return conv_bwd_data


@contextlib.contextmanager
def _swapped(module, name, fn):
    old = getattr(module, name)
    setattr(module, name, fn)
    try:
        yield
    finally:
        setattr(module, name, old)


def std_backward(params, h_list, saved, g_score, cfg, rounded=False):
    """std_train_ref.backward; rounded=True: W and g_z rounded at every data gradient it forms (all 3x3)."""
    if not rounded:
        return R.backward(params, h_list, saved, g_score, cfg)
    with _swapped(R, '_conv_bwd_data', rounding(R._conv_bwd_data)):
        return R.backward(params, h_list, saved, g_score, cfg)


def fcn8_backward(params, s, g_score, rounded=False):
    """fcn8_train_ref.backward; rounded=True: W and g_z rounded at the twelve 3x3 data gradients (fc6, fc7 and the
    1x1 layers go through the same function and are left alone)."""
    if not rounded:
        return RF.backward(params, s, g_score)
    with _swapped(RF, 'conv_bwd_data', rounding(RF.conv_bwd_data)):
        return RF.backward(params, s, g_score)


def cosines(a, b):
    """{name: cosine of (dW, db) of a to those of b}"""
    cat = lambda v: np.concatenate([np.asarray(t, np.float64).ravel() for t in v])
    return {n: float(cat(a[n]) @ cat(b[n]) / (np.linalg.norm(cat(a[n])) * np.linalg.norm(cat(b[n])))) for n in a}
