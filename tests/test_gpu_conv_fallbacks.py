"""GPU: the fp32 kernels every layer lands on that a specialised form refuses -- the table-driven gather
(conv_igemm_f32_kernel), the static-tap kernel (conv_taps_f32_kernel) and the im2col + split-K GEMM
(iiseg_conv_gemm_f32) -- against the float64 oracle, at shapes of their own.

Every case (tests/conv_fallback_cases.py; test_host_conv_dispatch.py holds the same table on the host)
  * asserts the kernel that runs it, from the library's own dispatch (iiseg_conv_direct_kernel; the GEMM
    form: `Conv._form` and S from the workspace size), so that a dispatch change cannot empty it silently;
  * is EQUAL to the oracle on integer data: x in [-3, 3], w in [-2, 2], bias in [-4, 4], skip-add in
    [-5, 5]; every product and every partial sum is an integer below 6 * 2352 + 9 < 2^24, exact in fp32
    in any order;
  * is within `conv_tol` (test_gpu_ops.py) of the oracle on seeded normal data;
  * writes into a larger tensor filled with a sentinel and leaves everything outside its window alone."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_fallback_cases as K
from oracle import nn as onn
from test_gpu_ops import conv_tol

pytestmark = pytest.mark.gpu

SENTINEL = -77.0
GUARD = 4096           # floats on either side of a dense output ('guard' placement)


@pytest.fixture(scope='module')
def ops(built_lib):
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from iterative_inference_segm_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _data(c, g, rng, integer):
    """Operands of a case (float32 values in float64 arrays) and its layer's parameters."""
    K_ = (c.C1 + c.C2) * c.k * c.k
    wshape = (c.C1 + c.C2, c.Cout, c.k, c.k) if c.transposed else (c.Cout, c.C1 + c.C2, c.k, c.k)
    if integer:
        draw = lambda lim, shape: rng.integers(-lim, lim + 1, size=shape).astype(np.float64)
        w, b = draw(2, wshape), draw(4, c.Cout)
    else:
        draw = lambda lim, shape: rng.standard_normal(shape).astype(np.float32).astype(np.float64)
        w = (draw(0, wshape) / np.sqrt(K_)).astype(np.float32).astype(np.float64)
        b = draw(0, c.Cout)
    t = {'x1': draw(3, g['x1'])}
    if c.C2:
        t['x2'] = draw(3, g['x2'])
    if c.unpool:
        # post-ReLU pre-pool map: exact-zero ties everywhere, and one constant (all-tie) window
        pre = np.maximum(draw(3, g['pre']), 0)
        pre[:, :, :2, :2] = 2.0 if integer else 0.75
        t['pre'], t['pooled'] = pre, onn.maxpool2(pre)
    if c.add:
        t['add'] = draw(5, g['add'])
    return w, b, t


def _reference(c, g, w, b, t):
    """float64: the layer on its whole map, then window, skip-add from its own offset, ReLU."""
    if c.transposed:
        full = onn.deconv2d(t['x1'], w, b, stride=2)
    else:
        x = t['x1']
        if c.unpool:
            x = onn.depool_eqmask(x, t['pre'], t['pooled'])
        if c.C2:
            x = onn.concat_h_first(x, t['x2'])
        full = onn.conv2d(x, w, b, pad=c.pad, dilation=c.dil)
    y0, x0, oh, ow = g['win']
    ref = full[:, :, y0:y0 + oh, x0:x0 + ow]
    if c.add:
        ay, ax = g['add_off']
        ref = ref + t['add'][:, :, ay:ay + oh, ax:ax + ow]
    return np.maximum(ref, 0) if c.relu else ref


def _layer(ops, c, w, b):
    conv = ops.Conv(w, b, pad=c.pad, relu=c.relu, dil=c.dil, layout='iohw' if c.transposed else 'oihw',
                    transposed=c.transposed, mma='f32')
    conv.wino = False
    return conv


def _split_k(conv, d):
    T = d.B * d.OH * d.OW
    Tpad = (T + 127) // 128 * 128
    per_pixel, rem = divmod(conv.lib.iiseg_conv_gemm_workspace_elems(C.byref(d)), Tpad)
    S, rem2 = divmod(per_pixel - d.Kpad, d.Mpad)
    assert rem == 0 and rem2 == 0
    return S


def _assert_route(conv, c, x1, kw):
    launch = conv._describe_call(x1, **kw)
    tiles = (C.c_int32 * 4)()
    family = conv.lib.iiseg_conv_direct_kernel(C.byref(launch.d), int(launch.add is not None),
                                               int(conv.b is not None), tiles)
    assert c.route is None or (family,) + tuple(tiles) == c.route
    if c.S is None:
        assert conv._form(launch) == 'direct'
    else:
        assert conv._form(launch) == 'gemm_f32' and _split_k(conv, launch.d) == c.S


def _run(conv, c, g, t, placed):
    """One launch of the case with the placement `placed`: (its window of the output, everything else of the
    tensor it wrote into)."""
    geo = K.geometry(c, placed if placed != 'guard' else None)
    B, (oh, ow) = c.B, g['win'][2:]
    flat = None
    if placed == 'guard':
        n = B * c.Cout * oh * ow
        flat = torch.full((n + 2 * GUARD,), SENTINEL, device='cuda')
        geo['out'] = (B, c.Cout, oh, ow)
    tensors = {k: dev(v) for k, v in t.items()}
    x1 = tensors.pop('x1')

    def tensor(name, shape):
        if name != 'out':
            return tensors[name]
        if flat is not None:
            return flat[GUARD:GUARD + n].view(shape)
        return torch.full(shape, SENTINEL, device='cuda')
    kw = K.call_kwargs(geo, tensor)
    _assert_route(conv, c, x1, kw)
    out = conv(x1, **kw)
    if placed is None:
        return host(out), None
    if placed == 'guard':
        whole = host(flat)
        return whole[GUARD:GUARD + n].reshape(B, c.Cout, oh, ow), np.concatenate([whole[:GUARD], whole[GUARD + n:]])
    whole = host(kw['out'])
    c0 = geo['out_c0'] or 0
    py, px = geo['place']
    window = (slice(None), slice(c0, c0 + c.Cout), slice(py, py + oh), slice(px, px + ow))
    got = whole[window].copy()
    whole[window] = SENTINEL
    return got, whole


def _seed(c):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(c.name))


@pytest.mark.parametrize('c', K.FALLBACK_CASES, ids=lambda c: c.name)
def test_fallback_kernel_matches_the_oracle(ops, c):
    if K.switched_off(c):
        pytest.skip('%s is not at its default' % K.switched_off(c))
    rng = np.random.default_rng(_seed(c))
    g = K.geometry(c, c.placed if c.placed != 'guard' else None)
    depth = (c.C1 + c.C2) * c.k * c.k
    # integer data: equal to the oracle, dense and placed; nothing outside the window is written
    w, b, t = _data(c, g, rng, integer=True)
    ref = _reference(c, g, w, b, t)
    assert np.abs(ref).max() < 2 ** 24
    conv = _layer(ops, c, w, b)
    for placed in (None, c.placed):
        got, rest = _run(conv, c, g, t, placed)
        assert got.shape == ref.shape and np.array_equal(got, ref.astype(np.float32)), placed
        assert rest is None or np.all(rest == SENTINEL), 'wrote outside the %s window' % placed
    # random data: fp32 chains against float64, the bound of test_gpu_ops.py
    w, b, t = _data(c, g, rng, integer=False)
    ref = _reference(c, g, w, b, t)
    conv = _layer(ops, c, w, b)
    got, rest = _run(conv, c, g, t, c.placed)
    err = np.abs(got - ref).max()
    print('%s: max |err| %.3e, conv_tol %.3e' % (c.name, err, conv_tol(ref, depth)))
    assert err <= conv_tol(ref, depth)
    assert np.all(rest == SENTINEL)
    if c.S is not None and c.S > 1:
        # `gemm_conv_geom`: S, and with it the order of an image's K sum, does not depend on the batch
        one = c._replace(B=1, route=None)        # (fewer pixel tiles; the form and S are asserted again)
        alone, _ = _run(conv, one, K.geometry(one), {k: v[:1] for k, v in t.items()}, None)
        assert np.array_equal(alone[0], got[0])
