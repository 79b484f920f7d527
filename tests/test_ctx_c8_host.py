"""CPU: the 16-bit leg of the context-module DAE (csrc/conv_c8_dil.hip, ContextModDAE(mma='bf16c8')) -- its ABI
entries check their arguments before any launch, the weight packer equals a numpy construction, the float64
restatement (tests/ctx_c8_ref.py) with rounding off is the oracle, and the driver refuses gradient mode."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import torch

import ctx_c8_ref as R8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, SHAPE, ALIGN, UNSUPPORTED = -1, -2, -3, -5
RELU, OUT_NCHW = 1, 0x100


def _desc(**kw):
    """dilconv-like 11 -> 11, 3 x 3, dilation 2 on a 44 x 40 map, dense output."""
    from iterative_inference_segm_amd import _lib
    d = _lib.C8DilDesc()
    d.B, d.Cin, d.Cout, d.H, d.W, d.K, d.dil, d.flags = 2, 11, 11, 44, 40, 3, 2, RELU
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_c8_dil_abi_status_codes_without_a_gpu(built_lib):
    from iterative_inference_segm_amd import _lib
    lib = _lib.load()
    assert lib.iiseg_abi_version() == 34 and _lib.ABI_VERSION == 34      # the additions are backward compatible
    fake = [C.c_void_p(4096 * (k + 1)) for k in range(5)]               # never dereferenced: checks come first
    ok = _desc()
    assert lib.iiseg_conv_c8_dil_check(C.byref(ok)) == 0
    assert lib.iiseg_conv_c8_dil_check(None) == NULL
    assert lib.iiseg_conv_c8_dil_pack_bytes(3) == 5 * 16 * 32 * 2 and lib.iiseg_conv_c8_dil_pack_bytes(1) == 16 * 32 * 2
    assert lib.iiseg_conv_c8_dil_pack_bytes(2) == UNSUPPORTED
    launch = lambda d, a: lib.iiseg_conv_c8_dil(None, C.byref(d) if d is not None else None, *a)
    pack = lambda d, a: lib.iiseg_conv_c8_dil_pack(None, C.byref(d) if d is not None else None, a[0], 99, 9, a[1])
    host = lambda d, a: lib.iiseg_conv_c8_dil_pack_host(C.byref(d) if d is not None else None, a[0], 99, 9, a[1])
    # null pointers: the descriptor, x8 (0), wpack (1), out (4); bias (2) and addend (3) may be NULL -- those two
    # calls would launch, so they are not made here
    assert launch(None, fake) == NULL
    for k in (0, 1, 4):
        args = list(fake)
        args[k] = None
        assert launch(ok, args) == NULL, k
    for fn in (pack, host):
        assert fn(None, fake) == NULL
        assert fn(ok, [None, fake[1]]) == NULL and fn(ok, [fake[0], None]) == NULL
    args = list(fake)
    args[1] = C.c_void_p(4096 + 8)                                      # wpack not 16-byte aligned
    assert launch(ok, args) == ALIGN and pack(ok, [fake[0], args[1]]) == ALIGN
    bads = [(dict(Cin=17), UNSUPPORTED), (dict(Cout=17), UNSUPPORTED), (dict(K=2), UNSUPPORTED),
            (dict(K=5), UNSUPPORTED), (dict(K=0), UNSUPPORTED), (dict(dil=0), UNSUPPORTED),
            (dict(dil=3), UNSUPPORTED), (dict(dil=32), UNSUPPORTED), (dict(dil=-1), UNSUPPORTED),
            (dict(flags=2), UNSUPPORTED),
            (dict(B=0), SHAPE), (dict(Cin=0), SHAPE), (dict(Cout=0), SHAPE), (dict(H=0), SHAPE), (dict(W=-4), SHAPE),
            # H <= d (K - 1) or W <= d (K - 1): no output pixel
            (dict(H=4), SHAPE), (dict(W=4), SHAPE), (dict(dil=16, H=32), SHAPE), (dict(dil=16, W=32), SHAPE),
            # a placement window that does not fit the (40, 36) map, or half a placement
            (dict(out_H=40, out_W=35), SHAPE), (dict(out_H=39, out_W=36), SHAPE),
            (dict(out_H=104, out_W=100, out_y0=65), SHAPE), (dict(out_H=104, out_W=100, out_x0=65), SHAPE),
            (dict(out_H=104, out_W=100, out_y0=-1), SHAPE), (dict(out_H=0, out_W=36), SHAPE),
            (dict(out_H=0, out_y0=1), SHAPE),
            # an image of a tensor beyond 32-bit byte offsets
            (dict(H=8192, W=8192), UNSUPPORTED), (dict(B=70000), UNSUPPORTED)]
    for bad, status in bads:
        d = _desc(**bad)
        assert lib.iiseg_conv_c8_dil_check(C.byref(d)) == status, bad
        assert launch(d, fake) == status, bad
        assert pack(d, fake) == status and host(d, fake) == status, bad
    for good in (dict(K=1, dil=1, H=1, W=1), dict(H=5, W=5), dict(dil=16, H=33, W=35), dict(Cin=1, Cout=16),
                 dict(out_H=104, out_W=100, out_y0=32, out_x0=32), dict(out_H=104, out_W=100, out_y0=64, out_x0=64),
                 dict(flags=RELU | OUT_NCHW), dict(flags=0, K=1)):
        assert lib.iiseg_conv_c8_dil_check(C.byref(_desc(**good))) == 0, good
    # strides of the packers
    for so, sc in ((0, 9), (99, 0), (-1, 9)):
        assert lib.iiseg_conv_c8_dil_pack(None, C.byref(ok), fake[0], so, sc, fake[1]) == SHAPE
        assert lib.iiseg_conv_c8_dil_pack_host(C.byref(ok), fake[0], so, sc, fake[1]) == SHAPE


def _bf16_bits(a):
    """float32 array -> uint16 bf16 patterns, round to nearest-even (numpy integer arithmetic)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _numpy_pack(W_oihw, K):
    """[m][g][co][j] = W[co][8 (g & 1) + j][tap 2 m + (g >> 1)], zero outside (include/iiseg.h)."""
    Cout, Cin = W_oihw.shape[:2]
    Wt = W_oihw.reshape(Cout, Cin, K * K)
    nm = 5 if K == 3 else 1
    img = np.zeros((nm, 4, 16, 8), dtype=np.float32)
    for m in range(nm):
        for g in range(4):
            tap = 2 * m + (g >> 1)
            if tap >= K * K:
                continue
            for j in range(8):
                ci = 8 * (g & 1) + j
                if ci < Cin:
                    img[m, g, :Cout, j] = Wt[:, ci, tap]
    return _bf16_bits(img)


def test_weight_packer_equals_a_numpy_construction(built_lib):
    from iterative_inference_segm_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(5)
    for K in (1, 3):
        for Cin, Cout in ((11, 11), (16, 16), (11, 16), (3, 5)):
            W = rng.standard_normal((Cout, Cin, K, K)).astype(np.float32)
            # values that sit exactly between two bf16 numbers: ties go to even
            W.reshape(-1)[:4] = np.array([1.00390625, 1.01171875, -1.00390625, 3.0], dtype=np.float32)
            want = _numpy_pack(W, K)
            for layout in ('oihw', 'iohw'):
                if layout == 'oihw':
                    arr, so, sc = np.ascontiguousarray(W), Cin * K * K, K * K
                else:
                    arr, so, sc = np.ascontiguousarray(W.transpose(1, 0, 2, 3)), K * K, Cout * K * K
                d = _desc(Cin=Cin, Cout=Cout, K=K, dil=1)
                got = np.zeros(want.size + 8, dtype=np.uint16)
                got[-8:] = 0xabcd                                    # the packer writes its bytes and no more
                st = lib.iiseg_conv_c8_dil_pack_host(C.byref(d), arr.ctypes.data_as(C.c_void_p), so, sc,
                                                     got.ctypes.data_as(C.c_void_p))
                assert st == 0
                assert (got[-8:] == 0xabcd).all()
                assert np.array_equal(got[:-8].reshape(want.shape), want), (K, Cin, Cout, layout)
    # the rounding is torch's (what the restatement uses)
    x = rng.standard_normal(4096).astype(np.float32)
    assert np.array_equal(_bf16_bits(x), torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))


def test_restatement_without_rounding_is_the_oracle():
    from iterative_inference_segm_amd import synthetic as S
    from oracle.contextmod import contextmod_forward
    rng = np.random.default_rng(11)
    params = {k: (W.astype(np.float64), b.astype(np.float64)) for k, (W, b) in S.make_contextmod_params().items()}
    h = rng.uniform(0, 1, (1, 3, 20, 18))
    y = rng.uniform(0, 1, (1, 11, 20, 18))
    want = contextmod_forward(params, [h], y, out_softmax=False)
    got = R8.forward(params, h, y, rounding=False)
    assert got.shape == want.shape == (1, 11, 20, 18)
    assert np.abs(got - want).max() <= 1e-12
    # ... and the rounding points do something, of the size of bf16's precision
    err = np.abs(R8.forward(params, h, y) - want).max()
    assert 1e-5 < err < 0.1


def test_driver_refuses_gradient_mode_on_the_16_bit_leg(tmp_path):
    # HIP_VISIBLE_DEVICES empty: a GPU call would fail differently; the refusal comes first
    env = dict(os.environ, HIP_VISIBLE_DEVICES='', CUDA_VISIBLE_DEVICES='')
    env.pop('IISEG_MMA', None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'iterative_inference.py'), '--synthetic', '--savepath',
                        str(tmp_path), '--update', 'gradient', '--mma', 'bf16c8'],
                       capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode != 0
    assert 'NotImplementedError' in r.stderr and 'bf16c8' in r.stderr, r.stderr
    assert not os.listdir(str(tmp_path))                       # nothing was written
