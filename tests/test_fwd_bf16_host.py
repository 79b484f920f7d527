"""CPU: the 16-bit mode of FCN-8's training forward (fwd='bf16'; include/iiseg.h iiseg_conv_fwd_kxk_bf16, kernel in
csrc/conv_kxk_bf16.hip) checks every argument before any launch; ops.conv_fwd_kxk refuses tensors and shapes it has
no kernel for before the library is called; ops.Conv, FCN8 and train_fcn8.py take the mode and refuse it, with the
reason, where nothing is built for it."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, SHAPE, ALIGN, UNSUPPORTED = -1, -2, -3, -5


def _desc(**kw):
    from iterative_inference_segm_amd import _lib
    d = _lib.ConvFwdKxKDesc()
    d.B, d.Cin, d.Cout, d.H, d.W, d.K, d.relu = 2, 24, 16, 13, 13, 7, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


BAD = [dict(K=0), dict(K=8), dict(H=6), dict(W=5), dict(B=0), dict(B=65536), dict(Cin=0), dict(Cout=65536),
       dict(relu=2), dict(relu=-1), dict(K=1, H=1 << 15, W=1 << 15)]


def test_the_library_is_still_abi_34(built_lib):
    from iterative_inference_segm_amd import _lib
    lib = _lib.load()
    assert lib.iiseg_abi_version() == _lib.ABI_VERSION == 34
    assert C.sizeof(_lib.ConvFwdKxKDesc) == 32


def test_conv_fwd_kxk_bf16_status_codes_without_a_gpu(built_lib):
    from iterative_inference_segm_amd import _lib
    lib = _lib.load()
    fake = [C.c_void_p(1 << (24 + k)) for k in range(5)]         # x, W, bias, ws, z: disjoint, never dereferenced
    assert lib.iiseg_conv_fwd_kxk_bf16_check(None) == NULL
    assert lib.iiseg_conv_fwd_kxk_bf16_slabs(None) == NULL
    assert lib.iiseg_conv_fwd_kxk_bf16_workspace_elems(None) == NULL
    assert lib.iiseg_conv_fwd_kxk_bf16(None, None, *fake) == NULL
    ok = _desc(Cin=130, Cout=65)                                 # 17 k-tiles over few tiles: several slabs
    assert lib.iiseg_conv_fwd_kxk_bf16_check(C.byref(ok)) == 0
    n = lib.iiseg_conv_fwd_kxk_bf16_slabs(C.byref(ok))
    assert n >= 2
    assert lib.iiseg_conv_fwd_kxk_bf16_workspace_elems(C.byref(ok)) == n * 2 * 65 * 7 * 7
    for k in (0, 1, 3, 4):                                       # the bias (2) may be NULL
        args = list(fake)
        args[k] = None
        assert lib.iiseg_conv_fwd_kxk_bf16(None, C.byref(ok), *args) == NULL, k
    for k in range(5):
        args = list(fake)
        args[k] = C.c_void_p(args[k].value + 2)
        assert lib.iiseg_conv_fwd_kxk_bf16(None, C.byref(ok), *args) == ALIGN, k
    for bad in BAD:
        d = _desc(**bad)
        assert lib.iiseg_conv_fwd_kxk_bf16_check(C.byref(d)) == SHAPE, bad
        assert lib.iiseg_conv_fwd_kxk_bf16_slabs(C.byref(d)) == SHAPE, bad
        assert lib.iiseg_conv_fwd_kxk_bf16_workspace_elems(C.byref(d)) == SHAPE, bad
        assert lib.iiseg_conv_fwd_kxk_bf16(None, C.byref(d), *fake) == SHAPE, bad
    # z may overlap neither x nor W: refused before any launch
    assert lib.iiseg_conv_fwd_kxk_bf16(None, C.byref(ok), fake[0], fake[1], None, fake[3], fake[0]) == UNSUPPORTED
    assert lib.iiseg_conv_fwd_kxk_bf16(None, C.byref(ok), fake[0], fake[1], None, fake[3], fake[1]) == UNSUPPORTED
    # a single slab needs no workspace: one k-tile of sixty-four channels at K = 1
    one = _desc(K=1, Cin=64, H=7, W=7)
    assert lib.iiseg_conv_fwd_kxk_bf16_slabs(C.byref(one)) == 1
    assert lib.iiseg_conv_fwd_kxk_bf16_workspace_elems(C.byref(one)) == 0
    # fc6 and fc7 of the real net at batch 10: the reduction is split, in the same way every time
    for d in (_desc(B=10, Cin=512, Cout=4096), _desc(B=10, Cin=4096, Cout=4096, K=1, H=7, W=7)):
        n = lib.iiseg_conv_fwd_kxk_bf16_slabs(C.byref(d))
        assert n >= 2 and lib.iiseg_conv_fwd_kxk_bf16_slabs(C.byref(d)) == n
        assert lib.iiseg_conv_fwd_kxk_bf16_workspace_elems(C.byref(d)) == n * 10 * 4096 * 49


def test_conv_fwd_kxk_refuses_tensors_and_shapes_before_the_library_is_called(built_lib):
    import torch
    from iterative_inference_segm_amd import ops
    assert ops.FWD_MODES == ('f32', 'bf16')
    x, W, b = torch.zeros((1, 2, 9, 9)), torch.zeros((3, 2, 7, 7)), torch.zeros(3)   # host tensors: nothing launches
    for bad in (dict(x=x.double()), dict(W=W.half()), dict(b=b.double()), dict(out=torch.zeros((1, 3, 3, 3)).double()),
                dict(x=None), dict(W=[1.0])):
        kw = dict(x=x, W=W, b=b, out=None)
        kw.update(bad)
        with pytest.raises(ValueError, match='float32'):
            ops.conv_fwd_kxk(kw['x'], kw['W'], kw['b'], out=kw['out'])
    with pytest.raises(ValueError, match='K x K'):
        ops.conv_fwd_kxk(x, torch.zeros((3, 2, 8, 8)), b)
    with pytest.raises(ValueError, match='K x K'):
        ops.conv_fwd_kxk(x, torch.zeros((3, 2, 3, 2)), b)
    with pytest.raises(ValueError, match='K x K'):
        ops.conv_fwd_kxk(x, torch.zeros((3, 2, 7)), b)
    with pytest.raises(ValueError, match='oihw'):
        ops.conv_fwd_kxk(torch.zeros((1, 3, 9, 9)), W, b)        # Cin of x and W differ
    with pytest.raises(ValueError, match='oihw'):
        ops.conv_fwd_kxk(torch.zeros((1, 2, 6, 9)), W, b)        # a plane smaller than the filter
    with pytest.raises(ValueError, match='output channels'):
        ops.conv_fwd_kxk(x, W, torch.zeros(4))
    with pytest.raises(ValueError, match='the map is'):
        ops.conv_fwd_kxk(x, W, b, out=torch.zeros((1, 3, 3, 4)))
    with pytest.raises(ValueError, match='device'):
        ops.conv_fwd_kxk(x, W, b)                                # all else right: host tensors are refused last


def test_conv_refuses_fwd16_where_it_has_no_kernel():
    import numpy as np
    import torch
    from iterative_inference_segm_amd import ops
    W3, W7 = np.zeros((4, 2, 3, 3), np.float32), np.zeros((4, 2, 7, 7), np.float32)
    for kw in (dict(W=W3, pad=1, dtype=torch.float64), dict(W=W3, pad=1, mma='bf16'), dict(W=W3, pad=1, dil=2),
               dict(W=W7, pad=1), dict(W=W7, pad=0, layout='iohw'), dict(W=np.zeros((4, 2, 8, 8), np.float32), pad=0)):
        kw = dict(dict(dtype=torch.float32, mma='f32'), **kw)
        with pytest.raises(NotImplementedError, match='fwd16'):
            ops.Conv(kw.pop('W'), None, relu=True, device='cpu', fwd16=True, **kw)
    conv = ops.Conv(W3, None, pad=1, relu=True, device='cpu', dtype=torch.float32, mma='f32')
    assert conv.fwd16 is False


def test_fcn8_refuses_fwd_bf16_where_it_has_no_meaning():
    """When the module is built, before any device work (the arguments are checked first)."""
    import torch
    from iterative_inference_segm_amd.fcn8 import FCN8
    for kw in (dict(trainable=True, dtype=torch.float64), dict(trainable=False, dtype=torch.float32)):
        with pytest.raises(NotImplementedError, match="fwd='bf16'"):
            FCN8({}, 11, device='cpu', fwd='bf16', **kw)
    with pytest.raises(ValueError, match='fwd'):
        FCN8({}, 11, device='cpu', trainable=True, fwd='fp8')
    # mma= on a trainable module keeps its refusal: the mode is a keyword of its own
    with pytest.raises(NotImplementedError, match='16-bit legs'):
        FCN8({}, 11, device='cpu', trainable=True, mma='bf16', fwd='bf16')


def test_check_fwd_is_the_twin_of_check_kxk():
    from iterative_inference_segm_amd import train
    train.check_fwd('f32', 'float64')
    train.check_fwd('bf16', 'float32')
    with pytest.raises(NotImplementedError, match="fwd='bf16'.*float32"):
        train.check_fwd('bf16', 'float64')
    with pytest.raises(ValueError, match='fwd'):
        train.check_fwd('fp8', 'float32')


def test_parse_args_of_train_fcn8_accepts_fwd_and_train_dae_has_no_such_flag():
    sys.path.insert(0, ROOT)
    try:
        import train_dae
        import train_fcn8
    finally:
        sys.path.remove(ROOT)
    assert train_fcn8.parse_args(['--savepath', 'x']).fwd == 'f32'
    a = train_fcn8.parse_args(['--savepath', 'x', '--fwd', 'bf16'])
    assert (a.fwd, a.wgrad, a.dgrad, a.kxk) == ('bf16', 'f32', 'f32', 'f32')   # independent of the other three modes
    with pytest.raises(SystemExit):
        train_fcn8.parse_args(['--savepath', 'x', '--fwd', 'fp8'])
    with pytest.raises(SystemExit):
        train_dae.parse_args(['--fwd', 'bf16'])


def test_train_fcn8_refuses_fwd_bf16_in_float64_with_status_2_before_any_gpu_work(tmp_path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES='', CUDA_VISIBLE_DEVICES='')    # no device to touch
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_fcn8.py'), '--synthetic', '--savepath',
                        str(tmp_path / 's'), '--fwd', 'bf16', '--dtype', 'float64'],
                       capture_output=True, text=True, cwd=ROOT, env=env)
    assert r.returncode == 2, r.stdout[-1000:] + r.stderr[-1000:]
    assert "fwd='bf16'" in r.stderr and 'float32' in r.stderr, r.stderr
    assert 'Traceback' not in r.stderr
    assert not os.path.exists(str(tmp_path / 's'))               # nothing was made
