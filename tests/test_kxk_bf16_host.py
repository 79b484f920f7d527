"""CPU: the 16-bit mode of FCN-8's fc6 / fc7 gradients (kxk='bf16'; include/iiseg.h iiseg_conv_wgrad_kxk_bf16 and
iiseg_conv_dgrad_kxk_bf16, kernels in csrc/conv_kxk_bf16.hip) checks every argument before any launch; the two ops
refuse modes, tensors and shapes they have no kernel for before the library is called; FCN8 and train_fcn8.py take
the mode and refuse it, with the reason, where nothing is built for it."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, SHAPE, ALIGN, UNSUPPORTED = -1, -2, -3, -5


def _wdesc(**kw):
    from iterative_inference_segm_amd import _lib
    d = _lib.ConvWgradKxKDesc()
    d.B, d.Cin, d.Cout, d.H, d.W, d.K = 2, 24, 16, 13, 13, 7
    for k, v in kw.items():
        setattr(d, k, v)
    if 'Cin_tot' not in kw:
        d.Cin_tot = d.ci0 + d.Cin
    if 'x_row' not in kw:
        d.x_row, d.x_plane, d.x_image = d.W, d.H * d.W, d.Cin * d.H * d.W
    if 'so' not in kw:
        d.so, d.sc = d.Cin_tot * d.K * d.K, d.K * d.K
    return d


def _ddesc(**kw):
    from iterative_inference_segm_amd import _lib
    d = _lib.ConvDgradDesc()
    d.B, d.Cin, d.Cout, d.H, d.W, d.K, d.pad = 2, 24, 16, 7, 7, 7, 6
    for k, v in kw.items():
        setattr(d, k, v)
    if 'Cin_tot' not in kw:
        d.Cin_tot = d.ci0 + d.Cin
    if 'so' not in kw:
        d.so, d.sc = d.Cin_tot * d.K * d.K, d.K * d.K
    return d


WBAD = [dict(K=0), dict(K=8), dict(H=6), dict(W=5), dict(B=0), dict(Cin=0), dict(Cout=65536), dict(ci0=-1),
        dict(ci0=1, Cin_tot=24), dict(so=7, sc=49), dict(x_row=12, x_plane=169, x_image=24 * 169), dict(x_y0=-1)]
DBAD = [dict(K=0), dict(K=8), dict(H=0), dict(W=-1), dict(B=0), dict(Cin=0), dict(Cout=65536), dict(ci0=-1),
        dict(ci0=1, Cin_tot=24), dict(so=7, sc=49), dict(accumulate=2), dict(H=1 << 15, W=1 << 15)]


def test_the_library_is_an_abi_34_addition(built_lib):
    from iterative_inference_segm_amd import _lib, build
    lib = _lib.load()
    assert 'conv_kxk_bf16.hip' in build.SOURCES
    assert lib.iiseg_abi_version() == _lib.ABI_VERSION == 34


def test_conv_wgrad_kxk_bf16_status_codes_without_a_gpu(built_lib):
    from iterative_inference_segm_amd import _lib
    lib = _lib.load()
    fake = [C.c_void_p(4096 * (k + 1)) for k in range(5)]        # never dereferenced: a refused call launches nothing
    assert lib.iiseg_conv_wgrad_kxk_bf16_check(None) == NULL
    assert lib.iiseg_conv_wgrad_kxk_bf16_slabs(None) == NULL
    assert lib.iiseg_conv_wgrad_kxk_bf16_workspace_elems(None) == NULL
    assert lib.iiseg_conv_wgrad_kxk_bf16(None, None, *fake) == NULL
    ok = _wdesc(K=1, H=37, W=150, B=3)                           # several slabs: the workspace is required
    n = lib.iiseg_conv_wgrad_kxk_bf16_slabs(C.byref(ok))
    assert n >= 2
    assert lib.iiseg_conv_wgrad_kxk_bf16_workspace_elems(C.byref(ok)) == n * (16 * 24 + 16)
    for k in (0, 1, 2, 3):                                       # db (4) may be NULL
        args = list(fake)
        args[k] = None
        assert lib.iiseg_conv_wgrad_kxk_bf16(None, C.byref(ok), *args) == NULL, k
    for bad in WBAD:
        d = _wdesc(**bad)
        assert lib.iiseg_conv_wgrad_kxk_bf16_check(C.byref(d)) == SHAPE, bad
        assert lib.iiseg_conv_wgrad_kxk_bf16(None, C.byref(d), *fake) == SHAPE, bad
        assert lib.iiseg_conv_wgrad_kxk_check(C.byref(d)) == SHAPE, bad          # the code of the float32 entry
    # fc6 and fc7 of the real net at batch 10: one slab, straight into dW
    fc6 = _wdesc(B=10, Cin=512, Cout=4096)
    fc7 = _wdesc(B=10, Cin=4096, Cout=4096, K=1, H=1, W=1)
    for d in (fc6, fc7):
        assert lib.iiseg_conv_wgrad_kxk_bf16_slabs(C.byref(d)) == 1
        assert lib.iiseg_conv_wgrad_kxk_bf16_workspace_elems(C.byref(d)) == 0
    assert lib.iiseg_conv_wgrad_kxk_bf16(None, C.byref(fc6), C.c_void_p(4098), *fake[1:]) == ALIGN


def test_conv_dgrad_kxk_bf16_status_codes_without_a_gpu(built_lib):
    from iterative_inference_segm_amd import _lib
    lib = _lib.load()
    fake = [C.c_void_p(1 << (20 + k)) for k in range(5)]         # gz, packed, gate, ws, gx: disjoint, never dereferenced
    assert lib.iiseg_conv_dgrad_kxk_bf16_check(None) == NULL
    assert lib.iiseg_conv_dgrad_kxk_bf16_pack_elems(None) == NULL
    assert lib.iiseg_conv_dgrad_kxk_bf16_workspace_elems(None) == NULL
    assert lib.iiseg_conv_dgrad_kxk_bf16(None, None, *fake) == NULL
    ok = _ddesc(Cin=33, Cout=130)                                # 9 k-tiles over few tiles: several slabs
    n = lib.iiseg_conv_dgrad_kxk_bf16_slabs(C.byref(ok))
    assert n >= 2
    assert lib.iiseg_conv_dgrad_kxk_bf16_workspace_elems(C.byref(ok)) == n * 2 * 33 * 13 * 13
    # [9 k-tiles][49 taps][16 co][64 ci]
    assert lib.iiseg_conv_dgrad_kxk_bf16_pack_elems(C.byref(ok)) == 9 * 49 * 16 * 64
    for k in (0, 1, 3, 4):                                       # the gate (2) may be NULL
        args = list(fake)
        args[k] = None
        assert lib.iiseg_conv_dgrad_kxk_bf16(None, C.byref(ok), *args) == NULL, k
    assert lib.iiseg_conv_dgrad_kxk_bf16_pack(None, C.byref(ok), None, fake[1]) == NULL
    assert lib.iiseg_conv_dgrad_kxk_bf16_pack(None, C.byref(ok), fake[0], C.c_void_p((1 << 21) + 8)) == ALIGN
    for bad in DBAD:
        d = _ddesc(**bad)
        assert lib.iiseg_conv_dgrad_kxk_bf16_check(C.byref(d)) == SHAPE, bad
        assert lib.iiseg_conv_dgrad_kxk_bf16_pack_elems(C.byref(d)) == SHAPE, bad
        assert lib.iiseg_conv_dgrad_kxk_bf16(None, C.byref(d), *fake) == SHAPE, bad
    # gx may not overlap gz: refused before any launch
    one = _ddesc(Cout=16, B=1)
    assert lib.iiseg_conv_dgrad_kxk_bf16(None, C.byref(one), fake[0], fake[1], None, fake[3], fake[0]) == UNSUPPORTED
    assert lib.iiseg_conv_dgrad_kxk_bf16(None, C.byref(one), fake[0], fake[1], None, fake[3], fake[1]) == UNSUPPORTED


def test_ops_refuse_modes_tensors_and_shapes_before_the_library_is_called(built_lib):
    import torch
    from iterative_inference_segm_amd import ops
    assert ops.KXK_MODES == ('f32', 'bf16')
    x, gz = torch.zeros((1, 2, 9, 9)), torch.zeros((1, 3, 3, 3))          # host tensors: nothing may reach a launch
    dW, db = torch.zeros((3, 2, 7, 7)), torch.zeros(3)
    for mma in ('fp8', 'bf16c8', 'f64', None, ''):
        with pytest.raises(ValueError, match='mma'):
            ops.conv_wgrad_kxk(x, gz, dW, db, mma=mma)
    with pytest.raises(ValueError, match='float32'):
        ops.conv_wgrad_kxk(x.double(), gz.double(), dW.double(), db.double(), mma='bf16')
    with pytest.raises(ValueError, match='float32'):
        ops.conv_wgrad_kxk(x, gz, dW.double(), None, mma='bf16')
    with pytest.raises(ValueError, match='shapes'):
        ops.conv_wgrad_kxk(x, torch.zeros((1, 3, 4, 3)), dW, db, mma='bf16')
    with pytest.raises(ValueError, match='shapes'):
        ops.conv_wgrad_kxk(x, gz, dW, torch.zeros(4), mma='bf16')
    with pytest.raises(ValueError, match='shapes'):
        ops.conv_wgrad_kxk(x, gz, dW, db, ci0=1, mma='bf16')
    with pytest.raises(ValueError, match='K x K'):
        ops.conv_wgrad_kxk(x, gz, torch.zeros((3, 2, 8, 8)), db, mma='bf16')
    with pytest.raises(ValueError, match='layout'):
        ops.conv_wgrad_kxk(x, gz, dW, db, layout='hwio', mma='bf16')
    with pytest.raises(ValueError, match='device'):
        ops.conv_wgrad_kxk(x, gz, dW, db, mma='bf16')            # all else right: host tensors are refused last

    W = torch.zeros((3, 2, 7, 7))
    with pytest.raises(ValueError, match='float32'):
        ops.conv_dgrad_kxk(gz.double(), W)
    with pytest.raises(ValueError, match='float32'):
        ops.conv_dgrad_kxk(gz, W.half())
    with pytest.raises(ValueError, match='K x K'):
        ops.conv_dgrad_kxk(gz, torch.zeros((3, 2, 8, 8)))
    with pytest.raises(ValueError, match='K x K'):
        ops.conv_dgrad_kxk(gz, torch.zeros((3, 2, 3, 2)))
    with pytest.raises(ValueError, match='layout'):
        ops.conv_dgrad_kxk(gz, W, layout='hwio')
    with pytest.raises(ValueError, match='input channels'):
        ops.conv_dgrad_kxk(torch.zeros((1, 4, 3, 3)), W)         # Cout of gz and W differ
    with pytest.raises(ValueError, match='input channels'):
        ops.conv_dgrad_kxk(gz, W, ci0=1, cin=2)
    with pytest.raises(ValueError, match='accumulate'):
        ops.conv_dgrad_kxk(gz, W, accumulate=True)
    with pytest.raises(ValueError, match='the gradient is'):
        ops.conv_dgrad_kxk(gz, W, out=torch.zeros((1, 2, 8, 9)))
    with pytest.raises(ValueError, match='the gradient is'):
        ops.conv_dgrad_kxk(gz, W, gate=torch.zeros((1, 2, 3, 3)))
    with pytest.raises(ValueError, match='packed'):
        ops.conv_dgrad_kxk(gz, W, packed=torch.zeros(8))
    with pytest.raises(ValueError, match='float32'):
        ops.conv_dgrad_kxk_pack(W.double(), (1, 3, 3, 3))


def test_fcn8_refuses_kxk_bf16_where_it_has_no_meaning():
    """When the module is built, before any device work (the arguments are checked first)."""
    import torch
    from iterative_inference_segm_amd.fcn8 import FCN8
    for kw in (dict(trainable=True, dtype=torch.float64), dict(trainable=False, dtype=torch.float32)):
        with pytest.raises(NotImplementedError, match="kxk='bf16'"):
            FCN8({}, 11, device='cpu', kxk='bf16', **kw)
    with pytest.raises(ValueError, match='kxk'):
        FCN8({}, 11, device='cpu', trainable=True, kxk='fp8')


def test_check_kxk_is_the_twin_of_check_wgrad():
    from iterative_inference_segm_amd import train
    train.check_kxk('f32', 'float64')
    train.check_kxk('bf16', 'float32')
    with pytest.raises(NotImplementedError, match="kxk='bf16'.*float32"):
        train.check_kxk('bf16', 'float64')
    with pytest.raises(ValueError, match='kxk'):
        train.check_kxk('fp8', 'float32')


def test_parse_args_of_train_fcn8_accepts_kxk_and_train_dae_has_no_such_flag():
    sys.path.insert(0, ROOT)
    try:
        import train_dae
        import train_fcn8
    finally:
        sys.path.remove(ROOT)
    assert train_fcn8.parse_args(['--savepath', 'x']).kxk == 'f32'
    a = train_fcn8.parse_args(['--savepath', 'x', '--kxk', 'bf16'])
    assert (a.kxk, a.wgrad, a.dgrad) == ('bf16', 'f32', 'f32')   # independent of the other two modes
    with pytest.raises(SystemExit):
        train_fcn8.parse_args(['--savepath', 'x', '--kxk', 'fp8'])
    with pytest.raises(SystemExit):
        train_dae.parse_args(['--kxk', 'bf16'])


def test_train_fcn8_refuses_kxk_bf16_in_float64_with_status_2_before_any_gpu_work(tmp_path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES='', CUDA_VISIBLE_DEVICES='')    # no device to touch
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_fcn8.py'), '--synthetic', '--savepath',
                        str(tmp_path / 's'), '--kxk', 'bf16', '--dtype', 'float64'],
                       capture_output=True, text=True, cwd=ROOT, env=env)
    assert r.returncode == 2, r.stdout[-1000:] + r.stderr[-1000:]
    assert "kxk='bf16'" in r.stderr and 'float32' in r.stderr, r.stderr
    assert 'Traceback' not in r.stderr
    assert not os.path.exists(str(tmp_path / 's'))               # nothing was made
