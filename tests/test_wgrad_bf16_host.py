"""CPU: the 16-bit weight-gradient mode (wgrad='bf16'; include/iiseg.h iiseg_conv_wgrad_bf16, kernel in
csrc/conv_wgrad_bf16.hip) checks every argument before any launch, its slab / workspace queries refuse what the
float32 ones refuse, ops.conv_wgrad refuses modes and tensors it has no kernel for, and both training drivers take
`--wgrad` and refuse it, with the reason, where nothing is built for it."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, SHAPE = -1, -2


def _desc(**kw):
    from iterative_inference_segm_amd import _lib
    d = _lib.ConvWgradDesc()
    d.B, d.Cin, d.Cout, d.H, d.W, d.K, d.pad = 2, 24, 16, 14, 13, 3, 1
    d.ci0 = 0
    for k, v in kw.items():
        setattr(d, k, v)
    if 'Cin_tot' not in kw:
        d.Cin_tot = d.ci0 + d.Cin
    if 'so' not in kw:
        d.so, d.sc = d.Cin_tot * 9, 9
    return d


# K != 3; ci0 + Cin > Cin_tot; strides that are neither layout; and the rest of the descriptor's limits
BAD = [dict(K=1), dict(K=2), dict(K=5), dict(K=0),
       dict(ci0=1, Cin_tot=24), dict(Cin_tot=23), dict(ci0=-1), dict(Cin_tot=0),
       dict(so=7, sc=9), dict(so=24 * 9, sc=8), dict(ci0=3, Cin_tot=30, so=24 * 9, sc=9), dict(so=9, sc=15 * 9),
       dict(B=0), dict(B=65536), dict(Cin=0), dict(Cout=0), dict(Cout=65536), dict(H=0), dict(W=-2), dict(pad=-1),
       dict(H=1, W=1, pad=0), dict(H=1 << 16, W=1 << 15), dict(Cin=30000, Cout=30000, Cin_tot=30000)]
GOOD = [dict(), dict(pad=0), dict(pad=100), dict(pad=5, H=3, W=4), dict(ci0=3, Cin_tot=40), dict(so=9, sc=16 * 9),
        dict(ci0=5, Cin_tot=29, so=9, sc=16 * 9), dict(Cin=1024, Cout=2048, H=7, W=7, B=10),
        dict(Cin=11, Cout=64, H=224, W=224, pad=100, B=10), dict(Cin=3, Cout=64, H=224, W=224, pad=100),
        dict(H=1, W=1)]


def test_conv_wgrad_bf16_status_codes_without_a_gpu(built_lib):
    from iterative_inference_segm_amd import _lib, build
    lib = _lib.load()
    assert 'conv_wgrad_bf16.hip' in build.SOURCES
    assert lib.iiseg_abi_version() == _lib.ABI_VERSION           # a backward-compatible addition
    fake = [C.c_void_p(4096 * (k + 1)) for k in range(5)]        # never dereferenced: a refused call launches nothing
    assert lib.iiseg_conv_wgrad_bf16_slabs(None) == NULL
    assert lib.iiseg_conv_wgrad_bf16_workspace_elems(None) == NULL
    assert lib.iiseg_conv_wgrad_bf16(None, None, *fake) == NULL
    ok = _desc(H=37, W=150)                                      # several slabs: the workspace is required
    assert lib.iiseg_conv_wgrad_bf16_slabs(C.byref(ok)) >= 2
    for k in (0, 1, 2, 3):                                       # db (4) may be NULL
        args = list(fake)
        args[k] = None
        assert lib.iiseg_conv_wgrad_bf16(None, C.byref(ok), *args) == NULL, k
    for bad in BAD:
        d = _desc(**bad)
        assert lib.iiseg_conv_wgrad_bf16(None, C.byref(d), *fake) == SHAPE, bad
        # the same codes as the float32 queries
        assert lib.iiseg_conv_wgrad_bf16_slabs(C.byref(d)) == lib.iiseg_conv_wgrad_slabs(C.byref(d), 4) == SHAPE, bad
        assert lib.iiseg_conv_wgrad_bf16_workspace_elems(C.byref(d)) == \
            lib.iiseg_conv_wgrad_workspace_elems(C.byref(d), 4) == SHAPE, bad
    # the checks come in the fp32 entry's order: the descriptor first, then the pointers
    assert lib.iiseg_conv_wgrad_bf16(None, C.byref(_desc(K=5)), None, None, None, None, None) == SHAPE


def test_conv_wgrad_bf16_workspace_is_what_the_launch_requires(built_lib):
    from iterative_inference_segm_amd import _lib
    lib = _lib.load()
    fake = [C.c_void_p(4096 * (k + 1)) for k in range(5)]
    for good in GOOD:
        d = _desc(**good)
        n = lib.iiseg_conv_wgrad_bf16_slabs(C.byref(d))
        ws = lib.iiseg_conv_wgrad_bf16_workspace_elems(C.byref(d))
        assert n >= 1, good
        assert ws == (0 if n == 1 else n * (d.Cout * d.Cin * 9 + d.Cout)), good
        if n > 1:                                                # without its workspace such a call is refused
            assert lib.iiseg_conv_wgrad_bf16(None, C.byref(d), fake[0], fake[1], None, fake[3], fake[4]) == NULL, good
    assert lib.iiseg_conv_wgrad_bf16_slabs(C.byref(_desc(H=7, W=7, B=1))) == 1
    assert lib.iiseg_conv_wgrad_bf16_slabs(C.byref(_desc(Cin=1024, Cout=2048, H=7, W=7, B=10))) == 1
    assert lib.iiseg_conv_wgrad_bf16_slabs(C.byref(_desc(Cin=11, Cout=64, H=224, W=224, pad=100, B=10))) >= 128


def test_ops_conv_wgrad_refuses_modes_and_tensors_before_any_launch(built_lib):
    import torch
    from iterative_inference_segm_amd import ops
    x, gz = torch.zeros((1, 2, 4, 4)), torch.zeros((1, 3, 4, 4))           # host tensors: nothing may reach a launch
    dW, db = torch.zeros((3, 2, 3, 3)), torch.zeros(3)
    for mma in ('fp8', 'bf16c8', 'f64', None, ''):
        with pytest.raises(ValueError, match='mma'):
            ops.conv_wgrad(x, gz, dW, db, pad=1, mma=mma)
    with pytest.raises(ValueError, match='float32'):
        ops.conv_wgrad(x.double(), gz.double(), dW.double(), db.double(), pad=1, mma='bf16')
    with pytest.raises(ValueError, match='float32'):
        ops.conv_wgrad(x, gz, dW.double(), None, pad=1, mma='bf16')
    assert ops.WGRAD_MODES == ('f32', 'bf16')


def test_modules_refuse_wgrad_bf16_where_it_has_no_meaning():
    """When the module is built, before any device work (the arguments are checked first)."""
    import torch
    from iterative_inference_segm_amd.dae import StandardDAE
    from iterative_inference_segm_amd.fcn8 import FCN8
    for kw in (dict(trainable=True, dtype=torch.float64), dict(trainable=False, dtype=torch.float32)):
        with pytest.raises(NotImplementedError, match="wgrad='bf16'"):
            StandardDAE({}, 11, concat_h=['pool4'], device='cpu', wgrad='bf16', **kw)
        with pytest.raises(NotImplementedError, match="wgrad='bf16'"):
            FCN8({}, 11, device='cpu', wgrad='bf16', **kw)
    with pytest.raises(ValueError, match='wgrad'):
        StandardDAE({}, 11, concat_h=['pool4'], device='cpu', trainable=True, wgrad='fp8')
    with pytest.raises(ValueError, match='wgrad'):
        FCN8({}, 11, device='cpu', trainable=True, wgrad='fp8')


def test_parse_args_of_both_drivers_accepts_wgrad():
    sys.path.insert(0, ROOT)
    try:
        import train_dae
        import train_fcn8
    finally:
        sys.path.remove(ROOT)
    assert train_dae.parse_args([])[0].wgrad == 'f32'
    assert train_dae.parse_args(['--wgrad', 'bf16'])[0].wgrad == 'bf16'
    assert train_fcn8.parse_args(['--savepath', 'x']).wgrad == 'f32'
    assert train_fcn8.parse_args(['--savepath', 'x', '--wgrad', 'bf16']).wgrad == 'bf16'
    for mod in (train_dae, train_fcn8):
        with pytest.raises(SystemExit):
            mod.parse_args(['--wgrad', 'fp8'])


STANDARD = '{"kind": "standard", "concat_h": ["pool4"]}'


@pytest.mark.parametrize('driver,argv,reason', [
    ('train_dae.py', ['--wgrad', 'bf16', '--dtype', 'float64', '-dae_dict', STANDARD, '-segmentation_net', 'fcn8'],
     'float32'),
    ('train_dae.py', ['--wgrad', 'bf16', '-dae_dict', '{"kind": "contextmod"}'], 'context module'),
    ('train_dae.py', ['--wgrad', 'bf16'], 'context module'),     # the default kind
    ('train_fcn8.py', ['--wgrad', 'bf16', '--dtype', 'float64'], 'float32'),
])
def test_drivers_refuse_wgrad_bf16_with_status_2_before_any_gpu_work(tmp_path, driver, argv, reason):
    env = dict(os.environ, HIP_VISIBLE_DEVICES='', CUDA_VISIBLE_DEVICES='')    # no device to touch
    r = subprocess.run([sys.executable, os.path.join(ROOT, driver), '--synthetic', '--savepath', str(tmp_path / 's')]
                       + argv, capture_output=True, text=True, cwd=ROOT, env=env)
    assert r.returncode == 2, r.stdout[-1000:] + r.stderr[-1000:]
    assert "wgrad='bf16'" in r.stderr and reason in r.stderr, r.stderr
    assert 'Traceback' not in r.stderr
    assert not os.path.exists(str(tmp_path / 's'))               # nothing was made


def test_check_supported_carries_the_mode():
    from iterative_inference_segm_amd import train
    dd = {'kind': 'standard', 'concat_h': ['pool4']}
    train.check_supported('standard', ('crossentropy',), dae_dict=dd, wgrad='bf16', dtype='float32')
    train.check_supported('contextmod', ('crossentropy',), wgrad='f32', dtype='float64')
    with pytest.raises(NotImplementedError, match='context module'):
        train.check_supported('contextmod', ('crossentropy',), wgrad='bf16')
    with pytest.raises(NotImplementedError, match='float32'):
        train.check_supported('standard', ('crossentropy',), dae_dict=dd, wgrad='bf16', dtype='float64')
    with pytest.raises(ValueError, match='wgrad'):
        train.check_supported('standard', ('crossentropy',), dae_dict=dd, wgrad='fp8')
