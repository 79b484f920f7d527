"""CPU: the 16-bit data-gradient mode (dgrad='bf16'; include/iiseg.h iiseg_conv_dgrad_bf16*, kernels in
csrc/conv_dgrad_bf16.hip) checks every argument before any launch, ops.conv_dgrad refuses tensors it has no kernel
for, the modules refuse the mode where it has no meaning and both training drivers take `--dgrad` and refuse it,
with the reason, where nothing is built for it."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, SHAPE, ALIGN, UNSUPPORTED = -1, -2, -3, -5


def _desc(**kw):
    from iterative_inference_segm_amd import _lib
    d = _lib.ConvDgradDesc()
    d.B, d.Cin, d.Cout, d.H, d.W, d.K, d.pad = 2, 24, 16, 14, 13, 3, 1
    d.ci0 = 0
    for k, v in kw.items():
        setattr(d, k, v)
    if 'Cin_tot' not in kw:
        d.Cin_tot = d.ci0 + d.Cin
    if 'so' not in kw:
        d.so, d.sc = d.Cin_tot * 9, 9
    return d


# K != 3; pad != 1; non-positive sizes; ci0 + Cin > Cin_tot; strides that are neither layout; the descriptor's limits
BAD = [dict(K=1), dict(K=2), dict(K=5), dict(K=0), dict(pad=0), dict(pad=2), dict(pad=100), dict(pad=-1),
       dict(B=0), dict(B=-1), dict(B=65536), dict(Cin=0), dict(Cin=-3), dict(Cout=0), dict(Cout=65536), dict(H=0),
       dict(W=-2), dict(ci0=1, Cin_tot=24), dict(Cin_tot=23), dict(ci0=-1), dict(Cin_tot=0),
       dict(so=7, sc=9), dict(so=24 * 9, sc=8), dict(ci0=3, Cin_tot=30, so=24 * 9, sc=9), dict(so=9, sc=15 * 9),
       dict(H=1 << 15, W=1 << 14), dict(Cin=30000, Cout=30000, Cin_tot=30000), dict(accumulate=2), dict(accumulate=-1)]
GOOD = [(dict(), 1 * 9 * 16 * 64), (dict(accumulate=1), 9 * 16 * 64), (dict(ci0=3, Cin_tot=40), 9 * 16 * 64),
        (dict(so=9, sc=16 * 9), 9 * 16 * 64), (dict(ci0=5, Cin_tot=29, so=9, sc=16 * 9), 9 * 16 * 64),
        (dict(Cin=64, Cout=32), 2 * 9 * 16 * 64), (dict(Cin=65, Cout=33), 3 * 9 * 16 * 128),
        (dict(Cin=11, Cout=64, H=224, W=224, B=10), 4 * 9 * 16 * 64),
        (dict(Cin=130, Cout=130, H=1, W=1, B=1), 9 * 9 * 16 * 192), (dict(Cin=512, Cout=512), 32 * 9 * 16 * 512)]


def test_conv_dgrad_bf16_status_codes_without_a_gpu(built_lib):
    from iterative_inference_segm_amd import _lib, build
    lib = _lib.load()
    assert 'conv_dgrad_bf16.hip' in build.SOURCES
    assert lib.iiseg_abi_version() == _lib.ABI_VERSION == 34     # a backward-compatible addition
    MB = 1 << 20                                                 # never dereferenced: a refused call launches nothing
    gz, packed, gate, gx, W = (C.c_void_p(MB * (k + 1)) for k in range(5))
    assert lib.iiseg_conv_dgrad_bf16_check(None) == NULL
    assert lib.iiseg_conv_dgrad_bf16_pack_elems(None) == NULL
    assert lib.iiseg_conv_dgrad_bf16_pack(None, None, W, packed) == NULL
    assert lib.iiseg_conv_dgrad_bf16(None, None, gz, packed, gate, gx) == NULL
    ok = _desc()
    assert lib.iiseg_conv_dgrad_bf16_check(C.byref(ok)) == 0
    assert lib.iiseg_conv_dgrad_bf16_pack(None, C.byref(ok), None, packed) == NULL
    assert lib.iiseg_conv_dgrad_bf16_pack(None, C.byref(ok), W, None) == NULL
    assert lib.iiseg_conv_dgrad_bf16(None, C.byref(ok), None, packed, gate, gx) == NULL
    assert lib.iiseg_conv_dgrad_bf16(None, C.byref(ok), gz, None, gate, gx) == NULL
    assert lib.iiseg_conv_dgrad_bf16(None, C.byref(ok), gz, packed, gate, None) == NULL      # (the gate may be NULL)
    for bad in BAD:
        d = _desc(**bad)
        assert lib.iiseg_conv_dgrad_bf16_check(C.byref(d)) == SHAPE, bad
        assert lib.iiseg_conv_dgrad_bf16_pack_elems(C.byref(d)) == SHAPE, bad
        assert lib.iiseg_conv_dgrad_bf16_pack(None, C.byref(d), W, packed) == SHAPE, bad
        assert lib.iiseg_conv_dgrad_bf16(None, C.byref(d), gz, packed, gate, gx) == SHAPE, bad
    # the descriptor first, then the pointers
    assert lib.iiseg_conv_dgrad_bf16(None, C.byref(_desc(K=5)), None, None, None, None) == SHAPE
    # gx aliasing g_z: the same address, or anywhere inside it; gx on the filter image; the image on W
    assert lib.iiseg_conv_dgrad_bf16(None, C.byref(ok), gz, packed, gate, gz) == UNSUPPORTED
    inside = C.c_void_p(gz.value + 4 * (2 * 16 * 14 * 13 - 1))
    assert lib.iiseg_conv_dgrad_bf16(None, C.byref(ok), gz, packed, None, inside) == UNSUPPORTED
    assert lib.iiseg_conv_dgrad_bf16(None, C.byref(ok), gz, packed, None, packed) == UNSUPPORTED
    assert lib.iiseg_conv_dgrad_bf16_pack(None, C.byref(ok), W, W) == UNSUPPORTED
    # alignment: 16 bytes for the image, 4 for the maps
    odd = C.c_void_p(packed.value + 8)
    assert lib.iiseg_conv_dgrad_bf16(None, C.byref(ok), gz, odd, gate, gx) == ALIGN
    assert lib.iiseg_conv_dgrad_bf16_pack(None, C.byref(ok), W, odd) == ALIGN
    assert lib.iiseg_conv_dgrad_bf16(None, C.byref(ok), C.c_void_p(gz.value + 2), packed, gate, gx) == ALIGN


def test_pack_elems_is_the_image_of_the_slice(built_lib):
    """[k-tiles of 16 output channels][9 taps][16][input channels rounded up to 64]: B, H, W do not enter."""
    from iterative_inference_segm_amd import _lib
    lib = _lib.load()
    for good, elems in GOOD:
        d = _desc(**good)
        assert lib.iiseg_conv_dgrad_bf16_check(C.byref(d)) == 0, good
        assert lib.iiseg_conv_dgrad_bf16_pack_elems(C.byref(d)) == elems, good
        assert elems == -(-d.Cout // 16) * 9 * 16 * (-(-d.Cin // 64) * 64)


def test_ops_conv_dgrad_refuses_tensors_before_the_library_is_called(built_lib, monkeypatch):
    import torch
    from iterative_inference_segm_amd import _lib, ops

    def no_library():
        raise AssertionError('the library was asked')
    gz, W = torch.zeros((1, 3, 4, 4)), torch.zeros((3, 2, 3, 3))            # host tensors: nothing may reach a launch
    out = torch.zeros((1, 2, 4, 4))
    monkeypatch.setattr(_lib, 'load', no_library)
    for args, kw in (((gz.double(), W), {}), ((gz, W.double()), {}), ((gz.half(), W.half()), {}),
                     ((gz, W), dict(out=out.double())), ((gz, W), dict(gate=out.to(torch.bfloat16))),
                     ((gz, W), dict(gate=out > 0)), ((gz.numpy(), W), {})):
        with pytest.raises(ValueError, match='float32'):
            ops.conv_dgrad(*args, **kw)
    with pytest.raises(ValueError, match='3x3'):
        ops.conv_dgrad(gz, torch.zeros((3, 2, 1, 1)))
    with pytest.raises(ValueError, match='layout'):
        ops.conv_dgrad(gz, W, layout='hwio')
    with pytest.raises(ValueError, match='accumulate'):
        ops.conv_dgrad(gz, W, accumulate=True)
    with pytest.raises(ValueError, match='packed'):
        ops.conv_dgrad(gz, W, packed=torch.zeros(8))
    with pytest.raises(ValueError, match='input channels'):
        ops.conv_dgrad(gz, W, ci0=1, cin=2)
    with pytest.raises(ValueError, match='input channels'):
        ops.conv_dgrad(torch.zeros((1, 2, 4, 4)), W)             # g_z has W's input channel count, not its output's
    with pytest.raises(ValueError, match='gradient is'):
        ops.conv_dgrad(gz, W, out=torch.zeros((1, 2, 4, 5)))
    with pytest.raises(ValueError, match='gradient is'):
        ops.conv_dgrad(gz, W, ci0=1, gate=out)
    assert ops.DGRAD_MODES == ('f32', 'bf16')


def test_modules_refuse_dgrad_bf16_where_it_has_no_meaning():
    """When the module is built, before any device work (the arguments are checked first)."""
    import torch
    from iterative_inference_segm_amd.dae import StandardDAE
    from iterative_inference_segm_amd.fcn8 import FCN8
    for kw in (dict(trainable=True, dtype=torch.float64), dict(trainable=False, dtype=torch.float32)):
        with pytest.raises(NotImplementedError, match="dgrad='bf16'"):
            StandardDAE({}, 11, concat_h=['pool4'], device='cpu', dgrad='bf16', **kw)
        with pytest.raises(NotImplementedError, match="dgrad='bf16'"):
            FCN8({}, 11, device='cpu', dgrad='bf16', **kw)
    with pytest.raises(ValueError, match='dgrad'):
        StandardDAE({}, 11, concat_h=['pool4'], device='cpu', trainable=True, dgrad='fp8')
    with pytest.raises(ValueError, match='dgrad'):
        FCN8({}, 11, device='cpu', trainable=True, dgrad='fp8')


def test_parse_args_of_both_drivers_accepts_dgrad():
    sys.path.insert(0, ROOT)
    try:
        import train_dae
        import train_fcn8
    finally:
        sys.path.remove(ROOT)
    assert train_dae.parse_args([])[0].dgrad == 'f32'
    assert train_dae.parse_args(['--dgrad', 'bf16'])[0].dgrad == 'bf16'
    assert train_fcn8.parse_args(['--savepath', 'x']).dgrad == 'f32'
    assert train_fcn8.parse_args(['--savepath', 'x', '--dgrad', 'bf16']).dgrad == 'bf16'
    for mod in (train_dae, train_fcn8):
        with pytest.raises(SystemExit):
            mod.parse_args(['--dgrad', 'fp8'])


STANDARD = '{"kind": "standard", "concat_h": ["pool4"]}'


@pytest.mark.parametrize('driver,argv,reason', [
    ('train_dae.py', ['--dgrad', 'bf16', '--dtype', 'float64', '-dae_dict', STANDARD, '-segmentation_net', 'fcn8'],
     'float32'),
    ('train_dae.py', ['--dgrad', 'bf16', '-dae_dict', '{"kind": "contextmod"}'], 'context module'),
    ('train_dae.py', ['--dgrad', 'bf16'], 'context module'),     # the default kind
    ('train_fcn8.py', ['--dgrad', 'bf16', '--dtype', 'float64'], 'float32'),
])
def test_drivers_refuse_dgrad_bf16_with_status_2_before_any_gpu_work(tmp_path, driver, argv, reason):
    env = dict(os.environ, HIP_VISIBLE_DEVICES='', CUDA_VISIBLE_DEVICES='')    # no device to touch
    r = subprocess.run([sys.executable, os.path.join(ROOT, driver), '--synthetic', '--savepath', str(tmp_path / 's')]
                       + argv, capture_output=True, text=True, cwd=ROOT, env=env)
    assert r.returncode == 2, r.stdout[-1000:] + r.stderr[-1000:]
    assert "dgrad='bf16'" in r.stderr and reason in r.stderr, r.stderr
    assert 'Traceback' not in r.stderr
    assert not os.path.exists(str(tmp_path / 's'))               # nothing was made


def test_check_supported_carries_the_mode():
    from iterative_inference_segm_amd import train
    dd = {'kind': 'standard', 'concat_h': ['pool4']}
    train.check_supported('standard', ('crossentropy',), dae_dict=dd, dgrad='bf16', dtype='float32')
    train.check_supported('standard', ('crossentropy',), dae_dict=dd, wgrad='bf16', dgrad='bf16', dtype='float32')
    train.check_supported('contextmod', ('crossentropy',), dgrad='f32', dtype='float64')
    train.check_dgrad('bf16', 'float32')
    with pytest.raises(NotImplementedError, match='context module'):
        train.check_supported('contextmod', ('crossentropy',), dgrad='bf16')
    with pytest.raises(NotImplementedError, match='float32'):
        train.check_supported('standard', ('crossentropy',), dae_dict=dd, dgrad='bf16', dtype='float64')
    with pytest.raises(NotImplementedError, match='float32'):
        train.check_dgrad('bf16', 'float64')
    with pytest.raises(ValueError, match='dgrad'):
        train.check_supported('standard', ('crossentropy',), dae_dict=dd, dgrad='fp8')
