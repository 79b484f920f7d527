"""CPU: fwd='bf16' on the standard DAE is taken and refused, with the reason, before any device
work -- by the module, by train.check_supported and by train_dae.py (through -train_dict: the driver has no flag for
it) -- and the check of a fwd16 launch (include/iiseg.h iiseg_conv_halo_bf16_fwd_check) lifts exactly one refusal of
iiseg_conv_halo_bf16_supported: a two-source layer whose first source is no multiple of 16 channels."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, SHAPE, UNSUPPORTED = -1, -2, -5


def _dae(**kw):
    from iterative_inference_segm_amd import synthetic as S
    from iterative_inference_segm_amd.dae import StandardDAE
    params = S.make_dae_params(4, (3,), concat_h=['pool1'], n_filters=4, additional_pool=1, seed=1)
    return StandardDAE(params, 4, concat_h=['pool1'], padding=3, n_filters=4, additional_pool=1, device='cpu', **kw)


def test_the_module_refuses_fwd_bf16_where_it_has_no_meaning(built_lib):
    """When the module is built, before any device work."""
    for kw in (dict(trainable=True, dtype=torch.float64), dict(trainable=False, dtype=torch.float32)):
        with pytest.raises(NotImplementedError, match="fwd='bf16'"):
            _dae(fwd='bf16', **kw)
    with pytest.raises(ValueError, match='fwd'):
        _dae(trainable=True, fwd='fp8')
    # mma= on a trainable module keeps its refusal: the mode is a keyword of its own
    with pytest.raises(NotImplementedError, match='16-bit legs'):
        _dae(trainable=True, mma='bf16', fwd='bf16')


def test_the_module_builds_every_layer_for_the_mode_and_none_without_it(built_lib):
    for kw, want in ((dict(), False), (dict(fwd='f32'), False), (dict(fwd='bf16'), True)):
        dae = _dae(trainable=True, dtype=torch.float32, mma='f32', **kw)
        assert dae.fwd == ('bf16' if want else 'f32') and dae.wgrad == dae.dgrad == 'f32'
        convs = dae.conv_layers()
        assert sorted(convs) == ['conv1_1', 'conv2_1', 'up_conv1', 'up_conv2']
        assert all(c.fwd16 is want and c.mma == 'f32' for c in convs.values())
    assert _dae(trainable=False, dtype=torch.float32).fwd == 'f32'


def test_check_supported_takes_fwd():
    from iterative_inference_segm_amd import train
    std = dict(kind='standard', dae_dict={'concat_h': ['pool4']})
    train.check_supported(**std)
    train.check_supported(fwd='f32', dtype='float64', **std)
    train.check_supported(fwd='bf16', **std)
    train.check_supported('contextmod', fwd='f32')
    with pytest.raises(NotImplementedError, match="fwd='bf16'.*float32"):
        train.check_supported(fwd='bf16', dtype='float64', **std)
    with pytest.raises(NotImplementedError, match="fwd='bf16'.*context module"):
        train.check_supported('contextmod', fwd='bf16')
    with pytest.raises(ValueError, match='fwd'):
        train.check_supported(fwd='fp8', **std)


def test_train_dae_takes_fwd_through_train_dict_only():
    sys.path.insert(0, ROOT)
    try:
        import train_dae
    finally:
        sys.path.remove(ROOT)
    assert 'fwd' not in train_dae.TRAIN_DICT
    args, train_dict, _ = train_dae.parse_args(['-train_dict', '{"fwd": "bf16"}'])
    assert train_dict['fwd'] == 'bf16' and train_dict['batch_size'] == [10, 10, 10]
    assert 'fwd' not in train_dae.parse_args([])[1]
    assert '"fwd": "bf16"' in train_dae.make_parser().format_help()


STANDARD = {'kind': 'standard', 'concat_h': ['pool2'], 'n_filters': 8, 'noise': 0.1, 'from_gt': True}


@pytest.mark.parametrize('extra,words', [
    (['--dtype', 'float64', '-dae_dict', json.dumps(STANDARD)], ("fwd='bf16'", 'float32')),
    ([], ("fwd='bf16'", 'context module'))], ids=['float64', 'contextmod'])
def test_train_dae_refuses_fwd_bf16_with_status_2_before_any_gpu_work(tmp_path, extra, words):
    env = dict(os.environ, HIP_VISIBLE_DEVICES='', CUDA_VISIBLE_DEVICES='')    # no device to touch
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_dae.py'), '--synthetic', '--savepath',
                        str(tmp_path / 's'), '--loadpath', str(tmp_path / 'l'), '-segmentation_net', 'fcn8',
                        '-train_dict', '{"fwd":"bf16"}'] + extra, capture_output=True, text=True, cwd=ROOT, env=env)
    assert r.returncode == 2, r.stdout[-1000:] + r.stderr[-1000:]
    assert all(w in r.stderr for w in words), r.stderr
    assert 'Traceback' not in r.stderr
    assert not os.path.exists(str(tmp_path / 's')) and not os.path.exists(str(tmp_path / 'l'))   # nothing was made


def _layer(Cin, Cout=8):
    from iterative_inference_segm_amd import ops
    return ops.Conv(np.zeros((Cout, Cin, 3, 3), np.float32), np.zeros(Cout, np.float32), pad=1, relu=True,
                    device='cpu', dtype=torch.float32, mma='f32', fwd16=True)


def test_the_straddling_check_status_codes_without_a_launch(built_lib):
    from iterative_inference_segm_amd import _lib
    lib = _lib.load()
    assert lib.iiseg_abi_version() == _lib.ABI_VERSION == 34
    assert lib.iiseg_conv_halo_bf16_fwd_check(None) == NULL
    assert lib.iiseg_conv_halo_bf16_fwd_weight_bytes(None) == 0
    fake = [C.c_void_p(1 << (24 + k)) for k in range(3)]         # never dereferenced: refused before any launch
    for C1, C2 in ((3, 4), (17, 13), (24, 16), (1, 1), (15, 2000)):
        conv = _layer(C1 + C2)
        d = conv._describe(2, C1, C2, 9, 33, None, None, False)
        # the refusal of the existing entries stays; the new check lifts it and nothing else
        assert lib.iiseg_conv_halo_bf16_supported(C.byref(d)) == 0
        assert lib.iiseg_conv_halo_bf16_weight_bytes(C.byref(d)) == 0
        assert lib.iiseg_conv_halo_bf16(None, C.byref(d), fake[0], fake[1], None, None, fake[2], None, None, fake[0],
                                        None, None, None) == UNSUPPORTED
        assert lib.iiseg_conv_halo_bf16_fwd_check(C.byref(d)) == 0
        nkt = (C1 + C2 + 15) // 16
        assert lib.iiseg_conv_halo_bf16_fwd_weight_bytes(C.byref(d)) == nkt * 18 * 32 * 16      # Cout 8: 32 rows
        # the second source is still required, and the other refusals still hold
        assert lib.iiseg_conv_halo_bf16_fwd(None, C.byref(d), fake[0], None, None, None, fake[2], None, None, fake[0],
                                            None, None, None) == NULL
        assert conv._choose(d, x2=True) == 'halo_bf16'
    conv = _layer(16 + 16)
    for C1, C2 in ((16, 16), (32, 0)):                           # aligned or single-source: both entries agree
        d = conv._describe(2, C1, C2, 9, 33, None, None, False)
        assert lib.iiseg_conv_halo_bf16_supported(C.byref(d)) == 1
        assert lib.iiseg_conv_halo_bf16_fwd_check(C.byref(d)) == 0
        assert lib.iiseg_conv_halo_bf16_fwd_weight_bytes(C.byref(d)) == lib.iiseg_conv_halo_bf16_weight_bytes(C.byref(d))
    conv = _layer(3 + 4)
    d = conv._describe(2, 3, 4, 9, 33, None, None, False)
    for field, value, status in (('KH', 1, UNSUPPORTED), ('dil', 2, UNSUPPORTED), ('B', 0, SHAPE), ('OH', 40, SHAPE),
                                 ('C2', -1, SHAPE), ('flags', 2, UNSUPPORTED)):    # 2: DePool2D has one source
        bad = type(d)()
        C.memmove(C.byref(bad), C.byref(d), C.sizeof(d))
        setattr(bad, field, value)
        assert lib.iiseg_conv_halo_bf16_fwd_check(C.byref(bad)) == status, field
    # a layer that is not fwd16 keeps the form it had: the straddling launch is not its business
    from iterative_inference_segm_amd import ops
    plain = ops.Conv(np.zeros((8, 7, 3, 3), np.float32), None, pad=1, relu=True, device='cpu', dtype=torch.float32,
                     mma='bf16')
    assert plain._choose(plain._describe(2, 3, 4, 9, 33, None, None, False), x2=True) == 'direct'
