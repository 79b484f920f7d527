"""CPU (no launch): the host side of FCN-8 training -- status codes of every new entry point, the slab / workspace
queries of the K x K weight gradient, the driver's defaults and refusals, the module's refusal of the 16-bit legs."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OK, ERR_NULL, ERR_SHAPE, ERR_UNSUPPORTED = 0, -1, -2, -5
P = C.c_void_p(16)          # a non-NULL pointer no check dereferences: every call below fails before a launch


@pytest.fixture(scope='module')
def lib(built_lib):
    from iterative_inference_segm_amd import _lib
    return _lib.load()


def kxk(B=2, Cin=5, Cout=3, H=9, W=8, K=3, ci0=0, Cin_tot=None, layout='oihw', y0=0, x0=0, mapH=None, mapW=None):
    from iterative_inference_segm_amd import ops
    mapH, mapW = mapH or y0 + H, mapW or x0 + W
    return ops.conv_wgrad_kxk_desc((B, Cin, mapH, mapW), Cout, K, (y0, x0, H, W), Cin_tot, ci0, layout)


def test_abi_version_is_unchanged(lib):
    from iterative_inference_segm_amd import _lib
    assert lib.iiseg_abi_version() == _lib.ABI_VERSION == 34


def test_kxk_status_codes(lib):
    chk = lambda d: lib.iiseg_conv_wgrad_kxk_check(C.byref(d))
    assert lib.iiseg_conv_wgrad_kxk_check(None) == ERR_NULL
    assert lib.iiseg_conv_wgrad_kxk_slabs(None, 4) == ERR_NULL
    assert lib.iiseg_conv_wgrad_kxk_workspace_elems(None, 4) == ERR_NULL
    for K in range(1, 8):
        assert chk(kxk(K=K)) == OK
    for K in (0, -1, 8, 9):
        d = kxk(K=3)
        d.K = K
        d.so, d.sc = 5 * K * K, K * K
        assert chk(d) == ERR_SHAPE, K
    for field in ('B', 'Cin', 'Cout', 'H', 'W'):
        for v in (0, -3):
            d = kxk()
            setattr(d, field, v)
            assert chk(d) == ERR_SHAPE, (field, v)
    d = kxk(H=2, K=3)                                     # smaller than the filter
    assert chk(d) == ERR_SHAPE
    # the window inside the planes: strides
    assert chk(kxk(y0=3, x0=2, mapH=20, mapW=17)) == OK
    for field, v in (('x_y0', -1), ('x_x0', -1)):
        d = kxk(y0=3, x0=2, mapH=20, mapW=17)
        setattr(d, field, v)
        assert chk(d) == ERR_SHAPE
    d = kxk(y0=3, x0=2, mapH=20, mapW=17)
    d.x_row = 2 + 8 - 1                                   # the window's rows would overlap the next row
    assert chk(d) == ERR_SHAPE
    d = kxk(y0=3, x0=2, mapH=20, mapW=17)
    d.x_plane = (3 + 9) * 17 - 1
    assert chk(d) == ERR_SHAPE
    d = kxk(y0=3, x0=2, mapH=20, mapW=17)
    d.x_image = 5 * d.x_plane - 1
    assert chk(d) == ERR_SHAPE
    # the parameter array
    assert chk(kxk(Cin_tot=9, ci0=4)) == OK
    assert chk(kxk(Cin_tot=9, ci0=4, layout='iohw')) == OK
    assert chk(kxk(Cin_tot=9, ci0=5)) == ERR_SHAPE        # ci0 + Cin > Cin_tot
    d = kxk(Cin_tot=9, ci0=-1)
    assert chk(d) == ERR_SHAPE
    d = kxk()
    d.so += 1                                             # neither layout
    assert chk(d) == ERR_SHAPE
    assert lib.iiseg_conv_wgrad_kxk_slabs(C.byref(kxk()), 2) == ERR_SHAPE
    # the launch entries: NULL operands, and a bad descriptor before anything else
    d = kxk()
    for fn in (lib.iiseg_conv_wgrad_kxk_f32, lib.iiseg_conv_wgrad_kxk_f64):
        assert fn(None, None, P, P, P, P, P) == ERR_NULL
        assert fn(None, C.byref(d), None, P, P, P, P) == ERR_NULL
        assert fn(None, C.byref(d), P, None, P, P, P) == ERR_NULL
        assert fn(None, C.byref(d), P, P, P, None, P) == ERR_NULL
        bad = kxk()
        bad.K = 8
        assert fn(None, C.byref(bad), P, P, P, P, P) == ERR_SHAPE


def test_kxk_slabs_and_workspace(lib):
    # fc6 at real size: 490 output pixels against 25 088 x 4096 outputs -- one slab, straight into dW
    fc6 = kxk(B=10, Cin=512, Cout=4096, H=13, W=13, K=7)
    for eb in (4, 8):
        assert lib.iiseg_conv_wgrad_kxk_slabs(C.byref(fc6), eb) == 1
        assert lib.iiseg_conv_wgrad_kxk_workspace_elems(C.byref(fc6), eb) == 0
    # score_pool3: 11 output channels on a wide window -- many slabs
    sp3 = kxk(B=1, Cin=256, Cout=11, H=37, W=150, K=1)
    for eb in (4, 8):
        n = lib.iiseg_conv_wgrad_kxk_slabs(C.byref(sp3), eb)
        assert n >= 2
        assert lib.iiseg_conv_wgrad_kxk_workspace_elems(C.byref(sp3), eb) == n * (11 * 256 * 1 + 11)
    # required exactly when non-zero
    assert lib.iiseg_conv_wgrad_kxk_f32(None, C.byref(sp3), P, P, None, P, P) == ERR_NULL
    d = kxk(B=3, Cin=33, Cout=130, H=20, W=37, K=7)
    n = lib.iiseg_conv_wgrad_kxk_slabs(C.byref(d), 4)
    assert lib.iiseg_conv_wgrad_kxk_workspace_elems(C.byref(d), 4) == (0 if n == 1 else n * (130 * 33 * 49 + 130))


def deconv_desc(B=2, Cin=4, H=3, W=5, Cout=7, K=4, s=2, window=None):
    from iterative_inference_segm_amd import ops
    return ops.deconv_desc((B, Cin, H, W), Cout, K, s, window)


def test_deconv_grad_status_codes(lib):
    d = deconv_desc()
    assert lib.iiseg_deconv_wgrad_partials(None) == ERR_NULL
    assert lib.iiseg_deconv_wgrad_partials(C.byref(d)) >= 1
    assert lib.iiseg_deconv_wgrad_partials(C.byref(deconv_desc(Cout=100, Cin=70, K=3))) >= 1   # any channel count
    for field in ('B', 'Cin', 'H', 'W', 'Cout', 'K', 'stride', 'OH', 'OW'):
        for v in (0, -2):
            bad = deconv_desc()
            setattr(bad, field, v)
            assert lib.iiseg_deconv_wgrad_partials(C.byref(bad)) == ERR_SHAPE, (field, v)
    full = ((3 - 1) * 2 + 4, (5 - 1) * 2 + 4)
    assert lib.iiseg_deconv_wgrad_partials(C.byref(deconv_desc(window=(1, 3, full[0] - 1, full[1] - 3)))) >= 1
    for win in ((1, 0, full[0], full[1]), (0, 1, full[0], full[1]), (-1, 0, 2, 2), (0, -1, 2, 2),
                (full[0], 0, 1, 1)):                                           # a window outside the full output
        assert lib.iiseg_deconv_wgrad_partials(C.byref(deconv_desc(window=win))) == ERR_SHAPE, win
    for fn in (lib.iiseg_deconv_dgrad_f32, lib.iiseg_deconv_dgrad_f64):
        assert fn(None, None, P, P, P) == ERR_NULL
        assert fn(None, C.byref(d), None, P, P) == ERR_NULL
        assert fn(None, C.byref(d), P, None, P) == ERR_NULL
        assert fn(None, C.byref(d), P, P, None) == ERR_NULL
        assert fn(None, C.byref(deconv_desc(window=(1, 0) + full)), P, P, P) == ERR_SHAPE
    for fn in (lib.iiseg_deconv_wgrad_f32, lib.iiseg_deconv_wgrad_f64):
        assert fn(None, None, P, P, P, P, P) == ERR_NULL
        assert fn(None, C.byref(d), None, P, P, P, P) == ERR_NULL
        assert fn(None, C.byref(d), P, None, P, P, P) == ERR_NULL
        assert fn(None, C.byref(d), P, P, None, P, P) == ERR_NULL              # the workspace is always required
        assert fn(None, C.byref(d), P, P, P, None, P) == ERR_NULL
        assert fn(None, C.byref(deconv_desc(window=(1, 0) + full)), P, P, P, P, P) == ERR_SHAPE


def test_small_kernels_status_codes(lib):
    from iterative_inference_segm_amd import _lib
    for fn in (lib.iiseg_relu_gate_f32, lib.iiseg_relu_gate_f64):
        assert fn(None, None, P, P, 4) == ERR_NULL
        assert fn(None, P, None, P, 4) == ERR_NULL
        assert fn(None, P, P, None, 4) == ERR_NULL
        assert fn(None, P, P, P, 0) == ERR_SHAPE
        assert fn(None, P, P, P, -1) == ERR_SHAPE
        assert fn(None, P, C.c_void_p(32), C.c_void_p(32), 4) == ERR_UNSUPPORTED    # dst aliasing out
    assert lib.iiseg_l2_term_partials(0) == ERR_SHAPE
    assert lib.iiseg_l2_term_partials(_lib.L2_MAX_RANGES + 1) == ERR_UNSUPPORTED
    assert lib.iiseg_l2_term_partials(21) >= 21
    table = lambda *v: (C.c_int64 * len(v))(*v)
    for fn in (lib.iiseg_l2_term_f32, lib.iiseg_l2_term_f64):
        good = table(0, 4, 6, 10)
        assert fn(None, None, P, 10, good, 2, 1e-4, P, P) == ERR_NULL
        assert fn(None, P, None, 10, good, 2, 1e-4, P, P) == ERR_NULL
        assert fn(None, P, P, 10, None, 2, 1e-4, P, P) == ERR_NULL
        assert fn(None, P, P, 10, good, 2, 1e-4, None, P) == ERR_NULL
        assert fn(None, P, P, 10, good, 2, 1e-4, P, None) == ERR_NULL
        assert fn(None, P, P, 0, good, 2, 1e-4, P, P) == ERR_SHAPE
        assert fn(None, P, P, 10, good, 0, 1e-4, P, P) == ERR_SHAPE
        assert fn(None, P, P, 9, good, 2, 1e-4, P, P) == ERR_SHAPE                  # past the buffer
        assert fn(None, P, P, 10, table(0, 4, 3, 10), 2, 1e-4, P, P) == ERR_SHAPE   # overlapping
        assert fn(None, P, P, 10, table(0, 4, 6, 6), 2, 1e-4, P, P) == ERR_SHAPE    # empty
        assert fn(None, P, P, 10, table(-1, 4, 6, 10), 2, 1e-4, P, P) == ERR_SHAPE


def test_driver_defaults_are_the_references():
    sys.path.insert(0, ROOT)
    try:
        import train_fcn8
    finally:
        sys.path.remove(ROOT)
    a = train_fcn8.make_parser().parse_args([])
    assert a.dataset == 'camvid' and a.learning_rate == 0.0001 and a.penal_cst == 0.0          # :276-284
    assert a.num_epochs == 750 and a.max_patience == 100 and a.batch_size == [10, 1, 1]        # :285-298
    assert a.data_augmentation == {'crop_size': [224, 224], 'horizontal_flip': True, 'fill_mode': 'constant'}
    assert a.early_stop_class is None and a.train_from_0_255 is False                          # :303-310
    assert train_fcn8.make_parser().parse_args(['-ne', '3']).num_epochs == 3
    assert a.dtype == 'float32' and not a.synthetic and not a.resume and a.savepath is None
    # the reference's operator precedence in exp_name, kept
    assert train_fcn8.experiment_name({'crop_size': [224, 224]}) == 'fcn8_data_aug'
    assert train_fcn8.experiment_name({}) == ''
    # GlorotUniform: symmetric limit, zero biases, seeded
    p = train_fcn8.glorot_params({'a': ((8, 4, 3, 3), 8), 'd': ((4, 4, 4, 4), 4)}, 7)
    lim = (6.0 / ((8 + 4) * 9)) ** 0.5
    assert abs(p['a'][0]).max() <= lim and abs(p['a'][0]).max() > 0.8 * lim and not p['a'][1].any()
    assert (train_fcn8.glorot_params({'a': ((8, 4, 3, 3), 8)}, 7)['a'][0] == p['a'][0]).all()
    import numpy as np
    T = train_fcn8.one_hot_void_last(np.array([[[0, 3], [11, 2]]]), 11)
    assert T.shape == (1, 12, 2, 2) and T[0, 11, 1, 0] == 1 and T[0, 3, 0, 1] == 1 and T.sum() == 4


@pytest.mark.parametrize('argv,reason', [
    (['--synthetic', '-pascal', 'true', '--savepath', '{tmp}/out'], 'pascal'),
    (['--synthetic'], 'saving directory'),
    (['--synthetic', '--savepath', '{tmp}/out', '--dtype', 'bfloat16'], '16-bit'),
    (['--synthetic', '--savepath', '{tmp}/out', '-dataset', 'nope'], 'Unknown dataset'),
    (['--synthetic', '--savepath', '{tmp}/out', '-batch_size', '[10, 0, 1]'], 'batch_size'),
])
def test_driver_refuses_before_the_gpu(tmp_path, argv, reason):
    env = dict(os.environ, HIP_VISIBLE_DEVICES='')
    env.pop('IISEG_SAVEPATH', None)
    argv = [a.replace('{tmp}', str(tmp_path)) for a in argv]
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_fcn8.py')] + argv, cwd=ROOT, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 2, (r.stdout, r.stderr)
    assert reason in r.stderr and r.stderr.startswith('train_fcn8.py: ')
    assert not os.listdir(str(tmp_path))                   # nothing created


def test_trainable_module_refuses_the_16_bit_legs(built_lib):
    """At construction, with the reason, before any device work (host parameters, no GPU here)."""
    import torch
    from iterative_inference_segm_amd import synthetic as S
    from iterative_inference_segm_amd.fcn8 import FCN8
    params = S.make_fcn8_params(3, 4, width_div=16, fc_channels=32)
    for kw in (dict(mma='bf16c8'), dict(mma='bf16'), dict(mma='bf16x3'), dict(dtype=torch.bfloat16, mma='f32')):
        with pytest.raises(NotImplementedError, match='16-bit'):
            FCN8(params, 4, trainable=True, device='cpu', **kw)
    with pytest.raises(NotImplementedError, match='temperature'):
        FCN8(params, 4, trainable=True, temperature=2.0, mma='f32', device='cpu')
    from iterative_inference_segm_amd.train import FCN8Trainer

    class NotTrainable:
        trainable = False
    with pytest.raises(NotImplementedError, match='trainable=True'):
        FCN8Trainer(NotTrainable(), 4, [4])
