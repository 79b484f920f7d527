"""CPU: the entries of the C ABI added for training the standard DAE (zero-padded 3x3 weight gradient, grid form
of the optimizer step) check their arguments before any launch; the slab / workspace queries agree.  train_dae.py
refuses what this slice of the standard kind does not train, before any GPU work, and lets the rest through."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, 'train_dae.py')

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


BAD = [dict(K=1), dict(K=2), dict(K=5), dict(K=0), dict(B=0), dict(B=-1), dict(B=65536), dict(Cin=0), dict(Cout=0),
       dict(Cout=-3), dict(Cin=65536, Cin_tot=65536), dict(Cout=65536), dict(H=0), dict(W=-2), dict(pad=-1),
       dict(H=1, W=1, pad=0),                                    # no output pixel
       dict(ci0=-1), dict(ci0=1, Cin_tot=24), dict(Cin_tot=23), dict(Cin_tot=0),
       dict(so=7, sc=9), dict(so=24 * 9, sc=8), dict(ci0=3, Cin_tot=30, so=24 * 9, sc=9),   # so of Cin, not Cin_tot
       dict(so=9, sc=15 * 9),
       dict(H=1 << 16, W=1 << 15),                               # H W past 2^30
       dict(H=1 << 15, W=(1 << 15) - 2, pad=2),                  # OH OW past 2^30
       dict(Cin=30000, Cout=30000, Cin_tot=30000)]               # Cout Cin_tot 9 past 2^31
GOOD = [dict(), dict(pad=0), dict(pad=100), dict(pad=5, H=3, W=4), dict(ci0=3, Cin_tot=40), dict(so=9, sc=16 * 9),
        dict(ci0=5, Cin_tot=29, so=9, sc=16 * 9), dict(Cin=1024, Cout=2048, H=7, W=7, B=10),
        dict(Cin=11, Cout=64, H=224, W=224, pad=100, B=10), dict(H=1, W=1), dict(H=1 << 15, W=1 << 15, pad=1)]


def test_conv_wgrad_status_codes_without_a_gpu(built_lib):
    from iterative_inference_segm_amd import _lib
    lib = _lib.load()
    assert lib.iiseg_abi_version() == _lib.ABI_VERSION           # a backward-compatible addition
    fake = [C.c_void_p(4096 * (k + 1)) for k in range(5)]        # never dereferenced: checks come first
    assert lib.iiseg_conv_wgrad_check(None) == NULL
    assert lib.iiseg_conv_wgrad_slabs(None, 4) == NULL
    assert lib.iiseg_conv_wgrad_workspace_elems(None, 4) == NULL
    ok = _desc(H=37, W=150)                                      # several slabs: the workspace is required
    assert lib.iiseg_conv_wgrad_check(C.byref(ok)) == 0
    for bytes_ in (2, 0, 16):
        assert lib.iiseg_conv_wgrad_slabs(C.byref(ok), bytes_) == SHAPE
        assert lib.iiseg_conv_wgrad_workspace_elems(C.byref(ok), bytes_) == SHAPE
    for sfx in ('f32', 'f64'):
        fn = getattr(lib, 'iiseg_conv_wgrad_' + sfx)
        assert fn(None, None, *fake) == NULL
        for k in (0, 1, 2, 3):                                   # db (4) may be NULL
            args = list(fake)
            args[k] = None
            assert fn(None, C.byref(ok), *args) == NULL, k
        for bad in BAD:
            d = _desc(**bad)
            assert lib.iiseg_conv_wgrad_check(C.byref(d)) == SHAPE, bad
            assert fn(None, C.byref(d), *fake) == SHAPE, bad
            assert lib.iiseg_conv_wgrad_slabs(C.byref(d), 4) == SHAPE, bad
            assert lib.iiseg_conv_wgrad_workspace_elems(C.byref(d), 8) == SHAPE, bad
    for good in GOOD:
        assert lib.iiseg_conv_wgrad_check(C.byref(_desc(**good))) == 0, good


def test_conv_wgrad_workspace_is_what_the_launch_requires(built_lib):
    """ws = slabs * (Cout Cin 9 + Cout) elements with more than one slab, none with one; the launch refuses a NULL
    workspace exactly when the query is non-zero."""
    from iterative_inference_segm_amd import _lib
    lib = _lib.load()
    fake = [C.c_void_p(4096 * (k + 1)) for k in range(5)]
    seen = set()
    for good in GOOD + [dict(H=37, W=150), dict(H=37, W=150, B=3, Cin=130, Cout=33), dict(H=7, W=7, B=1)]:
        d = _desc(**good)
        for size, sfx in ((4, 'f32'), (8, 'f64')):
            n = lib.iiseg_conv_wgrad_slabs(C.byref(d), size)
            ws = lib.iiseg_conv_wgrad_workspace_elems(C.byref(d), size)
            assert n >= 1
            assert ws == (0 if n == 1 else n * (d.Cout * d.Cin * 9 + d.Cout)), good
            seen.add(n > 1)
            if n > 1:                                            # (one slab: a launch would follow; not here)
                args = list(fake)
                args[2] = None
                assert getattr(lib, 'iiseg_conv_wgrad_' + sfx)(None, C.byref(d), *args) == NULL
    assert seen == {False, True}
    # one workgroup per tile set for the deep layer, pixel slabs for the shallow ones
    assert lib.iiseg_conv_wgrad_slabs(C.byref(_desc(Cin=1024, Cout=2048, H=7, W=7, B=10)), 4) == 1
    assert lib.iiseg_conv_wgrad_slabs(C.byref(_desc(Cin=11, Cout=64, H=224, W=224, pad=100, B=10)), 4) >= 256
    assert lib.iiseg_conv_wgrad_slabs(C.byref(_desc(H=37, W=150, B=1)), 4) >= 2
    assert lib.iiseg_conv_wgrad_slabs(C.byref(_desc(H=37, W=150, B=1)), 8) >= 2


def test_opt_step_grid_status_codes_without_a_gpu(built_lib):
    from iterative_inference_segm_amd import _lib
    lib = _lib.load()
    fake = [C.c_void_p(4096 * (k + 1)) for k in range(6)]
    for sfx in ('f32', 'f64'):
        fn = getattr(lib, 'iiseg_opt_step_grid_' + sfx)
        assert fn(None, 2, *fake, 100) == SHAPE and fn(None, -1, *fake, 100) == SHAPE
        assert fn(None, 0, *fake, 0) == SHAPE and fn(None, 1, *fake, -5) == SHAPE
        assert fn(None, 0, *fake, (1 << 30) + 1) == SHAPE
        for k in (0, 1, 2, 4):
            args = list(fake)
            args[k] = None
            assert fn(None, 0, *args, 100) == NULL, k
        for k in (3, 5):                                         # adam needs s2 and its state
            args = list(fake)
            args[k] = None
            assert fn(None, 1, *args, 100) == NULL, k


STD = {'kind': 'standard', 'concat_h': ['pool4']}


@pytest.mark.parametrize('argv,reason', [
    (['-dae_dict', json.dumps(dict(STD, bn=1))], 'bn'),
    (['-dae_dict', json.dumps(dict(STD, dropout=0.5))], 'dropout'),
    (['-dae_dict', json.dumps(dict(STD, unpool_type='standard'))], 'unpool_type'),
    (['-dae_dict', json.dumps(dict(STD, conv_before_pool=2))], 'conv_before_pool'),
    (['-dae_dict', json.dumps(STD), '-ae_h', 'true'], 'ae_h'),
    (['-dae_dict', json.dumps({'kind': 'fcn8'})], 'fcn8'),
    (['-dae_dict', json.dumps({'kind': 'fcn8', 'concat_h': ['pool4']})], 'fcn8'),
])
def test_driver_refuses_what_the_standard_slice_does_not_train(tmp_path, argv, reason):
    # HIP_VISIBLE_DEVICES empty: a GPU call would fail differently; the refusal comes first
    env = dict(os.environ, HIP_VISIBLE_DEVICES='')
    r = subprocess.run([sys.executable, DRIVER, '--synthetic', '--savepath', str(tmp_path)] + argv,
                       capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 2
    assert reason in r.stderr, r.stderr
    assert 'Traceback' not in r.stderr
    assert not os.listdir(str(tmp_path))                       # nothing was started


def test_check_supported_lets_the_standard_kind_with_h_at_a_pool_point_through():
    import train_dae as td
    from iterative_inference_segm_amd.train import check_supported
    for concat_h in (['pool4'], ['pool2'], ['pool1', 'pool3']):
        for unpool in ('trackind', 'inverse'):
            for skip in (True, False):
                _, train_dict, dae_dict = td.parse_args(
                    ['-dae_dict', json.dumps(dict(STD, concat_h=concat_h, unpool_type=unpool, skip=skip, n_filters=8))])
                assert td.check_supported(dae_dict, train_dict['training_loss'], False, False, 'rmsprop') is None
    assert check_supported('standard', ('crossentropy', 'squared_error'), optimizer='adam',
                           dae_dict={'concat_h': ['pool4']}) is None
    # the image concatenated at the input stays the context module's: the message names both
    with pytest.raises(NotImplementedError, match='contextmod') as e:
        check_supported('standard', dae_dict={'concat_h': ['input']})
    assert 'pool' in str(e.value)
    with pytest.raises(NotImplementedError, match='concat_h'):
        td.check_supported({'kind': 'contextmod', 'concat_h': ['pool4']}, ['crossentropy'], False, False, 'rmsprop')
    for loss in ('dice', 'squared_error_h'):
        with pytest.raises(NotImplementedError, match=loss):
            check_supported('standard', (loss,), dae_dict={'concat_h': ['pool4']})
    with pytest.raises(NotImplementedError, match='full_im_ft'):
        check_supported('standard', full_im_ft=True, dae_dict={'concat_h': ['pool4']})
