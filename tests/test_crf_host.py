"""CPU: the dense-CRF C ABI's host-side checks (no launch happens) and the crf_inference.py drop-in's
interface against the reference's crf_inference.py."""
import ctypes as C
import inspect
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _desc(**kw):
    from iterative_inference_segm_amd import _lib
    d = _lib.CrfDesc()
    d.B, d.C, d.H, d.W, d.R, d.flags = 2, 11, 24, 20, 12, _lib.CRF_BILATERAL
    d.sxy_g, d.w_g, d.sxy_b, d.srgb, d.w_b, d.clip = 3.0, 3.0, 3.0, 13.0, 10.0, 1e-5
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_crf_abi_status_codes_without_a_gpu(built_lib):
    from iterative_inference_segm_amd import _lib
    lib = _lib.load()
    fake = [C.c_void_p(4096 * (k + 1)) for k in range(7)]      # never dereferenced: checks come first
    ok = _desc()
    assert lib.iiseg_crf_supported(C.byref(ok)) == 1
    for fn in ('iiseg_crf_prepare_f32', 'iiseg_crf_prepare_f64'):
        assert getattr(lib, fn)(None, C.byref(ok), *([None] * 7)) == -1
        assert getattr(lib, fn)(None, None, *fake) == -1
        assert getattr(lib, fn)(None, C.byref(ok), *fake[:6], None) == -1
    for fn in ('iiseg_crf_step_f32', 'iiseg_crf_step_f64'):
        assert getattr(lib, fn)(None, C.byref(ok), *([None] * 6)) == -1
        assert getattr(lib, fn)(None, C.byref(ok), None, *fake[:5]) == -1
    for bad in (dict(C=17), dict(C=1), dict(R=0), dict(R=17), dict(H=0), dict(W=0), dict(B=0),
                dict(srgb=0.0), dict(flags=4)):
        d = _desc(**bad)
        assert lib.iiseg_crf_supported(C.byref(d)) == 0, bad
        for fn in ('iiseg_crf_prepare_f32', 'iiseg_crf_prepare_f64'):
            assert getattr(lib, fn)(None, C.byref(d), *fake) == -2, (fn, bad)
        for fn in ('iiseg_crf_step_f32', 'iiseg_crf_step_f64'):
            assert getattr(lib, fn)(None, C.byref(d), *fake[:6]) == -2, (fn, bad)
    for good in (dict(C=2), dict(C=16), dict(R=1), dict(R=16), dict(H=1, W=1), dict(H=3, W=200)):
        assert lib.iiseg_crf_supported(C.byref(_desc(**good))) == 1, good
    # ping-pong only: Q_in == Q_out is refused before any launch
    assert lib.iiseg_crf_step_f32(None, C.byref(ok), *fake[:5], fake[1]) == -2


def test_dense_crf_defaults_match_the_reference_set_up():
    from iterative_inference_segm_amd.crf import DenseCRF
    crf = DenseCRF()
    assert (crf.sxy_g, crf.w_g, crf.sxy_b, crf.srgb, crf.w_b, crf.clip) == (3, 3, 3, 13, 10, 1e-5)
    assert crf.radius == 12
    assert DenseCRF(sxy_b=2.5, sxy_g=1).radius == 10 and DenseCRF(radius=5).radius == 5


def test_crf_driver_signature_and_flags(monkeypatch, capsys, tmp_path):
    import crf_inference as ci
    params = list(inspect.signature(ci.inference).parameters)
    # reference crf_inference.py:44-45, in order
    assert params[:8] == ['dataset', 'segm_net', 'which_set', 'num_iter', 'Bilateral', 'savepath',
                          'loadpath', 'test_from_0_255']
    sig = inspect.signature(ci.inference)
    assert sig.parameters['which_set'].default == 'val' and sig.parameters['num_iter'].default == 5
    assert sig.parameters['Bilateral'].default is True and sig.parameters['test_from_0_255'].default is False
    monkeypatch.setattr(sys, 'argv', ['crf_inference.py', '-h'])
    with pytest.raises(SystemExit):
        ci.main()
    helptext = capsys.readouterr().out
    for flag in ['-dataset', '-segmentation_net', '-which_set', '--num_iter', '-nit', '-test_from_0_255',
                 '--sweep', '--synthetic', '--savepath', '--loadpath', '--weights_path', '--n_images',
                 '--image_size']:
        assert flag in helptext
    captured = {}
    monkeypatch.setattr(ci, 'inference', lambda *a, **k: captured.setdefault('calls', []).append((a, k)) or
                        __import__('numpy').zeros(11))
    monkeypatch.setattr(ci.np, 'savez', lambda *a, **k: captured.setdefault('saved', a))
    ci.main(['--loadpath', str(tmp_path)])
    (a, k), = captured['calls']
    assert a == ('camvid', 'fcn8') and k['which_set'] == 'test' and k['num_iter'] == 80
    assert k['test_from_0_255'] is False
    assert captured['saved'][0].endswith(os.path.join('camvid', 'fcn8', 'img_plots', 'crf', 'results_test.npz'))
    assert captured['saved'][1].shape == (11, 1)


def test_crf_driver_errors_without_gpu(tmp_path):
    import crf_inference as ci
    with pytest.raises(ValueError, match='saving directory'):
        ci.inference('camvid', 'fcn8', savepath=None)
    kw = dict(savepath=str(tmp_path / 's'), loadpath=str(tmp_path / 'l'), synthetic=True, verbose=False,
              n_images=2)
    with pytest.raises(ValueError):
        ci.inference('camvid', 'nonsense_net', **kw)
    with pytest.raises(NotImplementedError):
        ci.inference('camvid', 'fcn_fcresnet', **kw)
    with pytest.raises(ValueError, match='Unknown dataset'):
        ci.inference('imagenet', 'fcn8', **kw)


def test_crf_product_never_imports_oracle_or_tests():
    for path in (os.path.join(ROOT, 'crf_inference.py'),
                 os.path.join(ROOT, 'iterative_inference_segm_amd', 'crf.py')):
        src = open(path).read()
        assert not re.search(r'^\s*(from|import)\s+(oracle|tests|crf_ref)\b', src, flags=re.M), path
