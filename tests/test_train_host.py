"""CPU: the training entries of the C ABI check their arguments before any launch, and train_dae.py's host
side: what it refuses, how it parses its dict options, and the checkpoint its save routine writes."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, SHAPE = -1, -2


def _wdesc(**kw):
    from iterative_inference_segm_amd import _lib
    d = _lib.WgradDesc()
    d.B, d.Cin, d.Cout, d.H, d.W, d.K, d.dil = 2, 14, 11, 40, 36, 3, 1
    for k, v in kw.items():
        setattr(d, k, v)
    OH, OW = d.H - d.dil * (d.K - 1), d.W - d.dil * (d.K - 1)
    if 'gz_H' not in kw:
        d.gz_H, d.gz_W, d.gz_y0, d.gz_x0 = OH, OW, 0, 0
    if 'so' not in kw:
        d.so, d.sc = d.Cin * d.K * d.K, d.K * d.K
    return d


def test_training_abi_status_codes_without_a_gpu(built_lib):
    from iterative_inference_segm_amd import _lib
    lib = _lib.load()
    assert lib.iiseg_abi_version() == 34
    fake = [C.c_void_p(4096 * (k + 1)) for k in range(8)]      # never dereferenced: checks come first
    # ---- loss ----
    assert lib.iiseg_ctx_loss_partials(2, 40, 36) == 2 * 6
    assert lib.iiseg_ctx_loss_partials(0, 40, 36) == SHAPE and lib.iiseg_ctx_loss_partials(2, 0, 36) == SHAPE
    for sfx in ('f32', 'f64'):
        cnt = getattr(lib, 'iiseg_ctx_loss_count_' + sfx)
        assert cnt(None, None, fake[1], fake[2], 2, 11, 40, 36) == NULL
        assert cnt(None, fake[0], None, fake[2], 2, 11, 40, 36) == NULL
        assert cnt(None, fake[0], fake[1], None, 2, 11, 40, 36) == NULL
        for bad in ((2, 17, 40, 36), (2, 1, 40, 36), (0, 11, 40, 36), (2, 11, 0, 36), (2, 11, 40, -3)):
            assert cnt(None, *fake[:3], *bad) == SHAPE, bad
        loss = getattr(lib, 'iiseg_ctx_loss_' + sfx)
        ok = (2, 11, 40, 36, 1, 1.0)
        for k in (0, 1, 2, 4, 5):                               # g (3) may be NULL: validation
            args = list(fake[:6])
            args[k] = None
            assert loss(None, *args, *ok) == NULL, k
        for bad in ((2, 17, 40, 36, 1, 1.0), (2, 11, 0, 36, 1, 1.0), (0, 11, 40, 36, 1, 1.0),
                    (2, 11, 40, 36, 0, 1.0), (2, 11, 40, 36, 4, 1.0), (2, 11, 40, 36, 3, float('nan'))):
            assert loss(None, *fake[:6], *bad) == SHAPE, bad
    # ---- weight gradient ----
    ok = _wdesc()
    assert lib.iiseg_conv_small_wgrad_partials(C.byref(ok), 4) == 2 * 3 * 1
    assert lib.iiseg_conv_small_wgrad_partials(C.byref(ok), 8) == 2 * 5 * 1
    assert lib.iiseg_conv_small_wgrad_partials(C.byref(ok), 2) == SHAPE
    assert lib.iiseg_conv_small_wgrad_partials(None, 4) == NULL
    bads = [dict(K=2), dict(K=5), dict(K=0), dict(Cin=17), dict(Cout=17), dict(Cout=0), dict(B=0), dict(H=0),
            dict(W=-1), dict(dil=0), dict(dil=20), dict(gz_H=10, gz_W=10, gz_y0=0, gz_x0=0),
            dict(gz_H=60, gz_W=60, gz_y0=-1, gz_x0=0), dict(so=7, sc=9)]
    for sfx in ('f32', 'f64'):
        fn = getattr(lib, 'iiseg_conv_small_wgrad_' + sfx)
        for k in (0, 1, 4, 5, 6):                               # out (2) and gz (3) may be NULL
            args = list(fake[:7])
            args[k] = None
            assert fn(None, C.byref(ok), *args) == NULL, k
        assert fn(None, None, *fake[:7]) == NULL
        for bad in bads:
            d = _wdesc(**bad)
            assert fn(None, C.byref(d), *fake[:7]) == SHAPE, bad
            assert lib.iiseg_conv_small_wgrad_partials(C.byref(d), 4) == SHAPE, bad
    # both parameter layouts, 1x1, dilation up to the map
    for good in (dict(so=9, sc=99), dict(K=1, so=14, sc=1), dict(K=1, so=1, sc=11), dict(dil=16),
                 dict(Cin=11, so=99, sc=9), dict(Cin=1, Cout=16, so=9, sc=9)):
        assert lib.iiseg_conv_small_wgrad_partials(C.byref(_wdesc(**good)), 4) > 0, good
    # ---- optimizer ----
    for sfx in ('f32', 'f64'):
        fn = getattr(lib, 'iiseg_opt_step_' + sfx)
        assert fn(None, 2, *fake[:6], 100) == SHAPE and fn(None, -1, *fake[:6], 100) == SHAPE
        assert fn(None, 0, *fake[:6], 0) == SHAPE and fn(None, 1, *fake[:6], -5) == SHAPE
        for k in (0, 1, 2, 4):
            args = list(fake[:6])
            args[k] = None
            assert fn(None, 0, *args, 100) == NULL, k
        # rmsprop needs neither s2 nor the adam state; adam needs both
        rms = list(fake[:6])
        rms[3] = rms[5] = None
        assert fn(None, 1, *rms, 100) == NULL


DRIVER = os.path.join(ROOT, 'train_dae.py')


@pytest.mark.parametrize('argv,reason', [
    (['-dae_dict', '{"kind": "standard"}'], 'contextmod'),
    (['-dae_dict', '{"kind": "fcn8"}'], 'contextmod'),
    (['-train_dict', '{"training_loss": ["dice"]}'], 'dice'),
    (['-train_dict', '{"training_loss": ["crossentropy", "squared_error_h"]}'], 'squared_error_h'),
    (['-train_dict', '{"full_im_ft": true}'], 'full_im_ft'),
    (['-train_dict', '{"optimizer": "sgd"}'], 'optimizer'),
    (['-dae_dict', '{"concat_h": ["pool4"]}'], 'concat_h'),
])
def test_driver_refuses_what_is_not_built(tmp_path, argv, reason):
    # HIP_VISIBLE_DEVICES empty: a GPU call would fail differently; the refusal comes first
    env = dict(os.environ, HIP_VISIBLE_DEVICES='', CUDA_VISIBLE_DEVICES='')
    r = subprocess.run([sys.executable, DRIVER, '--synthetic', '--savepath', str(tmp_path)] + argv,
                       capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode != 0
    assert reason in r.stderr, r.stderr
    assert not os.listdir(str(tmp_path))                       # nothing was started


def test_train_function_refuses_ae_h_and_bad_arguments(tmp_path):
    import train_dae as td
    kw = dict(savepath=str(tmp_path), loadpath=str(tmp_path), synthetic=True,
              dae_dict_updates={'kind': 'contextmod'}, training_loss=['crossentropy'])
    with pytest.raises(NotImplementedError, match='ae_h'):
        td.train('camvid', 'fcn8', ae_h=True, **kw)
    with pytest.raises(NotImplementedError, match='contextmod'):
        td.train('camvid', 'fcn8', savepath=str(tmp_path))     # the function's own default kind is 'fcn8'
    with pytest.raises(ValueError, match='Unknown dataset'):
        td.train('imagenet', 'fcn8', **kw)
    with pytest.raises(ValueError, match='saving directory'):
        td.train('camvid', 'fcn8', **dict(kw, savepath=None))
    with pytest.raises(NotImplementedError):
        td.train('camvid', 'fcn_fcresnet', **kw)


def test_driver_arguments_and_defaults():
    import train_dae as td
    args, train_dict, dae_dict = td.parse_args([])
    # reference train_dae.py:462-499
    assert args.dataset == 'camvid' and args.segmentation_net == 'densenet' and args.train_from_0_255 is False
    assert train_dict == {'learning_rate': 0.0001, 'lr_anneal': 0.99, 'weight_decay': 0.0001, 'num_epochs': 500,
                          'max_patience': 100, 'optimizer': 'rmsprop', 'batch_size': [10, 10, 10],
                          'training_loss': ['crossentropy'], 'lmb': 1, 'full_im_ft': False}
    assert dae_dict['kind'] == 'contextmod' and dae_dict['from_gt'] is False and dae_dict['noise'] == 0
    assert dae_dict['exp_name'] == 'flip_final_' and dae_dict['concat_h'] == ['input']
    assert args.data_augmentation == {'crop_size': [224, 224], 'horizontal_flip': 0.5, 'fill_mode': 'constant'}
    args, train_dict, dae_dict = td.parse_args(
        ['-train_dict', '{"optimizer": "adam", "learning_rate": 0.001, "training_loss": ["squared_error"]}',
         '-dae_dict', '{"from_gt": true, "noise": 0.1}', '-data_augmentation', '{}', '--num_epochs', '3',
         '--synthetic', '--seed', '7', '-segmentation_net', 'fcn8', '-train_from_0_255', 'True'])
    assert train_dict['optimizer'] == 'adam' and train_dict['learning_rate'] == 0.001
    assert train_dict['num_epochs'] == 3 and train_dict['lr_anneal'] == 0.99          # the rest keeps its default
    assert dae_dict['from_gt'] is True and dae_dict['noise'] == 0.1 and dae_dict['kind'] == 'contextmod'
    assert args.data_augmentation == {} and args.synthetic and args.seed == 7 and args.train_from_0_255 is True
    helptext = td.make_parser().format_help()
    for flag in ['-dataset', '-segmentation_net', '-train_dict', '-dae_dict', '-data_augmentation',
                 '-train_from_0_255', '--synthetic', '--savepath', '--loadpath', '--resume', '--num_epochs',
                 '--seed']:
        assert flag in helptext
    assert 'only enters the experiment name' in re.sub(r'\s+', ' ', helptext)          # weight_decay


def test_checkpoint_written_by_the_driver_reads_back(tmp_path):
    import train_dae as td
    from iterative_inference_segm_amd import synthetic as S
    from iterative_inference_segm_amd.contextmod import PARAM_ORDER
    from iterative_inference_segm_amd.weights import load_param_list
    params = S.make_contextmod_params(11, 3, seed=3)
    errors = ([1.0, 0.5], [0.9, 0.6], [0.1, 0.2], [0.05, 0.04])
    td.save_checkpoint(str(tmp_path), 'best', params, errors)
    back = load_param_list(str(tmp_path / 'dae_model_best.npz'), PARAM_ORDER)
    assert list(back) == PARAM_ORDER
    for n in PARAM_ORDER:
        for a, b in zip(params[n], back[n]):
            assert a.dtype == b.dtype and np.array_equal(a, b)
    with np.load(str(tmp_path / 'dae_errors_best.npz')) as f:
        assert [f['arr_%d' % i].tolist() for i in range(4)] == [list(e) for e in errors]


def test_training_product_never_imports_oracle_or_tests():
    for path in (os.path.join(ROOT, 'train_dae.py'),
                 os.path.join(ROOT, 'iterative_inference_segm_amd', 'train.py'),
                 os.path.join(ROOT, 'scripts', 'bench_train.py')):
        src = open(path).read()
        assert not re.search(r'^\s*(from|import)\s+(oracle|tests|ctx_train_ref)\b', src, flags=re.M), path
