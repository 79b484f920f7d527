"""CPU: the true-gradient entries of the C ABI (csrc/ctx_grad.hip) check their arguments before any launch, and
the driver refuses --update gradient for a DAE kind without a backward pass before it touches the GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, SHAPE = -1, -2


def _ddesc(**kw):
    """dilconv-like 11 -> 11, 3 x 3, dilation 2 on a 40 x 36 gradient map, whole g_x, dense destination."""
    from iterative_inference_segm_amd import _lib
    d = _lib.DgradDesc()
    d.B, d.Cin, d.Cout, d.K, d.dil, d.OH, d.OW = 2, 11, 11, 3, 2, 40, 36
    for k in ('B', 'Cin', 'Cout', 'K', 'dil', 'OH', 'OW'):
        if k in kw:
            setattr(d, k, kw[k])
    span = d.dil * (d.K - 1)
    d.out_H, d.out_W, d.out_y0, d.out_x0 = d.OH, d.OW, 0, 0
    d.wy0, d.wx0, d.WH, d.WW = 0, 0, d.OH + span, d.OW + span
    d.ci0, d.nci = 0, d.Cin
    for k in ('wy0', 'wx0', 'WH', 'WW', 'ci0', 'nci'):
        if k in kw:
            setattr(d, k, kw[k])
    d.gx_C, d.gx_H, d.gx_W, d.gx_c0, d.gx_y0, d.gx_x0 = d.nci, d.WH, d.WW, 0, 0, 0
    d.so, d.sc = d.K * d.K, d.Cout * d.K * d.K                # W[in,out,k,k]
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_gradient_abi_status_codes_without_a_gpu(built_lib):
    from iterative_inference_segm_amd import _lib
    lib = _lib.load()
    assert lib.iiseg_abi_version() == 34                       # the additions are backward compatible
    fake = [C.c_void_p(4096 * (k + 1)) for k in range(8)]      # never dereferenced: checks come first
    # ---- masked data gradient ----
    ok = _ddesc()
    assert lib.iiseg_conv_small_dgrad_blocks(C.byref(ok)) == 2 * 3 * 1      # 44 x 40 -> 3 x 1 tiles per image
    assert lib.iiseg_conv_small_dgrad_blocks(None) == NULL
    bads = [dict(K=2), dict(K=5), dict(K=0), dict(Cin=17), dict(Cout=17), dict(Cin=0), dict(Cout=0), dict(B=0),
            dict(OH=0), dict(OW=-1), dict(dil=0), dict(dil=-2),
            # window outside the (44, 40) map of g_x, or empty
            dict(wy0=-1), dict(wx0=-1), dict(WH=0), dict(WW=0), dict(wy0=5), dict(wx0=1), dict(WH=45),
            dict(wy0=32, wx0=32, WH=20, WW=4),
            # channel range outside the layer's input channels
            dict(ci0=-1), dict(nci=0), dict(ci0=3, nci=9), dict(nci=12),
            # destination too small for the window / the channels, or a negative corner
            dict(gx_H=43), dict(gx_W=39), dict(gx_C=10), dict(gx_c0=1), dict(gx_y0=1), dict(gx_x0=-1),
            # the planes of `out` do not hold the map
            dict(out_H=39), dict(out_W=35), dict(out_y0=1), dict(out_x0=-1),
            # strides that are neither W[out,in,k,k] nor W[in,out,k,k]
            dict(so=7, sc=9), dict(so=9, sc=9), dict(so=99, sc=99), dict(so=0, sc=0)]
    for sfx in ('f32', 'f64'):
        fn = getattr(lib, 'iiseg_conv_small_dgrad_' + sfx)
        for k in (0, 2, 3):                                     # out (1) may be NULL: a linear layer
            args = list(fake[:4])
            args[k] = None
            assert fn(None, C.byref(ok), *args) == NULL, k
        assert fn(None, None, *fake[:4]) == NULL
        for bad in bads:
            d = _ddesc(**bad)
            assert fn(None, C.byref(d), *fake[:4]) == SHAPE, bad
            assert lib.iiseg_conv_small_dgrad_blocks(C.byref(d)) == SHAPE, bad
    # what is supported: both layouts, 1x1, the map smaller than the tap span, a window, the y half of conv1
    for good in (dict(so=99, sc=9), dict(K=1, so=1, sc=11), dict(K=1, so=11, sc=1), dict(OH=20, OW=18, dil=16),
                 dict(wy0=32, wx0=32, WH=12, WW=8), dict(Cin=14, ci0=3, nci=11, so=126, sc=9),
                 dict(Cin=1, Cout=16, so=9, sc=144), dict(gx_C=14, gx_c0=3, gx_H=50, gx_W=50, gx_y0=6, gx_x0=10),
                 dict(out_H=104, out_W=100, out_y0=32, out_x0=32)):
        assert lib.iiseg_conv_small_dgrad_blocks(C.byref(_ddesc(**good))) > 0, good
    # ---- head ----
    assert lib.iiseg_ctx_grad_head_blocks(2, 11, 11, 40, 36) == 2 * 6
    for bad in ((0, 11, 11, 40, 36), (2, 17, 11, 40, 36), (2, 1, 11, 40, 36), (2, 11, 17, 40, 36), (2, 11, 0, 40, 36),
                (2, 11, 11, 0, 36), (2, 11, 11, 40, -3)):
        assert lib.iiseg_ctx_grad_head_blocks(*bad) == SHAPE, bad
    for sfx in ('f32', 'f64'):
        fn = getattr(lib, 'iiseg_ctx_grad_head_' + sfx)
        dims = (2, 11, 11, 40, 36)
        for k in (0, 1, 3, 5):                                  # out6 (2) and gs (4) may be NULL
            args = list(fake[:6])
            args[k] = None
            assert fn(None, *args[:4], 1, 11, *args[4:], *dims) == NULL, k
        for bad in ((0, 11, 11, 40, 36), (2, 17, 11, 40, 36), (2, 11, 17, 40, 36), (2, 11, 11, 0, 36)):
            assert fn(None, *fake[:4], 1, 11, *fake[4:6], *bad) == SHAPE, bad
        for so, sc in ((2, 11), (11, 11), (0, 0), (1, 12)):     # neither W[out,in,1,1] nor W[in,out,1,1]
            assert fn(None, *fake[:4], so, sc, *fake[4:6], 2, 11, 12, 40, 36) == SHAPE, (so, sc)


DRIVER = os.path.join(ROOT, 'iterative_inference.py')


def test_driver_refuses_gradient_mode_for_a_dae_without_backward(tmp_path):
    # HIP_VISIBLE_DEVICES empty: a GPU call would fail differently; the refusal comes first
    env = dict(os.environ, HIP_VISIBLE_DEVICES='', CUDA_VISIBLE_DEVICES='')
    r = subprocess.run([sys.executable, DRIVER, '--synthetic', '--savepath', str(tmp_path), '--update', 'gradient',
                        '-dae_dict', '{"kind": "fcn8"}'], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode != 0
    assert 'NotImplementedError' in r.stderr and 'fcn8' in r.stderr and 'backward' in r.stderr, r.stderr
    assert not os.listdir(str(tmp_path))                       # nothing was written


def test_refine_refuses_a_dae_without_backward_before_any_work():
    """api._refine: NotImplementedError naming the DAE kind, before the DAE or the device is touched."""
    from iterative_inference_segm_amd.api import IterativeInference

    class NoBackward:
        kind = 'fcn8'

        def new_session(self, *a, **k):                         # any use of the DAE would show here
            raise AssertionError('the DAE was used')

        scores = new_session

    ii = IterativeInference.__new__(IterativeInference)
    ii.dae = NoBackward()
    with pytest.raises(NotImplementedError, match='fcn8'):
        ii._refine([None], None, 0.05, 2, mode='gradient')
    with pytest.raises(ValueError, match='mode'):
        ii._refine([None], None, 0.05, 2, mode='newton')


def test_context_module_refuses_training_and_gradient_mode_past_16_input_channels():
    """14 classes + an RGB image are 17 channels into conv1, one more than the weight- / data-gradient kernels take
    (Cin <= 16: the status codes above) -- and conv1 is the LAST layer a backward pass reaches.  Every entry that
    leads there refuses at its front, naming the limit; 13 classes (16 channels) pass the same point."""
    import torch

    from iterative_inference_segm_amd import synthetic as S
    from iterative_inference_segm_amd.api import IterativeInference
    from iterative_inference_segm_amd.contextmod import GRAD_MAX_CHANNELS, ContextModDAE
    assert GRAD_MAX_CHANNELS == 16
    dae = ContextModDAE(S.make_contextmod_params(14, 3, seed=31), 14, device='cpu')
    assert dae.conv1.Cin == 17
    h, y = torch.zeros(1, 3, 8, 8), torch.zeros(1, 14, 8, 8)
    limit = r'classes \+ h channels <= 16 for training and gradient mode'
    with pytest.raises(NotImplementedError, match=limit):
        dae.forward_train([h], y)
    with pytest.raises(NotImplementedError, match=limit):
        dae.backward(y)
    with pytest.raises(NotImplementedError, match=limit):
        dae.keep_pre = True
    assert dae.keep_pre is False
    with pytest.raises(NotImplementedError, match=limit):
        dae.backward_y(y, y.shape)
    with pytest.raises(NotImplementedError, match=limit):
        dae.sqerr_backward(y, y)
    ii = IterativeInference.__new__(IterativeInference)
    ii.dae = dae
    with pytest.raises(NotImplementedError, match=limit):
        ii._refine([h], y, 0.05, 2, mode='gradient')
    dae.keep_pre = False                                     # (switching it off is always allowed)
    ok = ContextModDAE(S.make_contextmod_params(13, 3, seed=31), 13, device='cpu')
    assert ok.conv1.Cin == 16
    ok.keep_pre = True
    assert ok.keep_pre is True


def test_gradient_product_never_imports_oracle_or_tests():
    for path in (os.path.join(ROOT, 'iterative_inference_segm_amd', 'contextmod.py'),
                 os.path.join(ROOT, 'scripts', 'bench_ctx_grad.py')):
        src = open(path).read()
        assert not re.search(r'^\s*(from|import)\s+(oracle|tests|ctx_train_ref|ctx_grad_ref)\b', src, flags=re.M), path
