"""CPU (no launch): the host side of deconv='bf16'  -- the switch's refusals in the module and
the driver, the argument errors of ops.deconv_wgrad / ops.deconv_dgrad before the library is touched, the status
codes and plans of the six entry points of csrc/deconv_grad_bf16.hip."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_NULL, ERR_SHAPE, ERR_UNSUPPORTED = 0, -1, -2, -5
P = C.c_void_p(16)          # a non-NULL pointer no check dereferences: every call below fails before a launch
THIN = dict(n_layers_per_block=[2, 3, 2, 3, 2], n_pool=2, growth=4)


def _thin_params(seed=5):
    from iterative_inference_segm_amd import synthetic as S
    from iterative_inference_segm_amd.densenet import layer_plan
    return S.make_densenet_params(layer_plan(THIN['n_layers_per_block'], THIN['n_pool'], THIN['growth'], 8, 3, 4),
                                  seed=seed)


def _driver():
    sys.path.insert(0, ROOT)
    try:
        import train_fcdensenet
    finally:
        sys.path.remove(ROOT)
    return train_fcdensenet


def test_switch_is_named_and_check_mode_refuses():
    import torch
    from iterative_inference_segm_amd import ops, params, train
    assert params.SWITCHES_16BIT['deconv'] == 'transposed-convolution gradients'
    assert ops.DECONV_MODES == params.MODES_16BIT == ('f32', 'bf16')
    assert train.check_deconv('f32', 'float64') == 'f32' and train.check_deconv('bf16', 'float32') == 'bf16'
    assert params.check_mode('deconv', 'bf16', torch.float32, True) == 'bf16'
    with pytest.raises(ValueError, match='deconv'):
        train.check_deconv('fp16', 'float32')
    with pytest.raises(NotImplementedError, match="deconv='bf16'"):
        train.check_deconv('bf16', 'float64')
    with pytest.raises(ValueError, match='deconv'):
        params.check_mode('deconv', 'tf32', torch.float32, True)
    with pytest.raises(NotImplementedError, match='transposed-convolution gradients'):
        params.check_mode('deconv', 'bf16', torch.float32, False)
    with pytest.raises(NotImplementedError, match="deconv='bf16'"):
        params.check_mode('deconv', 'bf16', torch.float64, True)


def test_module_takes_the_mode_and_refuses_it_where_it_does_not_apply(built_lib):
    import torch
    from iterative_inference_segm_amd.densenet import FCDenseNet
    params = _thin_params()
    assert FCDenseNet(params, 4, trainable=True, device='cpu', mma='f32', **THIN).deconv == 'f32'
    assert FCDenseNet(params, 4, device='cpu', mma='f32', **THIN).deconv == 'f32'
    net = FCDenseNet(params, 4, trainable=True, device='cpu', mma='f32', deconv='bf16', **THIN)
    assert net.deconv == 'bf16' and net.wgrad == 'f32'
    with pytest.raises(NotImplementedError, match="deconv='bf16'"):
        FCDenseNet(params, 4, trainable=False, device='cpu', mma='f32', deconv='bf16', **THIN)
    with pytest.raises(NotImplementedError, match="deconv='bf16'"):
        FCDenseNet(params, 4, trainable=True, device='cpu', mma='f32', dtype=torch.float64, deconv='bf16', **THIN)
    with pytest.raises(ValueError, match='deconv'):
        FCDenseNet(params, 4, trainable=True, device='cpu', mma='f32', deconv='fp16', **THIN)


def test_parser_default_and_check_supported():
    drv = _driver()
    assert drv.make_parser().parse_args([]).deconv == 'f32'
    assert drv.make_parser().parse_args(['--deconv', 'bf16']).deconv == 'bf16'
    drv.check_supported('camvid', '/nowhere', deconv='bf16')
    drv.check_supported('camvid', '/nowhere', wgrad='bf16', deconv='bf16')
    drv.check_supported('camvid', '/nowhere', dtype='float64', deconv='f32')
    with pytest.raises(NotImplementedError, match='deconv'):
        drv.check_supported('camvid', '/nowhere', dtype='float64', deconv='bf16')
    with pytest.raises(ValueError, match='deconv'):
        drv.check_supported('camvid', '/nowhere', deconv='tf32')


def test_driver_refuses_float64_with_bf16_before_the_gpu(tmp_path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES='')
    env.pop('IISEG_SAVEPATH', None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_fcdensenet.py'), '--synthetic', '--savepath',
                        str(tmp_path / 'out'), '--dtype', 'float64', '--deconv', 'bf16'], cwd=ROOT, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 2, (r.stdout, r.stderr)
    assert r.stderr.startswith('train_fcdensenet.py: ') and "deconv='bf16'" in r.stderr and 'float32' in r.stderr
    assert 'Traceback' not in r.stderr
    assert not os.listdir(str(tmp_path))                   # nothing created


def test_ops_refuse_before_the_library_is_touched(monkeypatch):
    """Host tensors; `_lib.load` is replaced by a function that fails the test if it is reached."""
    import torch
    from iterative_inference_segm_amd import _lib, ops

    def reached():
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'load', reached)
    B, Cin, Cout, H, W = 2, 5, 3, 4, 6
    x, g = torch.zeros((B, Cin, H, W)), torch.zeros((B, Cout, 2 * H + 1, 2 * W + 1))
    Wt, dW, db = torch.zeros((Cin, Cout, 3, 3)), torch.zeros((Cin, Cout, 3, 3)), torch.zeros(Cout)
    # the mode, in either precision of the call
    for mode in ('fp16', 'bf16c8', None, 16):
        with pytest.raises(ValueError, match='mma'):
            ops.deconv_wgrad(x, g, dW, db, 2, mma=mode)
        with pytest.raises(ValueError, match='mma'):
            ops.deconv_dgrad(g, Wt, 2, (H, W), mma=mode)
    # float32 tensors only
    for bad in ((x.double(), g, dW, db), (x, g.double(), dW, db), (x, g, dW.double(), db), (x, g, dW, db.double()),
                (x.numpy(), g, dW, db), (None, g, dW, db)):
        with pytest.raises(ValueError, match='float32'):
            ops.deconv_wgrad(*bad, 2, mma='bf16')
    for bad in ((g.double(), Wt), (g, Wt.double()), (g.numpy(), Wt), (g, None)):
        with pytest.raises(ValueError, match='float32'):
            ops.deconv_dgrad(*bad, 2, (H, W), mma='bf16')
    # the layer's kind, the shapes, contiguity
    with pytest.raises(ValueError, match='K = 3'):
        ops.deconv_wgrad(x, g, torch.zeros((Cin, Cout, 4, 4)), db, 2, mma='bf16')
    with pytest.raises(ValueError, match='stride'):
        ops.deconv_wgrad(x, g, dW, db, 1, mma='bf16')
    with pytest.raises(ValueError, match='K = 3'):
        ops.deconv_dgrad(g, torch.zeros((Cin, Cout, 4, 4)), 2, (H, W), mma='bf16')
    with pytest.raises(ValueError, match='stride'):
        ops.deconv_dgrad(g, Wt, 4, (H, W), mma='bf16')
    with pytest.raises(ValueError, match='contiguous'):
        ops.deconv_wgrad(torch.zeros((B, Cin, W, H)).transpose(2, 3), g, dW, db, 2, mma='bf16')
    with pytest.raises(ValueError, match='contiguous'):
        ops.deconv_dgrad(torch.zeros(tuple(g.shape[:2]) + (2 * W + 1, 2 * H + 1)).transpose(2, 3), Wt, 2, (H, W),
                         mma='bf16')
    for bad in ((x[:, :4], g, dW, db), (x, g[:, :2], dW, db), (x, g[:, :, :-1], dW, db), (x, g, dW, torch.zeros(Cout + 1)),
                (x[0], g, dW, db), (x, g, dW[0], db), (x, g, torch.zeros((Cin, Cout, 3, 2)), db)):
        with pytest.raises(ValueError, match='deconv_wgrad'):
            ops.deconv_wgrad(*(t.contiguous() for t in bad), 2, mma='bf16')
    with pytest.raises(ValueError, match='deconv_wgrad'):
        ops.deconv_wgrad(x, g, dW, db, 2, window=(0, 0, 2 * H, 2 * W), mma='bf16')        # g is the full output's
    for bad in ((g[:, :2].contiguous(), Wt), (g[:, :, :-1].contiguous(), Wt), (g[0], Wt), (g, Wt[0])):
        with pytest.raises(ValueError, match='deconv_dgrad'):
            ops.deconv_dgrad(*bad, 2, (H, W), mma='bf16')
    with pytest.raises(ValueError, match='deconv_dgrad'):
        ops.deconv_dgrad(g, Wt, 2, (H + 1, W), mma='bf16')
    # device tensors only (these are on the host): the last check before the library
    with pytest.raises(ValueError, match='device'):
        ops.deconv_wgrad(x, g, dW, db, 2, mma='bf16')
    with pytest.raises(ValueError, match='device'):
        ops.deconv_wgrad(x, g, dW, None, 2, mma='bf16')
    with pytest.raises(ValueError, match='device'):
        ops.deconv_dgrad(g, Wt, 2, (H, W), mma='bf16')


def _desc(B=2, Cin=5, Cout=3, H=4, W=6, K=3, stride=2, window=None):
    from iterative_inference_segm_amd import ops
    return ops.deconv_desc((B, Cin, H, W), Cout, K, stride, window)


def _entries(lib):
    """The six entries as functions of a descriptor pointer, every other pointer non-NULL."""
    return {'check': lambda d: lib.iiseg_deconv_grad_bf16_check(d),
            'slabs': lambda d: lib.iiseg_deconv_wgrad_bf16_slabs(d),
            'wgrad_ws': lambda d: lib.iiseg_deconv_wgrad_bf16_workspace_elems(d),
            'dgrad_ws': lambda d: lib.iiseg_deconv_dgrad_bf16_workspace_elems(d),
            'wgrad': lambda d: lib.iiseg_deconv_wgrad_bf16(None, d, P, P, P, P, P),
            'dgrad': lambda d: lib.iiseg_deconv_dgrad_bf16(None, d, P, P, P, P)}


def test_status_codes_without_a_gpu(built_lib):
    from iterative_inference_segm_amd import _lib
    lib = _lib.load()
    assert lib.iiseg_abi_version() == 34 == _lib.ABI_VERSION
    ent = _entries(lib)
    good = _desc()
    assert ent['check'](C.byref(good)) == OK
    for name, f in ent.items():
        assert f(None) == ERR_NULL, name
        for kw in (dict(B=0), dict(Cin=0), dict(Cout=0), dict(H=0), dict(W=0), dict(window=(0, 0, 10, 13)),
                   dict(window=(1, 0, 9, 13)), dict(window=(0, 0, 0, 5)), dict(window=(-1, 0, 3, 3)), dict(K=0)):
            assert f(C.byref(_desc(**kw))) == ERR_SHAPE, (name, kw)
        # valid layers this file does not do: FCN-8's K = 4 / 16 layers, any other stride
        for kw in (dict(K=4), dict(K=16, stride=8), dict(stride=1), dict(K=4, stride=2), dict(stride=3), dict(K=2)):
            assert f(C.byref(_desc(**kw))) == ERR_UNSUPPORTED, (name, kw)
    d = C.byref(good)
    for i in (0, 1, 3):                                              # x, g, dW; db may be NULL
        ptrs = [P] * 5
        ptrs[i] = None
        assert lib.iiseg_deconv_wgrad_bf16(None, d, *ptrs) == ERR_NULL, i
    for i in (0, 1, 3):                                              # g, w, gx; the workspace is not used
        ptrs = [P] * 4
        ptrs[i] = None
        assert lib.iiseg_deconv_dgrad_bf16(None, d, *ptrs) == ERR_NULL, i
    # an output that overlaps an input
    big = _desc(B=1, Cin=1, Cout=1, H=1, W=1)
    a, b = C.c_void_p(4096), C.c_void_p(4096 + 8)
    far = [C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p(3 << 20)]
    assert lib.iiseg_deconv_wgrad_bf16(None, C.byref(big), a, far[0], None, C.c_void_p(4096), far[1]) == ERR_UNSUPPORTED
    assert lib.iiseg_deconv_wgrad_bf16(None, C.byref(big), far[0], a, None, far[1], b) == ERR_UNSUPPORTED   # db in g
    assert lib.iiseg_deconv_dgrad_bf16(None, C.byref(big), a, far[0], None, b) == ERR_UNSUPPORTED           # gx in g
    assert lib.iiseg_deconv_dgrad_bf16(None, C.byref(big), far[0], a, None, b) == ERR_UNSUPPORTED           # gx in W


def test_plans_without_a_gpu(built_lib):
    from iterative_inference_segm_amd import _lib
    lib = _lib.load()
    # at most four tiles: one slab, straight into dW and db, no workspace (NULL is fine then -- not checked by a
    # launch here); the data gradient never has one
    for kw in (dict(B=1, Cin=1, Cout=1, H=1, W=1), dict(B=3, Cin=1, Cout=1, H=1, W=1),
               dict(B=1, Cin=240, Cout=240, H=1, W=1), dict(B=2, H=8, W=16)):
        d = C.byref(_desc(**kw))
        assert lib.iiseg_deconv_wgrad_bf16_slabs(d) == 1, kw
        assert lib.iiseg_deconv_wgrad_bf16_workspace_elems(d) == 0, kw
        assert lib.iiseg_deconv_dgrad_bf16_workspace_elems(d) == 0, kw
    # several slabs: slabs * (nW + Cout) floats, and then a NULL workspace is refused
    for Cin, Cout in ((1, 1), (20, 24), (80, 80), (33, 20)):
        for win in (None, (0, 0, 74, 100), (1, 1, 73, 99)):
            dd = _desc(B=3, Cin=Cin, Cout=Cout, H=37, W=50, window=win)
            d = C.byref(dd)
            n = lib.iiseg_deconv_wgrad_bf16_slabs(d)
            assert n >= 2, (Cin, Cout)
            assert lib.iiseg_deconv_wgrad_bf16_workspace_elems(d) == n * (Cin * Cout * 9 + Cout)
            assert lib.iiseg_deconv_dgrad_bf16_workspace_elems(d) == 0
            assert lib.iiseg_deconv_wgrad_bf16(None, d, P, P, None, P, P) == ERR_NULL
    # the plan counts channel blocks: many of them leave fewer slabs, never fewer than one
    narrow, wide = _desc(B=3, Cin=20, Cout=24, H=37, W=50), _desc(B=3, Cin=240, Cout=240, H=37, W=50)
    nn_, nw = (lib.iiseg_deconv_wgrad_bf16_slabs(C.byref(v)) for v in (narrow, wide))
    assert 1 <= nw < nn_
    # FC-DenseNet103's five TransitionUp layers at batch 3 and 10, 224 x 224: every plan is valid
    for B in (3, 10):
        for ch, hw in ((240, 7), (192, 14), (160, 28), (112, 56), (80, 112)):
            d = C.byref(_desc(B=B, Cin=ch, Cout=ch, H=hw, W=hw, window=(0, 0, 2 * hw, 2 * hw)))
            assert lib.iiseg_deconv_grad_bf16_check(d) == OK
            assert lib.iiseg_deconv_wgrad_bf16_slabs(d) >= 1
