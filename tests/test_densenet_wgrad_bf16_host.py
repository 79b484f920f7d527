"""CPU (no launch): the host side of wgrad='bf16' on FC-DenseNet -- the module's and the
driver's refusals, the rule that names the kernel form per layer, ops.conv_wgrad's argument errors, the status codes
and plans of the new entry points (the form's three, and db alone)."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_NULL, ERR_SHAPE = 0, -1, -2
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


def test_module_takes_the_mode_and_refuses_it_where_it_does_not_apply(built_lib):
    import torch
    from iterative_inference_segm_amd.densenet import FCDenseNet
    params = _thin_params()
    assert FCDenseNet(params, 4, trainable=True, device='cpu', mma='f32', **THIN).wgrad == 'f32'
    assert FCDenseNet(params, 4, device='cpu', mma='f32', **THIN).wgrad == 'f32'
    assert FCDenseNet(params, 4, trainable=True, device='cpu', mma='f32', wgrad='bf16', **THIN).wgrad == 'bf16'
    with pytest.raises(NotImplementedError, match="wgrad='bf16'"):
        FCDenseNet(params, 4, device='cpu', mma='f32', wgrad='bf16', **THIN)                 # not trainable
    with pytest.raises(NotImplementedError, match="wgrad='bf16'"):
        FCDenseNet(params, 4, trainable=True, device='cpu', mma='f32', dtype=torch.float64, wgrad='bf16', **THIN)
    with pytest.raises(ValueError, match='wgrad'):
        FCDenseNet(params, 4, trainable=True, device='cpu', mma='f32', wgrad='fp16', **THIN)


def test_form_rule():
    from iterative_inference_segm_amd.densenet import wgrad_co_block
    assert [wgrad_co_block(c) for c in (4, 11, 16)] == [16, 16, 16]
    assert [wgrad_co_block(c) for c in (17, 48)] == [64, 64]


def test_parser_default_and_check_supported():
    drv = _driver()
    assert drv.make_parser().parse_args([]).wgrad == 'f32'
    assert drv.make_parser().parse_args(['--wgrad', 'bf16']).wgrad == 'bf16'
    drv.check_supported('camvid', '/nowhere', wgrad='bf16')
    drv.check_supported('camvid', '/nowhere', dtype='float64', wgrad='f32')
    with pytest.raises(NotImplementedError, match='wgrad'):
        drv.check_supported('camvid', '/nowhere', dtype='float64', wgrad='bf16')
    with pytest.raises(ValueError, match='wgrad'):
        drv.check_supported('camvid', '/nowhere', wgrad='tf32')


def test_driver_refuses_float64_with_bf16_before_the_gpu(tmp_path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES='')
    env.pop('IISEG_SAVEPATH', None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_fcdensenet.py'), '--synthetic', '--savepath',
                        str(tmp_path / 'out'), '--dtype', 'float64', '--wgrad', 'bf16'], cwd=ROOT, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 2, (r.stdout, r.stderr)
    assert r.stderr.startswith('train_fcdensenet.py: ') and "wgrad='bf16'" in r.stderr and 'float32' in r.stderr
    assert 'Traceback' not in r.stderr
    assert not os.listdir(str(tmp_path))                   # nothing created


def test_ops_conv_wgrad_refuses_forms_before_the_library_is_touched(monkeypatch):
    """Host tensors; `_lib.load` is replaced by a function that fails the test if it is reached."""
    import torch
    from iterative_inference_segm_amd import _lib, ops

    def reached():
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'load', reached)
    x, gz = torch.zeros((1, 5, 4, 4)), torch.zeros((1, 16, 4, 4))
    dW, db = torch.zeros((16, 5, 3, 3)), torch.zeros(16)
    for cb in (0, 8, 32, 128, '16', None):
        with pytest.raises(ValueError, match='co_block'):
            ops.conv_wgrad(x, gz, dW, db, mma='bf16', co_block=cb)
    with pytest.raises(ValueError, match='co_block=16'):
        ops.conv_wgrad(x, gz, dW, db, mma='f32', co_block=16)
    with pytest.raises(ValueError, match='co_block=16'):
        ops.conv_wgrad(x, gz, dW, db, co_block=16)                                          # mma defaults to 'f32'
    for bad in ((x.double(), gz, dW, db), (x, gz.double(), dW, db), (x, gz, dW.double(), db), (x, gz, dW, db.double()),
                (x.double(), gz.double(), dW.double(), db.double())):
        with pytest.raises(ValueError, match='float32'):
            ops.conv_wgrad(*bad, mma='bf16', co_block=16)


def _desc(B=2, Cin=5, Cout=16, H=9, W=7, pad=1, **kw):
    from iterative_inference_segm_amd import ops
    return ops.conv_wgrad_desc((B, Cin, H, W), Cout, pad, **kw)


def test_co16_status_codes_and_plans_without_a_gpu(built_lib):
    from iterative_inference_segm_amd import _lib
    lib = _lib.load()
    d = _desc()
    assert lib.iiseg_conv_wgrad_bf16_co16_slabs(None) == ERR_NULL
    assert lib.iiseg_conv_wgrad_bf16_co16_workspace_elems(None) == ERR_NULL
    assert lib.iiseg_conv_wgrad_bf16_co16(None, None, P, P, P, P, P) == ERR_NULL
    for i in (0, 1, 3):                                              # x, gz, dW
        ptrs = [P] * 5
        ptrs[i] = None
        assert lib.iiseg_conv_wgrad_bf16_co16(None, C.byref(d), *ptrs) == ERR_NULL, i
    bad = _desc()
    bad.K = 5
    assert lib.iiseg_conv_wgrad_bf16_co16_slabs(C.byref(bad)) == ERR_SHAPE
    for kw in (dict(B=0), dict(Cin=0), dict(Cout=0), dict(H=1, W=1, pad=0), dict(Cin_tot=4), dict(ci0=-1)):
        assert lib.iiseg_conv_wgrad_bf16_co16_slabs(C.byref(_desc(**kw))) == ERR_SHAPE, kw
        assert lib.iiseg_conv_wgrad_bf16_co16_workspace_elems(C.byref(_desc(**kw))) == ERR_SHAPE, kw
        assert lib.iiseg_conv_wgrad_bf16_co16(None, C.byref(_desc(**kw)), P, P, P, P, P) == ERR_SHAPE, kw
    # one tile: one slab, straight into dW, no workspace; a 37 x 150 map: several slabs of Cout Cin 9 + Cout floats,
    # and then a NULL workspace is refused
    one = _desc(B=1, H=7, W=7)
    assert lib.iiseg_conv_wgrad_bf16_co16_slabs(C.byref(one)) == 1
    assert lib.iiseg_conv_wgrad_bf16_co16_workspace_elems(C.byref(one)) == 0
    for Cin, Cout in ((24, 16), (300, 16), (20, 33)):
        many = _desc(B=3, Cin=Cin, Cout=Cout, H=37, W=150)
        n = lib.iiseg_conv_wgrad_bf16_co16_slabs(C.byref(many))
        assert n >= 2
        assert lib.iiseg_conv_wgrad_bf16_co16_workspace_elems(C.byref(many)) == n * (Cout * Cin * 9 + Cout)
        assert lib.iiseg_conv_wgrad_bf16_co16(None, C.byref(many), P, P, None, P, P) == ERR_NULL
    # the slabs of a launch with many channel blocks are fewer: the plan counts blocks of 16 x 64 channels
    narrow, wide = _desc(B=3, Cin=48, H=37, W=150), _desc(B=3, Cin=1072, H=37, W=150)
    assert lib.iiseg_conv_wgrad_bf16_co16_slabs(C.byref(wide)) < lib.iiseg_conv_wgrad_bf16_co16_slabs(C.byref(narrow))


def test_db_alone_status_codes_and_workspace_without_a_gpu(built_lib):
    from iterative_inference_segm_amd import _lib
    lib = _lib.load()
    d = _desc()
    assert lib.iiseg_conv_wgrad_db_workspace_elems(None) == ERR_NULL
    assert lib.iiseg_conv_wgrad_db_f32(None, None, P, P, P) == ERR_NULL
    assert lib.iiseg_conv_wgrad_db_f32(None, C.byref(d), None, P, P) == ERR_NULL
    assert lib.iiseg_conv_wgrad_db_f32(None, C.byref(d), P, P, None) == ERR_NULL
    for kw in (dict(B=0), dict(Cin=0), dict(Cout=0), dict(H=1, W=1, pad=0)):
        assert lib.iiseg_conv_wgrad_db_workspace_elems(C.byref(_desc(**kw))) == ERR_SHAPE, kw
        assert lib.iiseg_conv_wgrad_db_f32(None, C.byref(_desc(**kw)), P, P, P) == ERR_SHAPE, kw
    # the plan is the fp32 weight gradient's, slab for slab -- it depends on Cin
    for Cin in (5, 48, 300):
        for H, W in ((7, 7), (37, 150)):
            dd = _desc(B=3, Cin=Cin, H=H, W=W)
            n = lib.iiseg_conv_wgrad_slabs(C.byref(dd), 4)
            assert lib.iiseg_conv_wgrad_db_workspace_elems(C.byref(dd)) == (0 if n == 1 else n * 16)
            if n > 1:
                assert lib.iiseg_conv_wgrad_db_f32(None, C.byref(dd), P, None, P) == ERR_NULL
