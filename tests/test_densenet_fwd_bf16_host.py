"""CPU (no launch): the host side of fwd='bf16' on FC-DenseNet -- the module's and the driver's
refusals, ops.bnrelu_conv_fwd's argument errors before the library is touched, the status codes and the slab rule of
the entry points of csrc/bnrelu_conv_bf16.hip."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_NULL, ERR_SHAPE, ERR_UNSUPPORTED = 0, -1, -2, -5
P = C.c_void_p(1 << 20)     # a non-NULL pointer no check dereferences: every call below fails before a launch
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


def test_switch_name_is_unchanged():
    from iterative_inference_segm_amd import params
    assert params.SWITCHES_16BIT['fwd'] == 'training forward'
    assert params.MODES_16BIT == ('f32', 'bf16')


def test_module_takes_the_mode_and_refuses_it_where_it_does_not_apply(built_lib):
    import torch
    from iterative_inference_segm_amd.densenet import FCDenseNet
    params = _thin_params()
    assert FCDenseNet(params, 4, trainable=True, device='cpu', mma='f32', **THIN).fwd == 'f32'
    assert FCDenseNet(params, 4, device='cpu', mma='f32', **THIN).fwd == 'f32'
    net = FCDenseNet(params, 4, trainable=True, device='cpu', mma='f32', fwd='bf16', **THIN)
    assert net.fwd == 'bf16' and net.wgrad == 'f32' and net.deconv == 'f32'
    with pytest.raises(NotImplementedError, match="fwd='bf16'"):
        FCDenseNet(params, 4, trainable=False, device='cpu', mma='f32', fwd='bf16', **THIN)
    with pytest.raises(NotImplementedError, match="fwd='bf16'"):
        FCDenseNet(params, 4, trainable=True, device='cpu', mma='f32', dtype=torch.float64, fwd='bf16', **THIN)
    with pytest.raises(ValueError, match='fwd'):
        FCDenseNet(params, 4, trainable=True, device='cpu', mma='f32', fwd='fp8', **THIN)


def test_parser_and_check_supported():
    drv = _driver()
    assert drv.SWITCHES['fwd'] == 'the dense-block 3x3 layers, in training and validation'
    assert drv.parse_args([]).fwd == 'f32'
    assert drv.parse_args(['--fwd', 'bf16']).fwd == 'bf16'
    with pytest.raises(SystemExit):
        drv.parse_args(['--fwd', 'fp8'])
    drv.check_supported('camvid', '/nowhere', fwd='bf16')
    drv.check_supported('camvid', '/nowhere', wgrad='bf16', deconv='bf16', fwd='bf16')
    drv.check_supported('camvid', '/nowhere', dtype='float64', fwd='f32')
    with pytest.raises(NotImplementedError, match='fwd'):
        drv.check_supported('camvid', '/nowhere', dtype='float64', fwd='bf16')
    with pytest.raises(ValueError, match='fwd'):
        drv.check_supported('camvid', '/nowhere', fwd='tf32')
    # appended last: the positions of the earlier arguments are what they were
    import inspect
    assert list(inspect.signature(drv.check_supported).parameters)[-3:] == ['wgrad', 'deconv', 'fwd']
    assert list(inspect.signature(drv.train).parameters)[-3:] == ['wgrad', 'deconv', 'fwd']


def test_driver_refuses_float64_with_bf16_before_the_gpu(tmp_path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES='')
    env.pop('IISEG_SAVEPATH', None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_fcdensenet.py'), '--synthetic', '--savepath',
                        str(tmp_path / 'out'), '--dtype', 'float64', '--fwd', 'bf16'], cwd=ROOT, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 2, (r.stdout, r.stderr)
    assert r.stderr.startswith('train_fcdensenet.py: ') and "fwd='bf16'" in r.stderr and 'float32' in r.stderr
    assert 'Traceback' not in r.stderr
    assert not os.listdir(str(tmp_path))                   # nothing created


def test_op_refuses_before_the_library_is_touched(monkeypatch):
    """Host tensors; `_lib.load` is replaced by a function that fails the test if it is reached."""
    import torch
    from iterative_inference_segm_amd import _lib, ops

    def reached():
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'load', reached)
    B, cap, n, Cout, H, W = 2, 12, 5, 4, 6, 7
    stack = torch.zeros((B, cap, H, W))
    v = torch.zeros(cap)
    bn = (v, v, v, v)
    Wt, b = torch.zeros((Cout, n, 3, 3)), torch.zeros(Cout)
    keep = torch.ones((B, Cout, H, W))
    f = ops.bnrelu_conv_fwd
    # float32 tensors only
    for bad in (dict(stack=stack.double()), dict(W=Wt.double()), dict(b=b.double()), dict(b=None), dict(W=Wt.numpy()),
                dict(bn=(v, v.double(), v, v)), dict(keep=keep.double()), dict(out=stack.double(), out_c0=n)):
        kw = dict(stack=stack, n=n, bn=bn, W=Wt, b=b)
        kw.update(bad)
        with pytest.raises(ValueError, match='float32'):
            f(**kw)
    with pytest.raises(ValueError, match='beta, gamma, mean, inv_std'):
        f(stack, n, (v, v, v), Wt, b)
    # shapes
    for bad_n in (0, cap + 1):
        with pytest.raises(ValueError, match='stack'):
            f(stack, bad_n, bn, Wt, b)
    with pytest.raises(ValueError, match='stack'):
        f(stack[0], n, bn, Wt, b)
    for badW in (torch.zeros((Cout, n + 1, 3, 3)), torch.zeros((Cout, n, 3, 2)), torch.zeros((Cout, n, 5, 5)),
                 torch.zeros((n, 3, 3))):
        with pytest.raises(ValueError, match='W'):
            f(stack, n, bn, badW, b)
    with pytest.raises(ValueError, match='b '):
        f(stack, n, bn, Wt, torch.zeros(Cout + 1))
    with pytest.raises(ValueError, match='gamma'):
        f(stack, n, (v, torch.zeros(n - 1), v, v), Wt, b)
    # where the result goes
    with pytest.raises(ValueError, match='overlap'):
        f(stack, n, bn, Wt, b, out=stack, out_c0=n - 1)
    with pytest.raises(ValueError, match='overlap'):
        f(stack, n, bn, Wt, b, out=stack, out_c0=0)
    with pytest.raises(ValueError, match='out'):
        f(stack, n, bn, Wt, b, out=stack, out_c0=cap - Cout + 1)
    with pytest.raises(ValueError, match='out'):
        f(stack, n, bn, Wt, b, out=torch.zeros((B, Cout, H, W + 1)))
    with pytest.raises(ValueError, match='out_c0'):
        f(stack, n, bn, Wt, b, out_c0=2)
    # the mask and p
    for bad_keep in (torch.ones((B, Cout + 1, H, W)), torch.ones((B, Cout, H)), torch.ones((1, Cout, H, W))):
        with pytest.raises(ValueError, match='keep'):
            f(stack, n, bn, Wt, b, keep=bad_keep, p=0.2)
    for bad_p in (-0.1, 1.0, 1.5, float('nan')):
        with pytest.raises(ValueError, match='p = '):
            f(stack, n, bn, Wt, b, keep=keep, p=bad_p)
    # contiguity, and at last the device
    with pytest.raises(ValueError, match='contiguous'):
        f(torch.zeros((B, cap, W, H)).transpose(2, 3), n, bn, Wt, b)
    with pytest.raises(ValueError, match='contiguous'):
        f(stack, n, bn, torch.zeros((Cout, n + 2, 3, 3))[:, :n], b)
    with pytest.raises(ValueError, match='device tensor'):
        f(stack, n, bn, Wt, b, out=stack, out_c0=n, keep=keep, p=0.2)


def _desc(B=2, cap=40, n=17, Cout=16, H=7, W=9, out_cap=None, out_c0=0):
    from iterative_inference_segm_amd import ops
    return ops.bnrelu_conv_desc((B, cap, H, W), n, Cout, out_cap, out_c0)


def test_status_codes_without_a_gpu(built_lib):
    from iterative_inference_segm_amd import _lib
    lib = _lib.load()
    run = lambda d, ptrs, p=0.0: lib.iiseg_bnrelu_conv_fwd_bf16(None, d, *ptrs[:8], p, *ptrs[8:])
    assert lib.iiseg_bnrelu_conv_fwd_bf16_check(None) == ERR_NULL
    assert lib.iiseg_bnrelu_conv_fwd_bf16_slabs(None) == ERR_NULL
    assert lib.iiseg_bnrelu_conv_fwd_bf16_workspace_elems(None) == ERR_NULL
    assert run(None, [P] * 10) == ERR_NULL
    d = _desc()
    assert lib.iiseg_bnrelu_conv_fwd_bf16_check(C.byref(d)) == OK
    for i in (0, 1, 2, 3, 4, 5, 6, 9):                    # x, the BatchNorm vectors, W, bias, z (keep, ws may be NULL)
        ptrs = [P] * 10
        ptrs[i] = None
        assert run(C.byref(d), ptrs) == ERR_NULL, i
    for kw in (dict(B=0), dict(n=0), dict(Cout=0), dict(H=0), dict(W=0), dict(n=41), dict(out_c0=-1),
               dict(out_cap=20, out_c0=5), dict(cap=70000, n=5), dict(B=70000), dict(H=1 << 15, W=1 << 14)):
        bad = _desc(**kw)
        assert lib.iiseg_bnrelu_conv_fwd_bf16_check(C.byref(bad)) == ERR_SHAPE, kw
        assert lib.iiseg_bnrelu_conv_fwd_bf16_slabs(C.byref(bad)) == ERR_SHAPE, kw
        assert lib.iiseg_bnrelu_conv_fwd_bf16_workspace_elems(C.byref(bad)) == ERR_SHAPE, kw
        assert run(C.byref(bad), [P] * 10) == ERR_SHAPE, kw
    for p in (-0.5, 1.0, float('nan')):
        assert run(C.byref(d), [P] * 10, p) == ERR_SHAPE, p
    # z inside the stack: behind the channels that are read, or refused
    far = lambda k: C.c_void_p((k + 1) << 28)
    ptrs = [far(0)] + [far(1 + i) for i in range(9)]
    inside = _desc(out_cap=40, out_c0=16)
    ptrs[9] = ptrs[0]
    assert run(C.byref(inside), ptrs) == ERR_UNSUPPORTED
    ptrs[9] = ptrs[5]                                      # z on W
    assert run(C.byref(d), ptrs) == ERR_UNSUPPORTED
    ptrs[9] = ptrs[7]                                      # z on keep
    assert run(C.byref(d), ptrs) == ERR_UNSUPPORTED


def test_slab_rule_is_a_function_of_the_layer_and_never_of_the_batch(built_lib):
    from iterative_inference_segm_amd import _lib
    lib = _lib.load()
    slabs = lambda **kw: lib.iiseg_bnrelu_conv_fwd_bf16_slabs(C.byref(_desc(**kw)))
    elems = lambda **kw: lib.iiseg_bnrelu_conv_fwd_bf16_workspace_elems(C.byref(_desc(**kw)))
    for n, H, W in ((48, 224, 224), (240, 224, 224), (17, 7, 9), (1, 1, 1), (64, 7, 7)):
        assert slabs(cap=n, n=n, H=H, W=W) == 1 and elems(cap=n, n=n, H=H, W=W) == 0, (n, H, W)
    for n, H, W in ((1072, 7, 7), (1072, 14, 13), (300, 7, 7), (130, 14, 13), (656, 28, 28)):
        k = [slabs(B=B, cap=n, n=n, H=H, W=W) for B in (1, 3, 10)]
        assert k[0] >= 2 and k[0] == k[1] == k[2], (n, H, W, k)
        assert elems(B=3, cap=n, n=n, H=H, W=W) == k[0] * 3 * 16 * H * W
        assert k[0] <= (n + 31) // 32
    # a NULL workspace with several slabs
    d = _desc(B=1, cap=1072, n=1072, H=7, W=7)
    assert lib.iiseg_bnrelu_conv_fwd_bf16(None, C.byref(d), *[P] * 8, 0.0, None, P) == ERR_NULL
