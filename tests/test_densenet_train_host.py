"""CPU (no launch): the host side of FC-DenseNet training -- status codes of the two new entry points, the driver's
defaults and refusals, the module's refusals, the flat buffer's order and `state_list()` against `layer_plan` /
`load_params` on host tensors."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OK, ERR_NULL, ERR_SHAPE, ERR_UNSUPPORTED = 0, -1, -2, -5
P = C.c_void_p(16)          # a non-NULL pointer no check dereferences: every call below fails before a launch
THIN = dict(n_layers_per_block=[2, 3, 2, 3, 2], n_pool=2, growth=4)


@pytest.fixture(scope='module')
def lib(built_lib):
    from iterative_inference_segm_amd import _lib
    return _lib.load()


def test_bn_relu_bwd_status_codes(lib):
    from iterative_inference_segm_amd import _lib
    both = _lib.BN_BWD_REDUCE | _lib.BN_BWD_APPLY
    for fn in (lib.iiseg_bn_relu_bwd_f32, lib.iiseg_bn_relu_bwd_f64):
        good = [P, 11 * 6, P, P, 2, 5, 6] + [P] * 7 + [both]        # x, bstride, g_t, gstack, B, C, HW, 7 pointers
        for i, a in enumerate(good):
            if a is P:
                bad = list(good)
                bad[i] = None
                assert fn(None, *bad) == ERR_NULL, i
        for i in (4, 5, 6):                                          # B, C, HW
            for v in (0, -2):
                bad = list(good)
                bad[i] = v
                assert fn(None, *bad) == ERR_SHAPE, (i, v)
        bad = list(good)
        bad[1] = 5 * 6 - 1                                           # images closer than C planes
        assert fn(None, *bad) == ERR_SHAPE
        for stages in (0, 4, 7):
            assert fn(None, *(good[:-1] + [stages])) == ERR_UNSUPPORTED
        bad = list(good)
        bad[5], bad[1] = 65536, 65536 * 6
        assert fn(None, *bad) == ERR_UNSUPPORTED
    assert lib.iiseg_bn_relu_bwd_workspace_elems(0, 6) == ERR_SHAPE
    assert lib.iiseg_bn_relu_bwd_workspace_elems(5, 0) == ERR_SHAPE
    assert lib.iiseg_bn_relu_bwd_workspace_elems(5, 6) == 2 * 5      # one chunk per channel on a small plane
    # a 224 x 224 plane: many chunks at 16 channels, fewer at 1000 -- both two thousand workgroups
    hw = 224 * 224
    assert lib.iiseg_bn_relu_bwd_workspace_elems(16, hw) // (2 * 16) >= 32
    assert 2 <= lib.iiseg_bn_relu_bwd_workspace_elems(1000, hw) // (2 * 1000) <= 4


def test_maxpool2x2_bwd_status_codes(lib):
    for fn in (lib.iiseg_maxpool2x2_bwd_f32, lib.iiseg_maxpool2x2_bwd_f64):
        for i in range(4):
            ptrs = [P] * 4
            ptrs[i] = None
            assert fn(None, *ptrs, 3, 4, 4) == ERR_NULL
        for BC, H, W in ((0, 4, 4), (-1, 4, 4), (3, 1, 4), (3, 4, 1), (3, 0, 0)):
            assert fn(None, P, P, P, P, BC, H, W) == ERR_SHAPE


def _driver():
    sys.path.insert(0, ROOT)
    try:
        import train_fcdensenet
    finally:
        sys.path.remove(ROOT)
    return train_fcdensenet


def test_driver_defaults():
    from iterative_inference_segm_amd import densenet
    drv = _driver()
    a = drv.make_parser().parse_args([])
    assert a.dataset == 'camvid' and a.learning_rate == 1e-3 and a.lr_decay == 0.995 and a.weight_decay == 1e-4
    assert a.batch_size == [3, 1, 1] and a.optimizer == 'rmsprop' and a.dropout == 0.2 and a.dtype == 'float32'
    assert a.layers_per_block == densenet.LAYERS_PER_BLOCK and a.growth == densenet.GROWTH
    assert a.n_first == densenet.N_FILTERS_FIRST and a.image_size is None
    assert not a.synthetic and not a.resume and a.savepath is None
    assert drv.make_parser().parse_args(['-ne', '3']).num_epochs == 3
    plan = densenet.layer_plan([1, 1, 1], 1, 4, 8, 3, 5)
    p = drv.he_params(plan, 7)
    assert [q['kind'] for q in p] == [k for k, _, _ in plan]
    lim = (6.0 / (3 * 9)) ** 0.5
    assert abs(p[0]['W']).max() <= lim and abs(p[0]['W']).max() > 0.8 * lim and not p[0]['b'].any()
    assert (p[1]['gamma'] == 1).all() and not p[1]['beta'].any()
    assert (drv.he_params(plan, 7)[0]['W'] == p[0]['W']).all()


@pytest.mark.parametrize('argv,reason', [
    (['--synthetic'], 'saving directory'),
    (['--synthetic', '--savepath', '{tmp}/out', '--mma', 'bf16'], '16-bit'),
    (['--synthetic', '--savepath', '{tmp}/out', '--mma', 'bf16c8'], '16-bit'),
    (['--synthetic', '--savepath', '{tmp}/out', '--dtype', 'bfloat16'], '16-bit'),
    (['--synthetic', '--savepath', '{tmp}/out', '--optimizer', 'sgd'], 'Unknown optimizer'),
    (['--synthetic', '--savepath', '{tmp}/out', '--dropout', '1.0'], 'dropout'),
    (['--synthetic', '--savepath', '{tmp}/out', '--dropout', '-0.1'], 'dropout'),
    (['--synthetic', '--savepath', '{tmp}/out', '-dataset', 'nope'], 'Unknown dataset'),
    (['--synthetic', '--savepath', '{tmp}/out', '--batch_size', '[3, 0, 1]'], 'batch_size'),
    (['--synthetic', '--savepath', '{tmp}/out', '--layers_per_block', '[2, 2]'], 'layers_per_block'),
    (['--synthetic', '--savepath', '{tmp}/out', '--image_size', '16', '16'], 'too small'),
])
def test_driver_refuses_before_the_gpu(tmp_path, argv, reason):
    env = dict(os.environ, HIP_VISIBLE_DEVICES='')
    env.pop('IISEG_SAVEPATH', None)
    argv = [a.replace('{tmp}', str(tmp_path)) for a in argv]
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_fcdensenet.py')] + argv, cwd=ROOT, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 2, (r.stdout, r.stderr)
    assert reason in r.stderr and r.stderr.startswith('train_fcdensenet.py: ') and 'Traceback' not in r.stderr
    assert not os.listdir(str(tmp_path))                   # nothing created


def _thin_params(seed=5):
    from iterative_inference_segm_amd import synthetic as S
    from iterative_inference_segm_amd.densenet import layer_plan
    plan = layer_plan(THIN['n_layers_per_block'], THIN['n_pool'], THIN['growth'], 8, 3, 4)
    return plan, S.make_densenet_params(plan, seed=seed)


def test_trainable_module_refusals(built_lib):
    """At construction, with the reason, before any device work (host parameters, no GPU here)."""
    import torch
    from iterative_inference_segm_amd.densenet import FCDenseNet
    plan, params = _thin_params()
    for kw in (dict(mma='bf16c8'), dict(mma='bf16'), dict(mma='bf16x3'), dict(dtype=torch.bfloat16, mma='f32')):
        with pytest.raises(NotImplementedError, match='16-bit'):
            FCDenseNet(params, 4, trainable=True, device='cpu', **THIN, **kw)
    for p in (1.0, -0.5):
        with pytest.raises(ValueError, match='dropout'):
            FCDenseNet(params, 4, trainable=True, device='cpu', mma='f32', dropout=p, **THIN)
    from iterative_inference_segm_amd.train import DenseNetTrainer
    net = FCDenseNet(params, 4, device='cpu', mma='f32', **THIN)
    assert not net.trainable
    for what in (lambda: net.forward_train(None), net.refresh, net.state_list, lambda: net.backward(None)):
        with pytest.raises(RuntimeError, match='trainable=True'):
            what()
    with pytest.raises(NotImplementedError, match='trainable=True'):
        DenseNetTrainer(net, 4, [4])
    tnet = FCDenseNet(params, 4, trainable=True, device='cpu', mma='f32', **THIN)
    with pytest.raises(ValueError, match='Unknown optimizer'):
        DenseNetTrainer(tnet, 4, [4], optimizer='sgd')


def test_flat_buffer_and_state_list_order(built_lib, tmp_path):
    import torch
    from iterative_inference_segm_amd import densenet
    from iterative_inference_segm_amd.densenet import FCDenseNet
    plan, params = _thin_params()
    net = FCDenseNet(params, 4, trainable=True, device='cpu', mma='f32', dtype=torch.float64, **THIN)
    steps, caps = densenet.train_program(THIN['n_layers_per_block'], THIN['n_pool'], THIN['growth'], 8)
    assert [e['kind'] for e in steps] == [k for k, _, _ in plan]
    for e, (kind, cin, cout) in zip(steps, plan):
        if kind in ('brc', 'td', 'softmax'):
            assert e['n'] == cin
        if kind == 'tu':
            assert (e['n'] - e['block0'], e['keep']) == (cin, cout)
    # the flat buffer: creation order, a BatchNorm layer as (gamma, beta) in front of its convolution's (W, b)
    want = []
    for p in params:
        want += ([p['gamma'], p['beta']] if p['kind'] in ('brc', 'td') else []) + [p['W'], p['b']]
    assert np.array_equal(net.flat.numpy(), np.concatenate([np.asarray(a, np.float64).ravel() for a in want]))
    names = densenet.store_names([k for k, _, _ in plan])
    assert list(net.parameters()) == names and names[:3] == ['conv000', 'bn001', 'conv001']
    for e in net.layers:                                   # views, not copies
        assert net._params.holds(e['conv'].W) and net._params.holds(e['conv'].b)
        if e['kind'] in ('brc', 'td'):
            assert net._params.holds(e['gamma']) and net._params.holds(e['beta'])
    # weight_ranges: every W and every gamma, nothing else
    total = sum(hi - lo for lo, hi in net.weight_ranges())
    assert total == sum(p['W'].size + (p['gamma'].size if 'gamma' in p else 0) for p in params)
    lo0, hi0 = net.weight_ranges()[1]
    assert np.array_equal(net.flat[lo0:hi0].numpy(), params[1]['gamma'].astype(np.float64))
    # state_list: what load_params reads, with the running averages at their start (0, 1)
    arrays = net.state_list()
    path = str(tmp_path / 'w.npz')
    densenet.save_checkpoint(path, net, 8)
    back = densenet.load_params(path, plan)
    for p, q in zip(params, back):
        assert p['kind'] == q['kind']
        for f in ('beta', 'gamma', 'W', 'b'):
            if f in p:
                assert np.array_equal(q[f], p[f].astype(np.float32)), (p['kind'], f)
    i = 0
    for kind, cin, cout in plan:
        if kind in ('brc', 'td'):
            assert arrays[i + 2].shape == arrays[i + 3].shape == (cin,)
            assert not arrays[i + 2].any() and (arrays[i + 3] == 1).all()
            i += 4
        i += 2
    assert i == len(arrays)
    assert densenet.read_config(path) == dict(n_pool=2, growth=4, n_first=8, n_layers_per_block=[2, 3, 2, 3, 2])
    # a DenseNet103 checkpoint records nothing and reads as before
    np.savez(str(tmp_path / 'plain.npz'), *arrays)
    assert densenet.read_config(str(tmp_path / 'plain.npz')) is None
    assert len(densenet.load_params(str(tmp_path / 'plain.npz'), plan)) == len(plan)
