"""GPU: fwd='bf16' on FC-DenseNet -- the dense-block layer's BatchNorm + ReLU + 3x3 convolution +
bias + dropout mask as one launch on the 16-bit matrix pipe (csrc/bnrelu_conv_bf16.hip, ops.bnrelu_conv_fwd) and the
switch through FCDenseNet, the trainer and train_fcdensenet.py.  The kernel: exact on data bf16 holds exactly, over
every shape at which it takes another path, with nothing written outside its slice; y pinned to bn_relu's bits; on real
data within the any-order fp32 accumulation bound of the float64 sum over operands rounded on the CPU
(tests/densenet_fwd_bf16_ref.py), ties included, and far outside the bound of the unrounded sum; mask and scale as
dropout_apply's; the same bits twice and for every batch size.  The module: one launch per dense-block layer, nothing
else changes.

Measured on an MI355X (for the record; the assertions are the derived bounds): see DESIGN.md section 25."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import densenet_fwd_bf16_ref as F
import densenet_train_ref as R
from kxk_bf16_ref import bf16

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = torch.float32
SENTINEL = -77.0


def _dev(a, dt=F32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda().contiguous()


def _conv64(t, W, b):
    """float64 zero-padded 3x3 correlation + bias (torch on the CPU: exact on small integers in any order)."""
    return torch.nn.functional.conv2d(torch.from_numpy(np.ascontiguousarray(t, np.float64)),
                                      torch.from_numpy(np.ascontiguousarray(W, np.float64)),
                                      torch.from_numpy(np.ascontiguousarray(b, np.float64)), padding=1).numpy()


def _slabs(B, cap, n, Cout, H, W):
    from iterative_inference_segm_amd import _lib, ops
    return _lib.load().iiseg_bnrelu_conv_fwd_bf16_slabs(C.byref(ops.bnrelu_conv_desc((B, cap, H, W), n, Cout)))


# ---- 1. exact on small integers, nothing else written ----
CHANNELS = [(1, 16), (5, 16), (16, 16), (17, 16), (33, 16), (48, 16), (67, 16), (24, 4), (24, 11), (20, 33)]
GEOMETRY = [(1, 1), (2, 9), (7, 7), (14, 13), (37, 150)]
DEEP = [(130, 16), (300, 16), (1072, 16)]                       # many k-tiles, slabs: the small maps only
INT_CASES = [(n, co, h, w) for n, co in CHANNELS for h, w in GEOMETRY] + \
            [(n, co, h, w) for n, co in DEEP for h, w in ((7, 7), (14, 13))]


def _int_case(n, Cout, B, H, W):
    rng = np.random.default_rng(n * 1000 + Cout + 7 * B + 31 * H + W)
    x = rng.integers(-3, 4, size=(B, n, H, W)).astype(np.float64)
    mean = rng.integers(-1, 2, size=n).astype(np.float64)
    inv_std = 2.0 ** rng.integers(-1, 2, size=n)
    gamma = rng.integers(1, 3, size=n).astype(np.float64)
    beta = rng.integers(1, 3, size=n).astype(np.float64)         # positive: BN(0) on the ring would be seen
    Wt = rng.integers(-2, 3, size=(Cout, n, 3, 3)).astype(np.float64)
    b = rng.integers(-3, 4, size=Cout).astype(np.float64)
    keep = rng.integers(0, 2, size=(B, Cout, H, W)).astype(np.float64)
    t = F.bn_relu(x, beta, gamma, mean, inv_std)
    assert np.array_equal(bf16(t), t) and t.max() > 0
    z = _conv64(t, Wt, b)
    assert np.abs(z).max() < 2 ** 22
    return x, (beta, gamma, mean, inv_std), Wt, b, keep, z


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('n,Cout,H,W', INT_CASES)
def test_exact_on_integers_and_writes_nothing_else(built_lib, n, Cout, B, H, W):
    from iterative_inference_segm_amd import ops
    x, bn, Wt, b, keep, z = _int_case(n, Cout, B, H, W)
    cap = n + Cout + 5
    if (n, H, W, B) == (1072, 7, 7, 1):
        assert _slabs(B, cap, n, Cout, H, W) >= 2
    stack = torch.full((B, cap, H, W), SENTINEL, dtype=F32, device='cuda')
    stack[:, :n] = _dev(x)
    bnd = tuple(_dev(v) for v in bn)
    Wd, bd, kd = _dev(Wt), _dev(b), _dev(keep)
    r = ops.bnrelu_conv_fwd(stack, n, bnd, Wd, bd, out=stack, out_c0=n, keep=kd, p=0.5)
    assert r is stack
    dense = ops.bnrelu_conv_fwd(stack, n, bnd, Wd, bd)            # no mask, a new dense tensor
    torch.cuda.synchronize()
    got = stack.cpu().double().numpy()
    assert np.array_equal(got[:, :n], x)                           # what was read is what it was
    assert (got[:, n + Cout:] == SENTINEL).all()                   # behind the slice: untouched
    assert np.array_equal(got[:, n:n + Cout], z * keep * 2.0), np.abs(got[:, n:n + Cout] - z * keep * 2.0).max()
    assert tuple(dense.shape) == (B, Cout, H, W) and dense.dtype == F32
    assert np.array_equal(dense.cpu().double().numpy(), z)


# ---- 2. the BatchNorm expression and the gate are bn_relu's, bit for bit ----
@pytest.mark.parametrize('n', [5, 67])
def test_y_and_the_gate_are_bn_relus_bits(built_lib, n):
    from iterative_inference_segm_amd import ops
    B, H, W = 2, 9, 35
    rng = np.random.default_rng(40 + n)
    x = _dev(rng.standard_normal((B, n + 3, H, W)) * 1.7 + 0.4)
    beta, gamma = _dev(rng.uniform(-0.5, 0.5, n)), _dev(rng.uniform(0.5, 1.5, n))
    mean, inv_std = _dev(rng.uniform(-0.3, 0.7, n)), _dev(rng.uniform(0.4, 1.1, n))
    t = ops.bn_relu(x, n, beta, gamma, mean, inv_std)
    want = t.cpu().to(torch.bfloat16).to(F32)                      # rounded on the CPU
    assert 0.2 < float((want == 0).float().mean()) < 0.8           # both sides of the gate
    zero = torch.zeros(16, dtype=F32, device='cuda')
    for c0 in range(0, n, 16):
        k = min(16, n - c0)
        Wt = torch.zeros((16, n, 3, 3), dtype=F32)
        for co in range(k):
            Wt[co, c0 + co, 1, 1] = 1.0
        z = ops.bnrelu_conv_fwd(x, n, (beta, gamma, mean, inv_std), Wt.cuda(), zero).cpu()
        assert torch.equal(z[:, :k], want[:, c0:c0 + k]), (c0, float((z[:, :k] - want[:, c0:c0 + k]).abs().max()))
        assert not bool(z[:, k:].any())


# ---- 3. the rounding point, ties, direction ----
def test_rounded_sum_inside_the_bound_unrounded_sum_outside(built_lib):
    from iterative_inference_segm_amd import ops
    Wt, b, x, beta, gamma, mean, inv_std = F.rounding_case()
    n = x.shape[1]
    xd, bnd = _dev(x), tuple(_dev(v) for v in (beta, gamma, mean, inv_std))
    t = ops.bn_relu(xd, n, *bnd).cpu().double().numpy()            # the GPU's own fp32 t, rounded below on the CPU
    z = ops.bnrelu_conv_fwd(xd, n, bnd, _dev(Wt), _dev(b)).cpu().double().numpy()
    ref, unr, bd = F.layer(Wt, b, t), F.layer(Wt, b, t, rounded=False), F.bound(Wt, b, t)
    err = np.abs(z - ref)
    outside = float((np.abs(z - unr) > bd).mean())
    print('17 -> 16 at 7 x 9: worst error / bound %.3f; outside the unrounded sum\'s bound: %.3f of the entries'
          % (float((err / bd).max()), outside))
    assert (err <= bd).all(), float((err / bd).max())
    assert outside > 0.9, outside


TIE_CHANNELS = (0, 9, 18, 27, 35)                                 # one per 8-channel chunk of k-tile 0; the ragged k-tile
TIE_PIXELS = ((2, 3), (5, 20))                                    # a pixel in each half of a 32-column tile


def test_ties_in_W_round_to_even(built_lib):
    from iterative_inference_segm_amd import ops
    n, Cout, H, W = 37, 16, 8, 40
    one = torch.ones(n, dtype=F32, device='cuda')
    zero = torch.zeros(n, dtype=F32, device='cuda')
    bn = (zero, one, zero, one)                                    # beta 0, gamma 1, mean 0, inv_std 1: t = relu(x)
    b = np.zeros(Cout)
    for c in TIE_CHANNELS:
        for (i, j) in TIE_PIXELS:
            x = np.zeros((1, n, H, W))
            x[0, c, i, j] = 1.0                                    # a single unit pixel of t
            Wt = np.zeros((Cout, n, 3, 3))
            Wt[:, c] = np.resize(F.TIES.astype(np.float64), (Cout, 3, 3))
            z = ops.bnrelu_conv_fwd(_dev(x), n, bn, _dev(Wt), _dev(b)).cpu().double().numpy()
            ref = F.layer(Wt, b, x)                                # one product per entry: exact
            assert np.abs(ref).max() > 1 and not np.array_equal(ref, F.layer(Wt, b, x, rounded=False))
            assert np.array_equal(z, ref), (c, i, j)


def test_ties_in_t_round_to_even(built_lib):
    from iterative_inference_segm_amd import ops
    n, Cout, H, W = 37, 16, 8, 40
    one = torch.ones(n, dtype=F32, device='cuda')
    zero = torch.zeros(n, dtype=F32, device='cuda')
    ties = F.TIES[F.TIES > 0].astype(np.float64)
    b = np.zeros(Cout)
    for c in TIE_CHANNELS:
        x = np.zeros((1, n, H, W))
        for k, (i, j) in enumerate(TIE_PIXELS):
            x[0, c, i, j:j + len(ties)] = np.roll(ties, k)
        Wt = np.zeros((Cout, n, 3, 3))
        Wt[3, c, 1, 1] = 1.0
        z = ops.bnrelu_conv_fwd(_dev(x), n, (zero, one, zero, one), _dev(Wt), _dev(b)).cpu().double().numpy()
        assert not np.array_equal(bf16(x[:, c]), x[:, c])
        assert np.array_equal(z[:, 3], bf16(x[:, c])), c
        assert not z[:, :3].any() and not z[:, 4:].any()


# ---- 4. mask and scale, the same bits twice, the batch ----
@pytest.mark.parametrize('n,H,W', [(17, 7, 9), (67, 14, 13), (40, 9, 70)])
def test_mask_scale_determinism_and_batch_invariance(built_lib, n, H, W):
    from iterative_inference_segm_amd import ops
    B, Cout, p = 3, 16, 0.2
    rng = np.random.default_rng(n + H)
    x = _dev(rng.standard_normal((B, n, H, W)) + 0.2)
    bn = tuple(_dev(v) for v in (rng.uniform(-0.2, 0.2, n), rng.uniform(0.7, 1.3, n), rng.uniform(-0.1, 0.5, n),
                                 rng.uniform(0.6, 1.2, n)))
    Wt, b = _dev(rng.standard_normal((Cout, n, 3, 3)) * np.sqrt(2.0 / (9 * n))), _dev(rng.uniform(-0.1, 0.1, Cout))
    keep = _dev((rng.random((B, Cout, H, W)) >= p).astype(np.float64))
    if n == 67:
        assert _slabs(B, n, n, Cout, H, W) >= 2                   # the finalize launch's expression too
    else:
        assert _slabs(B, n, n, Cout, H, W) == 1
    fused = ops.bnrelu_conv_fwd(x, n, bn, Wt, b, keep=keep, p=p)
    plain = ops.bnrelu_conv_fwd(x, n, bn, Wt, b)
    assert not torch.equal(fused, plain)
    assert torch.equal(fused, ops.dropout_apply(plain.clone(), keep, p))
    assert torch.equal(fused, ops.bnrelu_conv_fwd(x, n, bn, Wt, b, keep=keep, p=p))
    first = ops.bnrelu_conv_fwd(x[:1].contiguous(), n, bn, Wt, b, keep=keep[:1].contiguous(), p=p)
    assert torch.equal(first[0], fused[0])


# ---- 5. the module ----
CASES = {'thin': R.THIN, 'wide': R.WIDE}
_CASES, _RUNS = {}, {}


def _model_case(name):
    if name not in _CASES:
        _CASES[name] = R.make_case(CASES[name], seed=3)
    return _CASES[name]


def _net(name, params=None, **kw):
    from iterative_inference_segm_amd.densenet import FCDenseNet
    cfg = CASES[name]
    return FCDenseNet(_model_case(name)[0] if params is None else params, cfg['n_classes'], layer=[],
                      n_layers_per_block=cfg['nlpb'], n_pool=cfg['n_pool'], growth=cfg['growth'], dtype=F32, mma='f32',
                      trainable=True, **kw)


def _grads_as_ref(net, gv):
    out = []
    for li, L in enumerate(net.layers):
        q = dict(W=gv['conv%03d' % li][0], b=gv['conv%03d' % li][1])
        if L['kind'] in ('brc', 'td'):
            q['gamma'], q['beta'] = gv['bn%03d' % li]
        out.append({k: v.cpu().numpy().astype(np.float64) for k, v in q.items()})
    return out


def _run(name, **kw):
    """(net, score, gflat copy, grads) of one forward_train + backward with the case's masks; once per mode, shared."""
    from iterative_inference_segm_amd import ops
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _RUNS:
        params, x, T, keeps = _model_case(name)
        net = _net(name, **kw)
        score = net.forward_train(_dev(x), [_dev(k) for k in keeps])
        res, g, _ = ops.ctx_loss(score, _dev(T), ('crossentropy',), 1.0)
        gv = net.backward(g)
        torch.cuda.synchronize()
        _RUNS[key] = (net, score.clone(), net.gflat.clone(), _grads_as_ref(net, gv))
    return _RUNS[key]


@pytest.mark.parametrize('name', list(CASES))
def test_f32_mode_is_the_module_without_the_keyword(built_lib, name):
    a, b = _run(name), _run(name, fwd='f32')
    assert a[0].fwd == b[0].fwd == 'f32'
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


@pytest.mark.parametrize('name', list(CASES))
def test_one_fused_launch_per_dense_block_layer(built_lib, name, monkeypatch):
    from iterative_inference_segm_amd import ops
    from iterative_inference_segm_amd.train import DenseNetTrainer
    cfg = CASES[name]
    params, x, T, keeps = _model_case(name)
    steps = R.program(cfg)[0]
    n_brc, n_td = (sum(1 for e in steps if e['kind'] == k) for k in ('brc', 'td'))
    calls = dict(fused=[], bn_relu=0, dropout=0)
    real_fused, real_bn, real_drop = ops.bnrelu_conv_fwd, ops.bn_relu, ops.dropout_apply

    def fused(stack, n, bn, W, b, out=None, out_c0=0, keep=None, p=0.0):
        calls['fused'].append((n, out is stack, out_c0, keep is not None, p))
        return real_fused(stack, n, bn, W, b, out=out, out_c0=out_c0, keep=keep, p=p)

    def bn_relu(*a, **k):
        calls['bn_relu'] += 1
        return real_bn(*a, **k)

    def dropout(*a, **k):
        calls['dropout'] += 1
        return real_drop(*a, **k)
    monkeypatch.setattr(ops, 'bnrelu_conv_fwd', fused)
    monkeypatch.setattr(ops, 'bn_relu', bn_relu)
    monkeypatch.setattr(ops, 'dropout_apply', dropout)
    net = _net(name, fwd='bf16')
    net.forward_train(_dev(x), [_dev(k) for k in keeps])
    want_n = [e['n'] for e in steps if e['kind'] == 'brc']
    assert [c[0] for c in calls['fused']] == want_n and len(want_n) == n_brc
    assert all(c[1] and c[2] == c[0] and c[3] and c[4] == net.dropout for c in calls['fused'])
    assert calls['bn_relu'] == n_td and calls['dropout'] == n_td  # TransitionDown only
    # the deterministic forward and val_fn: the same kernel, no mask
    calls.update(fused=[], bn_relu=0, dropout=0)
    net.forward_train(_dev(x), deterministic=True)
    assert [c[0] for c in calls['fused']] == want_n and not any(c[3] for c in calls['fused'])
    assert calls['bn_relu'] == n_td and calls['dropout'] == 0
    calls.update(fused=[], bn_relu=0, dropout=0)
    tr = DenseNetTrainer(net, cfg['n_classes'], [cfg['n_classes']])
    loss, _ = tr.val_step(_dev(x), _dev(T))
    assert len(calls['fused']) == n_brc and bool(torch.isfinite(loss))
    # the 'f32' mode never reaches it
    calls.update(fused=[], bn_relu=0, dropout=0)
    _net(name).forward_train(_dev(x), [_dev(k) for k in keeps])
    assert not calls['fused'] and calls['bn_relu'] == n_brc + n_td


@pytest.mark.parametrize('name', list(CASES))
def test_every_dense_block_layer_teacher_forced_within_its_bound(built_lib, name):
    from iterative_inference_segm_amd import ops
    cfg = CASES[name]
    keeps = _model_case(name)[3]
    net, f32net = _run(name, fwd='bf16')[0], _run(name)[0]
    n0, g = cfg['n_first'], cfg['growth']
    s, s32 = net.saved_maps(), f32net.saved_maps()
    assert torch.equal(s['stacks'][0][:, :n0], s32['stacks'][0][:, :n0])       # the first layer: the same launch
    assert not torch.equal(s['stacks'][0][:, n0:], s32['stacks'][0][:, n0:])
    worst = 0.0
    for e in R.program(cfg)[0]:
        if e['kind'] != 'brc':
            continue
        L, n, sid = net.layers[e['li']], e['n'], e['sid']
        stack = s['stacks'][sid]
        # the GPU's own saved stack, statistics and mask; t as bn_relu forms it, rounded on the CPU
        t = ops.bn_relu(stack, n, L['beta'], L['gamma'], s['mean'][sid], s['inv_std'][sid]).cpu().double().numpy()
        Wt, b = L['conv'].W.cpu().double().numpy(), L['conv'].b.cpu().double().numpy()
        keep = s['keeps'][e['ki']].cpu().double().numpy()
        assert np.array_equal(keep, keeps[e['ki']])
        ref, bd = F.layer(Wt, b, t, keep, net.dropout), F.bound(Wt, b, t, keep, net.dropout)
        err = np.abs(stack[:, n:n + g].cpu().double().numpy() - ref)
        assert (err <= bd).all(), (e['li'], float((err / bd).max()))
        worst = max(worst, float((err / bd).max()))
    print('%s: worst error / bound over the dense-block layers %.4f' % (name, worst))


@pytest.mark.parametrize('name', list(CASES))
def test_gradients_against_the_f32_mode(built_lib, name):
    """Per gradient array (dead ones left out): 1 - cosine between the modes at most 2 x the same quantity between
    the rounded and the unrounded float64 restatement on the same case, plus 1e-6 (the factor covers ReLU and pool
    decisions that flip on rounded operands)."""
    cfg = CASES[name]
    params, x, T, keeps = _model_case(name)
    ref = {}
    for rounded in (False, True):
        s = F.forward(params, x, cfg, keeps, 0.2, rounded=rounded)
        ref[rounded] = R.backward(params, s, R.loss_and_grad(s['score'], T)[3], cfg)
    want = F.one_minus_cosines(ref[True], ref[False], cfg)
    got = F.one_minus_cosines(_run(name, fwd='bf16')[3], _run(name)[3], cfg)
    assert sorted(got) == sorted(want)
    worst = max(got, key=lambda k: got[k] / (2 * want[k] + 1e-6))
    print('%s: 1 - cosine between the modes: largest %.3g (restatement %.3g); closest to its limit %s: %.3g against '
          '2 x %.3g + 1e-6' % (name, max(got.values()), max(want.values()), worst, got[worst], want[worst]))
    for k in want:
        assert got[k] <= 2 * want[k] + 1e-6, (k, got[k], want[k])


def test_training_is_deterministic_refresh_leaves_no_stale_weights_and_the_loss_goes_down(built_lib, tmp_path):
    from iterative_inference_segm_amd.densenet import layer_plan, load_params, save_checkpoint
    from iterative_inference_segm_amd.train import DenseNetTrainer
    cfg = R.THIN
    params, x, T, keeps = _model_case('thin')
    xd, Td, kd = _dev(x), _dev(T), [_dev(k) for k in keeps]
    C_ = cfg['n_classes']
    flats = []
    for _ in range(2):
        tr = DenseNetTrainer(_net('thin', fwd='bf16'), C_, [C_], learning_rate=1e-2, weight_decay=1e-4, seed=3)
        tr.train_step(xd, Td, kd)
        tr.train_step(xd, Td)                                      # masks from the seeded generator
        torch.cuda.synchronize()
        flats.append(tr.net.flat.clone())
    assert torch.equal(flats[0], flats[1]) and bool(torch.isfinite(flats[0]).all())
    assert not torch.equal(flats[0], _dev(R.flatten(params)))
    # after the optimizer step and refresh(): the forward of a module freshly built on the new parameters
    path = str(tmp_path / 'w.npz')
    save_checkpoint(path, tr.net, cfg['n_first'])
    plan = layer_plan(cfg['nlpb'], cfg['n_pool'], cfg['growth'], cfg['n_first'], 3, C_)
    again = _net('thin', params=load_params(path, plan), fwd='bf16')
    assert torch.equal(again.flat, tr.net.flat)
    assert torch.equal(again.forward_train(xd, deterministic=True), tr.net.forward_train(xd, deterministic=True))
    assert torch.equal(again.forward_train(xd, kd), tr.net.forward_train(xd, kd))
    # test_loss_goes_down_over_40_steps_f32's assertion, in this mode
    tr = DenseNetTrainer(_net('thin', fwd='bf16'), C_, [C_], learning_rate=1e-3, seed=2)
    losses = [tr.train_step(xd, Td) for _ in range(40)]
    losses = [float(v) for v in torch.stack(losses).cpu()]
    print('fwd=bf16 loss, steps 0-9: %.5f, steps 30-39: %.5f' % (np.mean(losses[:10]), np.mean(losses[-10:])))
    assert np.all(np.isfinite(losses))
    assert np.mean(losses[-10:]) < np.mean(losses[:10])


def test_all_three_switches_together(built_lib):
    from iterative_inference_segm_amd.train import DenseNetTrainer
    cfg = R.WIDE
    params, x, T, keeps = _model_case('wide')
    C_ = cfg['n_classes']
    got = _run('wide', fwd='bf16', wgrad='bf16', deconv='bf16')
    assert (got[0].fwd, got[0].wgrad, got[0].deconv) == ('bf16', 'bf16', 'bf16')
    assert torch.equal(got[1], _run('wide', fwd='bf16')[1])        # the forward is the fwd switch's alone
    cos = F.one_minus_cosines(got[3], _run('wide')[3], cfg)
    print('all three switches: largest 1 - cosine to the f32 mode %.3g' % max(cos.values()))
    assert max(cos.values()) < 1e-2
    tr = DenseNetTrainer(_net('wide', fwd='bf16', wgrad='bf16', deconv='bf16'), C_, [C_], learning_rate=1e-3, seed=2)
    xd, Td = _dev(x), _dev(T)
    losses = [float(v) for v in torch.stack([tr.train_step(xd, Td) for _ in range(10)]).cpu()]
    assert np.all(np.isfinite(losses)) and losses[-1] < losses[0]


# ---- 6. the driver ----
def test_driver_end_to_end(built_lib, tmp_path):
    from iterative_inference_segm_amd.densenet import build_fcdensenet
    save = str(tmp_path / 'save')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_fcdensenet.py'), '--synthetic', '--num_epochs', '2',
                        '--n_images', '2', '--image_size', '16', '16', '--batch_size', '[2, 2, 2]', '--savepath', save,
                        '--layers_per_block', '[2, 3, 2, 3, 2]', '--growth', '4', '--n_first', '8',
                        '--max_batches', '1', '--fwd', 'bf16'], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    folder = os.path.join(save, 'camvid', 'fc_densenet')
    files = os.listdir(folder)
    assert 'FC-DenseNet103_weights_best.npz' in files and 'output.log' in files and 'config.txt' in files
    config = open(os.path.join(folder, 'config.txt')).read()
    assert 'fwd = bf16' in config and 'wgrad = f32' in config
    assert len(open(os.path.join(folder, 'output.log')).read().splitlines()) == 2
    net = build_fcdensenet(layer=[], n_classes=11, weight_path=os.path.join(folder, 'FC-DenseNet103_weights_best.npz'))
    probs = net(_dev(np.random.default_rng(1).random((2, 3, 16, 16))))[-1]
    assert tuple(probs.shape) == (2, 11, 16, 16) and bool(torch.isfinite(probs).all())
