"""GPU: training FC-DenseNet -- the BatchNorm + ReLU backward with batch statistics and the
ungated max-pool adjoint (csrc/bn_grad.hip) at their edges; FCDenseNet.forward_train / backward / refresh, the
trainer and train_fcdensenet.py against the float64 restatement (tests/densenet_train_ref.py)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import densenet_train_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {'f32': torch.float32, 'f64': torch.float64}
NP = {'f32': np.float32, 'f64': np.float64}
SENTINEL = 777.0


def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda().contiguous()


# ---- 1. bn_relu_bwd ----
def _bn_operands(B, n, H, W, npdt, seed, gamma=None, beta=None):
    """Operands in the precision under test: the stack (cap = n + 6), its statistics over the first n channels, the
    consumer's (beta, gamma), g_t, and a gradient stack pre-filled with values (sentinel in channels >= n)."""
    rng = np.random.default_rng(seed)
    cap = n + 6
    x = (rng.standard_normal((B, cap, H, W)) * rng.uniform(0.5, 2.0, size=(1, cap, 1, 1)) +
         rng.uniform(-1, 1, size=(1, cap, 1, 1))).astype(npdt)
    x64 = x[:, :n].astype(np.float64)
    mean = np.zeros(cap, npdt)
    inv_std = np.ones(cap, npdt)
    mean[:n] = x64.mean(axis=(0, 2, 3))
    inv_std[:n] = 1.0 / np.sqrt(x64.var(axis=(0, 2, 3)) + 1e-4)
    q = dict(gamma=(rng.uniform(0.7, 1.3, size=n) if gamma is None else np.full(n, gamma)).astype(npdt),
             beta=(rng.uniform(-0.2, 0.2, size=n) if beta is None else np.full(n, beta)).astype(npdt))
    g_t = rng.standard_normal((B, n, H, W)).astype(npdt)
    gstack = rng.standard_normal((B, cap, H, W)).astype(npdt)
    gstack[:, n:] = SENTINEL
    return x, mean, inv_std, q, g_t, gstack


def _bn_run(prec, x, mean, inv_std, q, g_t, gstack, n):
    from iterative_inference_segm_amd import ops
    dt = DT[prec]
    xd, gtd, gsd = _dev(x, dt), _dev(g_t, dt), _dev(gstack, dt)
    bn = tuple(_dev(a, dt) for a in (q['beta'], q['gamma'], mean, inv_std))
    dbeta = torch.full((n,), SENTINEL, dtype=dt, device='cuda')
    dgamma = torch.full((n,), SENTINEL, dtype=dt, device='cuda')
    ops.bn_relu_bwd(xd, n, bn, gtd, gsd, dbeta, dgamma)
    torch.cuda.synchronize()
    # nothing but gstack[:, :n], dbeta, dgamma is written
    assert np.array_equal(xd.cpu().numpy(), x) and np.array_equal(gtd.cpu().numpy(), g_t)
    for got, want in zip(bn, (q['beta'], q['gamma'], mean, inv_std)):
        assert np.array_equal(got.cpu().numpy(), want)
    out = gsd.cpu().numpy()
    assert np.array_equal(out[:, n:], gstack[:, n:])
    return out[:, :n], dbeta.cpu().numpy(), dgamma.cpu().numpy()


def _bn_ref(x, mean, inv_std, q, g_t, gstack, n, npdt):
    c = lambda a: np.asarray(a).astype(npdt)
    g_x, dbeta, dgamma = R.bn_relu_bwd(c(x[:, :n]), dict(gamma=c(q['gamma']), beta=c(q['beta'])), c(mean), c(inv_std),
                                       c(g_t))
    return (c(gstack[:, :n]) + g_x).astype(npdt), dbeta.astype(npdt), dgamma.astype(npdt)


def _bn_magnitude(x, mean, inv_std, q, g_t, gstack, n):
    """The formula on absolute values (float64), with the gate as it is: what bounds any summation order."""
    x64, r = x[:, :n].astype(np.float64), inv_std[:n].astype(np.float64)[None, :, None, None]
    m = mean[:n].astype(np.float64)[None, :, None, None]
    gamma, beta = (q[k].astype(np.float64)[None, :, None, None] for k in ('gamma', 'beta'))
    N = x.shape[0] * x.shape[2] * x.shape[3]
    y = (x64 - m) * (gamma * r) + beta
    gy = np.where(y > 0, np.abs(g_t.astype(np.float64)), 0.0)
    xh = (np.abs(x64) + np.abs(m)) * r
    mb = gy.sum(axis=(0, 2, 3))
    mg = (gy * xh).sum(axis=(0, 2, 3))
    mx = np.abs(gstack[:, :n].astype(np.float64)) + np.abs(gamma) * r * (
        gy + mb[None, :, None, None] / N + xh * mg[None, :, None, None] / N)
    return mx, mb, mg


@pytest.mark.parametrize('H,W', [(1, 1), (2, 3), (7, 9), (37, 50)])
@pytest.mark.parametrize('prec', ['f32', 'f64'])
def test_bn_relu_bwd(built_lib, prec, H, W):
    """float32: the error against numpy float64 on the same operands is at most 4 x numpy float32's (DESIGN.md section
    12's rule), per output (gstack, dbeta, dgamma) as the maximum over the B x n cases of one plane size: the rule
    compares two maxima, and means something only where the reference's maximum is taken over enough entries to hold
    the half ulp that ANY float32 result carries -- at n = 1 dgamma is ONE number, numpy's may land anywhere inside
    that half ulp, and 4 x it then refuses a correctly rounded sum.  Every case's figures are printed.
    float64: per entry at most (N + 16) 2^-53 M, M the formula on absolute values.  The same bits twice; the sentinel
    channels of gstack, x, g_t and the BatchNorm vectors keep theirs."""
    from iterative_inference_segm_amd import _lib
    npdt = NP[prec]
    lib = _lib.load()
    names = ('gstack', 'dbeta', 'dgamma')
    worst = {w: [0.0, 0.0] for w in names}
    for B in (1, 3):
        for n in (1, 5, 16, 67):
            ops_ = _bn_operands(B, n, H, W, npdt, seed=1000 * B + 10 * n + H)
            if (H, W) == (37, 50):
                assert lib.iiseg_bn_relu_bwd_workspace_elems(n, H * W) >= 2 * 2 * n      # several partial sums
            else:
                assert lib.iiseg_bn_relu_bwd_workspace_elems(n, H * W) == 2 * n
            got = _bn_run(prec, *ops_, n)
            again = _bn_run(prec, *ops_, n)
            assert all(np.array_equal(a, b) for a, b in zip(got, again)), (B, n)
            ref = _bn_ref(*ops_, n, np.float64)
            if prec == 'f32':
                np32 = _bn_ref(*ops_, n, np.float32)
                assert all(a.dtype == np.float32 for a in np32)
                for g, r, n32, what in zip(got, ref, np32, names):
                    err, ref_err = np.abs(g - r).max(), np.abs(n32.astype(np.float64) - r).max()
                    print('bn_relu_bwd f32 B=%d n=%d %dx%d %s: max error %.3g, numpy float32 %.3g'
                          % (B, n, H, W, what, err, ref_err))
                    worst[what] = [max(worst[what][0], err), max(worst[what][1], ref_err)]
            else:
                N = B * H * W
                for g, r, m, what in zip(got, ref, _bn_magnitude(*ops_, n), names):
                    assert (np.abs(g - r) <= (N + 16) * 2.0 ** -53 * m).all(), (B, n, what)
    for what, (err, ref_err) in worst.items():
        assert err <= 4 * ref_err, (what, err, ref_err)


@pytest.mark.parametrize('prec', ['f32', 'f64'])
def test_bn_relu_bwd_edges(built_lib, prec):
    npdt = NP[prec]
    B, n, H, W = 3, 5, 7, 9
    # gamma = beta = 0: y = 0, nothing passes (relu'(0) = 0)
    ops_ = _bn_operands(B, n, H, W, npdt, seed=1, gamma=0.0, beta=0.0)
    gx, dbeta, dgamma = _bn_run(prec, *ops_, n)
    assert not dbeta.any() and not dgamma.any() and np.array_equal(gx, ops_[5][:, :n])
    # gamma = 0, beta > 0: y = beta > 0 everywhere, everything passes; g_x = 0
    ops_ = _bn_operands(B, n, H, W, npdt, seed=2, gamma=0.0, beta=0.25)
    gx, dbeta, dgamma = _bn_run(prec, *ops_, n)
    want = ops_[4].astype(np.float64).sum(axis=(0, 2, 3))
    tol = B * H * W * (2.0 ** -24 if prec == 'f32' else 2.0 ** -53) * np.abs(ops_[4]).astype(np.float64).sum(axis=(0, 2, 3))
    assert (np.abs(dbeta - want) <= tol).all() and np.array_equal(gx, ops_[5][:, :n])
    # B = 1 on 1 x 1: variance 0, inv_std = 100, xhat = 0
    x, mean, inv_std, q, g_t, gstack = _bn_operands(1, n, 1, 1, npdt, seed=3)
    assert np.allclose(inv_std[:n], 100.0)
    gx, dbeta, dgamma = _bn_run(prec, x, mean, inv_std, q, g_t, gstack, n)
    gy = np.where(q['beta'] > 0, g_t[0, :, 0, 0], 0)
    assert np.array_equal(dbeta, gy) and not dgamma.any()
    assert np.array_equal(gx, gstack[:, :n])                     # g_y - dbeta / 1 = 0


# ---- 2. maxpool2x2_bwd, exact on small integers ----
@pytest.mark.parametrize('prec', ['f32', 'f64'])
@pytest.mark.parametrize('H,W', [(2, 2), (5, 7), (6, 9), (13, 18)])
def test_maxpool2x2_bwd_is_exact_on_integers(built_lib, prec, H, W):
    from iterative_inference_segm_amd import ops
    dt = DT[prec]
    rng = np.random.default_rng(H * 100 + W)
    BC = (2, 3)
    pre = rng.integers(-3, 1, size=BC + (H, W)).astype(np.float64)          # ties everywhere, negative maxima
    pre[0, 0, :2, :2] = -2.0                                                 # a whole window tied, negative
    pre[1, 1, :2, :2] = 0.0                                                  # ... and tied at 0
    pooled = R.maxpool2(pre)
    assert (pooled < 0).any() and (pooled == 0).any()
    gpool = rng.integers(-4, 5, size=pooled.shape).astype(np.float64)
    gpool[0, 0, 0, 0], gpool[1, 1, 0, 0] = 3.0, -2.0
    h, w = H // 2, W // 2
    want = np.zeros_like(pre)
    want[:, :, :2 * h, :2 * w] = np.where(R._eqmask(pre, pooled), np.repeat(np.repeat(gpool, 2, 2), 2, 3), 0.0)
    pd, pld, gd = _dev(pre, dt), _dev(pooled, dt), _dev(gpool, dt)
    got = ops.maxpool2x2_bwd(gd, pd, pld).cpu().numpy()
    assert np.array_equal(got, want)
    assert (got[0, 0, :2, :2] == 3.0).all() and (got[1, 1, :2, :2] == -2.0).all()       # every tied position
    if H % 2:
        assert not got[:, :, -1].any()
    if W % 2:
        assert not got[:, :, :, -1].any()
    gated = ops.pool_relu_bwd(gd, pd, pld).cpu().numpy()                     # the gated entry keeps its behaviour
    assert not gated.any() and got.any()
    assert np.array_equal(pd.cpu().numpy(), pre) and np.array_equal(pld.cpu().numpy(), pooled)


# ---- 3. the module against the restatement ----
CASES = {'thin': R.THIN, 'wide': R.WIDE}
_CASES = {}


def _model_case(name):
    """(params, x, T, keeps, loss, grads, saved maps) of the float64 restatement: computed once, shared, not changed."""
    if name not in _CASES:
        cfg = CASES[name]
        params, x, T, keeps = R.make_case(cfg, seed=3)
        loss, grads, s = R.loss_and_param_grads(params, x, T, cfg, keeps)
        _CASES[name] = (params, x, T, keeps, loss, grads, s)
    return _CASES[name]


def _net(name, dt, params=None, **kw):
    from iterative_inference_segm_amd.densenet import FCDenseNet
    cfg = CASES[name]
    return FCDenseNet(_model_case(name)[0] if params is None else params, cfg['n_classes'], layer=[],
                      n_layers_per_block=cfg['nlpb'], n_pool=cfg['n_pool'], growth=cfg['growth'], dtype=dt, mma='f32',
                      trainable=True, **kw)


def _grads_as_ref(net, gv):
    out = []
    for li, L in enumerate(net.layers):
        q = dict(W=gv['conv%03d' % li][0], b=gv['conv%03d' % li][1])
        if L['kind'] in ('brc', 'td'):
            q['gamma'], q['beta'] = gv['bn%03d' % li]
        out.append({k: v.cpu().numpy().astype(np.float64) for k, v in q.items()})
    return out


def _gpu_backward(name, dt):
    from iterative_inference_segm_amd import ops
    params, x, T, keeps = _model_case(name)[:4]
    net = _net(name, dt)
    score = net.forward_train(_dev(x, dt), [_dev(k, dt) for k in keeps])
    res, g, _ = ops.ctx_loss(score, _dev(T, dt), ('crossentropy',), 1.0)
    gv = net.backward(g)
    torch.cuda.synchronize()
    return net, res, g, _grads_as_ref(net, gv)


def _ref_maps(saved, dtype):
    """FCDenseNet.saved_maps() as the dict tests/densenet_train_ref.backward reads."""
    conv = lambda v: v.cpu().numpy().astype(dtype) if torch.is_tensor(v) else v
    return {k: ([conv(a) for a in v] if isinstance(v, list) else conv(v)) for k, v in saved.items()}


def _rel_err(got, ref, cfg, mags):
    """max over the arrays of max|got - ref| / max|ref| -- for an array that is zero by construction
    (R.dead_arrays: its reference value is the rounding of a sum that cancels, 6e-18 on 'thin', and a quotient by
    it measures nothing) the denominator is the magnitude of that sum, max sum|g|."""
    worst = 0.0
    dead = R.dead_arrays(cfg)
    for li, (a, b) in enumerate(zip(got, ref)):
        assert sorted(a) == sorted(b), li
        for f in b:
            assert a[f].shape == b[f].shape, (li, f)
            den = np.abs(mags[li]).max() if (li, f) in dead else np.abs(b[f]).max()
            worst = max(worst, float(np.abs(np.asarray(a[f], np.float64) - b[f]).max() / den))
    return worst


F64_BOUND = 1e-13          # rounding only: DESIGN.md section 12's bound


@pytest.mark.parametrize('name', list(CASES))
def test_whole_backward_f64(built_lib, name):
    """Measured on an MI355X ('thin' / 'wide'): max relative error 4.8e-15 / 5.1e-15."""
    loss_ref, ref, s64 = _model_case(name)[4:7]
    net, res, _, got = _gpu_backward(name, torch.float64)
    saved = net.saved_maps()
    assert [tuple(a.shape) for a in saved['stacks']] == [a.shape for a in s64['stacks']]
    if name == 'wide':
        assert max(a.shape[1] for a in s64['stacks']) > 64 > CASES[name]['n_first']      # crosses the wgrad tile
    cfg = CASES[name]
    mags = {}
    R.backward(_model_case(name)[0], s64, R.loss_and_grad(s64['score'], _model_case(name)[2])[3], cfg, mags)
    dead = R.dead_arrays(cfg)
    assert len(dead) == cfg['n_pool'] - 1
    for li, q in enumerate(ref):
        for f, a in q.items():
            if (li, f) in dead:
                assert np.abs(a).max() <= 1e-13 * mags[li].max(), (li, f)                # zero but for rounding
            else:
                assert np.abs(a).max() > 1e-6 * max(np.abs(v).max() for v in q.values()), (li, f)   # alive
    err = _rel_err(got, ref, cfg, mags)
    print('FC-DenseNet backward f64 (%s): max relative error %.3g (loss %.12f / %.12f)'
          % (name, err, float(res[0]), loss_ref))
    assert abs(float(res[0]) - loss_ref) <= 1e-12 * abs(loss_ref)
    assert err <= F64_BOUND


@pytest.mark.parametrize('name', list(CASES))
def test_whole_backward_f32(built_lib, name):
    """Teacher-forced: the restatement ON the float32 forward's saved maps, statistics, masks and g_score (the same
    ReLU / pool decisions up to the rounding of y itself).  The bound is 4 x the error numpy float32 makes on the same
    maps against float64.  Free-running float32 against free-running float64: the number of differing decisions and
    every layer's cosine are reported; nothing beyond finiteness is asserted on them.
    Measured on an MI355X ('thin' / 'wide'): teacher-forced 8.8e-07 / 9.9e-07, numpy float32 1.35e-06 / 7.5e-07, 0 / 1
    differing decisions, every layer's cosine at least 0.999986."""
    cfg = CASES[name]
    params, x, T, keeps, _, free, s64 = _model_case(name)
    net, res, g, got = _gpu_backward(name, torch.float32)
    saved = net.saved_maps()
    g32 = g.cpu().numpy()
    mags = {}
    ref = R.backward(params, _ref_maps(saved, np.float64), g32.astype(np.float64), cfg, mags)
    p32 = [{k: (v.astype(np.float32) if k != 'kind' else v) for k, v in q.items()} for q in params]
    np32 = R.backward(p32, _ref_maps(saved, np.float32), g32, cfg)
    assert all(a.dtype == np.float32 for q in np32 for a in q.values())
    ref_err, err = _rel_err(np32, ref, cfg, mags), _rel_err(got, ref, cfg, mags)
    m64 = _ref_maps(saved, np.float64)
    gates = []
    for e in R.program(cfg)[0]:
        if e['kind'] in ('brc', 'td'):
            gates.append(R.bn_parts(m64['stacks'][e['sid']][:, :e['n']], params[e['li']], m64['mean'][e['sid']],
                                    m64['inv_std'][e['sid']])[1] > 0)
    gates += [R._eqmask(a, b) for a, b in zip(m64['td_pre'], m64['td_pooled'])]
    flips = sum(int((a != b).sum()) for a, b in zip(gates, R.decisions(s64)))
    cat = lambda q: np.concatenate([q[f].ravel() for f in R.FIELDS if f in q])
    cos = [float(cat(a) @ cat(b) / (np.linalg.norm(cat(a)) * np.linalg.norm(cat(b)))) for a, b in zip(got, free)]
    print('FC-DenseNet backward f32 (%s): teacher-forced max relative error %.3g, numpy float32 %.3g; free-running: '
          '%d differing decisions, gradient cosine per layer %s'
          % (name, err, ref_err, flips, ' '.join('%.6f' % c for c in cos)))
    assert err <= 4 * ref_err
    assert all(np.isfinite(a).all() for q in got for a in q.values()) and np.isfinite(cos).all()


def _trainer(name, dt, **kw):
    from iterative_inference_segm_amd.train import DenseNetTrainer
    C_ = CASES[name]['n_classes']
    return DenseNetTrainer(_net(name, dt), C_, [C_], **kw)


# ---- 4. five float64 RMSprop steps ----
def test_first_five_steps_match_the_restatement_f64(built_lib):
    """RMSprop, weight_decay 1e-4, fixed dropout masks; bound: a relative 1e-9 (the bound of the FCN-8 test).  Measured
    on an MI355X: the losses agree to every one of twelve printed digits."""
    cfg = R.THIN
    params, x, T, keeps = _model_case('thin')[:4]
    dt = torch.float64
    wd, lr = 1e-4, 1e-3
    tr = _trainer('thin', dt, learning_rate=lr, weight_decay=wd)
    xd, Td, kd = _dev(x, dt), _dev(T, dt), [_dev(k, dt) for k in keeps]
    flat = R.flatten(params)
    assert np.array_equal(tr.net.flat.cpu().numpy(), flat)                   # the flat buffer's order
    acc = np.zeros_like(flat)
    worst = 0.0
    for step in range(5):
        loss = float(tr.train_step(xd, Td, kd))
        loss_ref, grads, _ = R.loss_and_param_grads(R.unflatten(flat, params), x, T, cfg, keeps, wd)
        flat, acc = R.rmsprop_step(flat, R.flatten(grads), acc, lr)
        worst = max(worst, abs(loss - loss_ref) / abs(loss_ref))
        print('step %d: loss %.12f restatement %.12f' % (step, loss, loss_ref))
        assert abs(loss - loss_ref) <= 1e-9 * abs(loss_ref)
    print('FC-DenseNet five float64 steps: worst relative loss difference %.3g' % worst)


# ---- 5. determinism, refresh, checkpoints ----
def test_train_step_is_deterministic_and_every_path_sees_the_new_weights(built_lib, tmp_path):
    from iterative_inference_segm_amd.densenet import FCDenseNet, build_fcdensenet, layer_plan, load_params, save_checkpoint
    cfg = R.THIN
    params, x, T, keeps = _model_case('thin')[:4]
    dt = torch.float32
    xd, Td, kd = _dev(x, dt), _dev(T, dt), [_dev(k, dt) for k in keeps]
    flats = []
    for _ in range(2):
        tr = _trainer('thin', dt, learning_rate=1e-2, weight_decay=1e-4, seed=3)
        before = tr.net.forward(xd)[-1].clone()                              # packed weights exist BEFORE the steps
        tr.train_step(xd, Td, kd)
        tr.train_step(xd, Td)                                                # masks from the seeded generator
        torch.cuda.synchronize()
        flats.append(tr.net.flat.clone())
    assert torch.equal(flats[0], flats[1])                                   # two identical runs: identical bits
    assert not torch.equal(flats[0], _dev(R.flatten(params), dt))
    assert bool(torch.isfinite(flats[0]).all())
    after = tr.net.forward(xd)[-1].clone()
    assert not torch.equal(after, before)
    path = str(tmp_path / 'FC-DenseNet103_weights.npz')
    save_checkpoint(path, tr.net, cfg['n_first'])
    loaded = build_fcdensenet(layer=[], n_classes=cfg['n_classes'], weight_path=path, dtype=dt)
    assert (loaded.nlpb, loaded.n_pool, loaded.growth) == (cfg['nlpb'], cfg['n_pool'], cfg['growth'])
    for e in loaded.layers:
        e['conv'].wino = e['conv'].wino_f64 = False                          # the direct kernels only
    assert torch.equal(loaded(xd)[-1], after)
    plan = layer_plan(cfg['nlpb'], cfg['n_pool'], cfg['growth'], cfg['n_first'], 3, cfg['n_classes'])
    again = _net('thin', dt, params=load_params(path, plan))
    assert torch.equal(again.flat, tr.net.flat)
    assert torch.equal(again.forward_train(xd, deterministic=True), tr.net.forward_train(xd, deterministic=True))
    # the running averages the checkpoint carries: two updates from (0, 1), alpha 0.1
    with np.load(path) as f:
        run_mean, run_inv = f['arr_4'], f['arr_5']                           # of the first 'brc' layer (W, b | beta, gamma)
    assert run_mean.shape == (cfg['n_first'],) and np.abs(run_mean).max() > 0 and (run_inv != 1).all()
    # the non-trainable module: the same bits with and without the new keyword
    kw = dict(layer=['pool1'], n_layers_per_block=cfg['nlpb'], n_pool=cfg['n_pool'], growth=cfg['growth'], dtype=dt)
    a = FCDenseNet(params, cfg['n_classes'], **kw)(xd)
    b = FCDenseNet(params, cfg['n_classes'], trainable=False, **kw)(xd)
    assert len(a) == len(b) == 2 and all(torch.equal(u, v) for u, v in zip(a, b))


# ---- 6. the loss goes down ----
def test_loss_goes_down_over_40_steps_f32(built_lib):
    x, T = _model_case('thin')[1:3]
    dt = torch.float32
    tr = _trainer('thin', dt, learning_rate=1e-3, seed=2)
    xd, Td = _dev(x, dt), _dev(T, dt)
    losses = [tr.train_step(xd, Td) for _ in range(40)]
    losses = [float(v) for v in torch.stack(losses).cpu()]
    print('FC-DenseNet loss, steps 0-9: %.5f, steps 30-39: %.5f' % (np.mean(losses[:10]), np.mean(losses[-10:])))
    assert np.all(np.isfinite(losses))
    assert np.mean(losses[-10:]) < np.mean(losses[:10])


# ---- 7. the driver end to end, and train_dae.py from its checkpoint ----
def test_driver_end_to_end(built_lib, tmp_path):
    from iterative_inference_segm_amd.densenet import build_fcdensenet
    save, weights = str(tmp_path / 'save'), str(tmp_path / 'weights')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_fcdensenet.py'), '--synthetic', '--num_epochs', '2',
                        '--n_images', '2', '--image_size', '16', '16', '--batch_size', '[2, 2, 2]', '--savepath', save,
                        '--layers_per_block', '[2, 3, 2, 3, 2]', '--growth', '4', '--n_first', '8',
                        '--max_batches', '1'], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    folder = os.path.join(save, 'camvid', 'fc_densenet')
    files = os.listdir(folder)
    assert 'FC-DenseNet103_weights_best.npz' in files and 'output.log' in files and 'config.txt' in files
    assert any(f.startswith('errors_') for f in files)
    assert len(open(os.path.join(folder, 'output.log')).read().splitlines()) == 2
    os.makedirs(os.path.join(weights, 'camvid'))
    path = os.path.join(weights, 'camvid', 'FC-DenseNet103_weights.npz')
    shutil.copy(os.path.join(folder, 'FC-DenseNet103_weights_best.npz'), path)
    net = build_fcdensenet(layer=[], n_classes=11, weight_path=path)
    x = _dev(np.random.default_rng(1).random((2, 3, 16, 16)), torch.float32)
    probs = net(x)[-1]
    assert tuple(probs.shape) == (2, 11, 16, 16) and bool(torch.isfinite(probs).all())
    # train_dae.py starts from it (16 x 16 maps: DenseNet103's five pools would have nothing left to pool)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_dae.py'), '--synthetic', '--num_epochs', '1',
                        '--n_images', '4', '--image_size', '16', '16', '--savepath', str(tmp_path / 'dae'),
                        '--loadpath', str(tmp_path / 'dae_load'), '--weights_path', weights,
                        '-segmentation_net', 'densenet'], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    exp, = os.listdir(os.path.join(str(tmp_path / 'dae'), 'camvid'))
    assert exp.startswith('flip_final_densenet_contextmod')
    line, = open(os.path.join(str(tmp_path / 'dae'), 'camvid', exp, 'output.log')).read().splitlines()
    assert line.startswith('EPOCH 0:')
