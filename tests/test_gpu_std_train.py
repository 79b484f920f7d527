"""GPU: training the standard DAE -- the zero-padded 3x3 weight gradient (csrc/conv_wgrad.hip: float32 on the
matrix pipe, float64 on the vector ALU) and the grid form of the optimizer step (csrc/ctx_train.hip), bit for bit
on data where every sum is exact; StandardDAE.forward_train / backward / refresh, the trainer and train_dae.py
against the float64 restatement (tests/std_train_ref.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import std_train_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {'f32': torch.float32, 'f64': torch.float64}


def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda().contiguous()


# ---- 1. weight gradient, exact on small-integer data ----
def _wgrad_ref(x, gz, pad):
    """int64: dW[co, ci, ky, kx] = sum gz[b, co, y, x] xpad[b, ci, y + ky, x + kx], db[co] = sum gz."""
    B, Cin, H, W = x.shape
    OH, OW = gz.shape[2:]
    xp = np.zeros((B, Cin, H + 2 * pad, W + 2 * pad), dtype=np.int64)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    dW = np.zeros((gz.shape[1], Cin, 3, 3), dtype=np.int64)
    for ky in range(3):
        for kx in range(3):
            dW[:, :, ky, kx] = np.tensordot(gz, xp[:, :, ky:ky + OH, kx:kx + OW], axes=([0, 2, 3], [0, 2, 3]))
    return dW, gz.sum(axis=(0, 2, 3))


CHANNELS = [(11, 64), (24, 16), (64, 130), (130, 33)]            # none a multiple of the 64 / 32 channel blocks
# (H, W of the input, pad): pad 1 on the three maps (37 x 150 needs several pixel slabs); pad 5 on an input smaller
# than the padding (every output pixel's patch is mostly padding, some lie wholly inside it) and on 14 x 13
GEOMETRY = [(7, 7, 1), (14, 13, 1), (37, 150, 1), (3, 4, 5), (14, 13, 5)]
_REF = {}


def _case(Cin, Cout, B, H, W, pad):
    key = (Cin, Cout, B, H, W, pad)
    if key not in _REF:
        rng = np.random.default_rng(Cin * 1000 + Cout + 7 * B + H + 3 * pad)
        x = rng.integers(-2, 3, size=(B, Cin, H, W))
        gz = rng.integers(-2, 3, size=(B, Cout, H + 2 * pad - 2, W + 2 * pad - 2))
        gz[rng.integers(0, 2, size=gz.shape) == 0] = 0           # as behind a ReLU mask
        dW, db = _wgrad_ref(x, gz, pad)
        assert np.abs(dW).max() < 2 ** 24 and np.abs(db).max() < 2 ** 24 and np.abs(dW).max() > 0
        _REF[key] = (x, gz, dW, db)
    return _REF[key]


@pytest.mark.parametrize('prec', ['f32', 'f64'])
@pytest.mark.parametrize('H,W,pad', GEOMETRY)
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('Cin,Cout', CHANNELS)
def test_conv_weight_gradient_is_exact_on_integers(built_lib, prec, Cin, Cout, B, H, W, pad):
    from iterative_inference_segm_amd import _lib, ops
    dt = DT[prec]
    x, gz, dW_ref, db_ref = _case(Cin, Cout, B, H, W, pad)
    xd, gzd = _dev(x, dt), _dev(gz, dt)
    d = ops.conv_wgrad_desc(x.shape, Cout, pad)
    nslab = _lib.load().iiseg_conv_wgrad_slabs(C.byref(d), 4 if prec == 'f32' else 8)
    if (H, W) == (37, 150):
        assert nslab >= 2                                        # slabs + the finalize launch
    if (H, W) == (7, 7) and B == 1:
        assert nslab == 1                                        # straight into dW
    # the layer's own array, W[out, in, 3, 3]
    dW = torch.full(dW_ref.shape, 7.0, dtype=dt, device='cuda')
    db = torch.full((Cout,), 7.0, dtype=dt, device='cuda')
    ops.conv_wgrad(xd, gzd, dW, db, pad=pad)
    # the middle of a larger parameter, in both layouts: the other input channels keep the sentinel; no db
    lo, hi = 3, 5
    big = torch.full((Cout, lo + Cin + hi, 3, 3), -9.0, dtype=dt, device='cuda')
    ops.conv_wgrad(xd, gzd, big, None, pad=pad, ci0=lo)
    bigT = torch.full((lo + Cin + hi, Cout, 3, 3), -9.0, dtype=dt, device='cuda')
    ops.conv_wgrad(xd, gzd, bigT, None, pad=pad, ci0=lo, layout='iohw')
    torch.cuda.synchronize()
    assert np.array_equal(dW.cpu().numpy(), dW_ref.astype(np.float64))
    assert np.array_equal(db.cpu().numpy(), db_ref.astype(np.float64))
    want = np.full(tuple(big.shape), -9.0)
    want[:, lo:lo + Cin] = dW_ref
    assert np.array_equal(big.cpu().numpy(), want)
    assert np.array_equal(bigT.cpu().numpy(), want.transpose(1, 0, 2, 3))


@pytest.mark.parametrize('prec', ['f32', 'f64'])
def test_conv_weight_gradient_gives_the_same_bits_twice(built_lib, prec):
    """No atomics, fixed slab order: real-valued data, several slabs, two runs."""
    from iterative_inference_segm_amd import ops
    dt = DT[prec]
    rng = np.random.default_rng(5)
    x = _dev(rng.standard_normal((3, 24, 37, 150)), dt)
    gz = _dev(rng.standard_normal((3, 16, 37, 150)), dt)
    runs = []
    for _ in range(2):
        dW = torch.zeros((16, 24, 3, 3), dtype=dt, device='cuda')
        db = torch.zeros(16, dtype=dt, device='cuda')
        ops.conv_wgrad(x, gz, dW, db, pad=1)
        runs.append((dW.cpu().numpy(), db.cpu().numpy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    # and it is the gradient: against float64 numpy, at the precision of the format over 16650 pixels
    xp = np.pad(x.double().cpu().numpy(), ((0, 0), (0, 0), (1, 1), (1, 1)))
    g = gz.double().cpu().numpy()
    ref = np.stack([np.stack([np.tensordot(g, xp[:, :, ky:ky + 37, kx:kx + 150], axes=([0, 2, 3], [0, 2, 3]))
                              for kx in range(3)], axis=-1) for ky in range(3)], axis=-2)
    # |error| <= n u sum|a b| for ANY summation order of n = 16650 fused multiply-adds, sum|a b| taken from the
    # data per entry (about 0.64 n, so the bound is near 0.66 in float32 on sums of magnitude about 130)
    u = 2.0 ** -24 if prec == 'f32' else 2.0 ** -53
    n = 3 * 37 * 150
    mag = np.stack([np.stack([np.tensordot(np.abs(g), np.abs(xp[:, :, ky:ky + 37, kx:kx + 150]),
                                           axes=([0, 2, 3], [0, 2, 3]))
                              for kx in range(3)], axis=-1) for ky in range(3)], axis=-2)
    assert (np.abs(runs[0][0] - ref) <= (n + 1) * u * mag).all()
    assert (np.abs(runs[0][1] - g.sum(axis=(0, 2, 3))) <= (n + 1) * u * np.abs(g).sum(axis=(0, 2, 3))).all()


# ---- 3. the grid form of the optimizer step equals the one-workgroup form, bit for bit ----
@pytest.mark.parametrize('prec', ['f32', 'f64'])
@pytest.mark.parametrize('kind', ['rmsprop', 'adam'])
def test_grid_optimizer_step_equals_the_single_workgroup_step(built_lib, prec, kind):
    from iterative_inference_segm_amd import ops
    dt = DT[prec]
    n = 1000003                                                  # more than one workgroup's stride, a multiple of nothing
    rng = np.random.default_rng(11)
    p0 = rng.standard_normal(n)

    def state():
        return dict(p=_dev(p0, dt), s1=torch.zeros(n, dtype=dt, device='cuda'),
                    s2=torch.zeros(n, dtype=dt, device='cuda') if kind == 'adam' else None,
                    st=torch.tensor([0.0, 1.0, 1.0], dtype=dt, device='cuda') if kind == 'adam' else None,
                    lr=torch.tensor([1e-3], dtype=dt, device='cuda'))
    one, grid = state(), state()
    for step in range(3):
        g = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 1, size=n)
        g[rng.integers(0, n, size=50)] = 0
        gd = _dev(g, dt)
        ops.opt_step(kind, one['p'], gd, one['s1'], one['s2'], one['lr'], one['st'])
        ops.opt_step(kind, grid['p'], gd, grid['s1'], grid['s2'], grid['lr'], grid['st'], grid=True)
        for k in ('p', 's1', 's2', 'st'):
            if one[k] is not None:
                assert torch.equal(one[k], grid[k]), (step, k)
        assert not torch.equal(grid['p'], _dev(p0, dt))
        for s in (one, grid):
            s['lr'].mul_(0.5)                                    # annealed on the device between steps
    if kind == 'adam':
        assert grid['st'][0].item() == 3.0


# ---- 2. the whole backward on the two models ----
MODELS = {'small': R.SMALL, 'second': R.SECOND}
_CASES = {}


def _model_case(which):
    """(params, [h], y, T, float64 loss, float64 gradients, float64 net): computed once, shared, never changed."""
    if which not in _CASES:
        params, hs, y, T = R.make_case(MODELS[which])
        loss, grads, net = R.loss_and_param_grads(params, hs, y, T, MODELS[which][3])
        _CASES[which] = (params, hs, y, T, loss, grads, net)
    return _CASES[which]


def _std_dae(which, params, dt):
    from iterative_inference_segm_amd.dae import StandardDAE
    return StandardDAE(params, MODELS[which][0], device='cuda', dtype=dt, mma='f32', trainable=True,
                       **MODELS[which][3])


def _gpu_backward(which, dt):
    from iterative_inference_segm_amd import ops
    params, hs, y, T = _model_case(which)[:4]
    dae = _std_dae(which, params, dt)
    score = dae.forward_train([_dev(h, dt) for h in hs], _dev(y, dt))
    res, g, _ = ops.ctx_loss(score, _dev(T, dt), ('crossentropy',), 1.0)
    grads = dae.backward(g)
    torch.cuda.synchronize()
    return dae, res, g, {n: (a.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64))
                         for n, (a, b) in grads.items()}


def _rel_err(got, ref):
    """max over the arrays of max|got - ref| / max|ref|"""
    worst = 0.0
    for n in ref:
        for a, b in zip(got[n], ref[n]):
            assert a.shape == b.shape, n
            worst = max(worst, float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max()))
    return worst


# rounding only: the bound DESIGN.md section 9 uses for the same statement about the context module
F64_BOUND = 1e-13


@pytest.mark.parametrize('which', ['small', 'second'])
def test_whole_backward_f64(built_lib, which):
    loss_ref, ref = _model_case(which)[4:6]
    _, res, _, got = _gpu_backward(which, torch.float64)
    err = _rel_err(got, ref)
    print('standard DAE backward f64 (%s): max relative error %.3g (loss %.12f / %.12f)'
          % (which, err, float(res[0]), loss_ref))
    assert abs(float(res[0]) - loss_ref) <= 1e-12 * abs(loss_ref)
    assert err <= F64_BOUND


@pytest.mark.parametrize('which', ['small', 'second'])
def test_whole_backward_f32(built_lib, which):
    """Teacher-forced: the restatement ON the float32 forward's saved maps and its g_score (the same ReLU / pool
    decisions, rounding only).  The bound is 4 x the error numpy float32 makes on the same maps against float64
    (the margin: another, but fixed, summation order over up to 1e5 pixels).  Free-running float32 against
    free-running float64: cosine per layer >= 0.999.
    Measured on an MI355X (small / second model): teacher-forced 1.89e-07 / 2.11e-07, numpy float32 1.14e-07 /
    1.95e-07, no differing decision, cosine 1.000000 on every layer (DESIGN.md section 12 holds the same figures)."""
    cfg = MODELS[which][3]
    params, hs, y, T, _, free, net64 = _model_case(which)
    dae, res, g, got = _gpu_backward(which, torch.float32)
    saved32 = {k: v.cpu().numpy() for k, v in dae.saved_maps().items()}
    g32 = g.cpu().numpy()
    to = lambda d, t: {k: v.astype(t) for k, v in d.items()}
    ref = R.backward(params, hs, to(saved32, np.float64), g32.astype(np.float64), cfg)
    p32 = {k: tuple(a.astype(np.float32) for a in v) for k, v in params.items()}
    np32 = R.backward(p32, [h.astype(np.float32) for h in hs], saved32, g32, cfg)
    assert all(a.dtype == np.float32 for v in np32.values() for a in v)
    ref_err, err = _rel_err(np32, ref), _rel_err(got, ref)
    total = len(R.order_of(cfg)) // 2
    flips = sum(int((a != b).sum()) for a, b in zip(R.decisions(to(saved32, np.float64), total),
                                                    R.decisions(net64, total)))
    cos = {n: float(np.concatenate([a.ravel() for a in got[n]]) @ np.concatenate([a.ravel() for a in free[n]]) /
                    (np.linalg.norm(np.concatenate([a.ravel() for a in got[n]])) *
                     np.linalg.norm(np.concatenate([a.ravel() for a in free[n]])))) for n in free}
    print('standard DAE backward f32 (%s): teacher-forced max relative error %.3g, numpy float32 %.3g; '
          'free-running: %d differing decisions, gradient cosine per layer %s'
          % (which, err, ref_err, flips, {n: '%.6f' % c for n, c in cos.items()}))
    assert err <= 4 * ref_err
    assert min(cos.values()) >= 0.999


# the bounds of tests/test_gpu_e2e.py::test_true_gradient_mode, x (1 + max|g|)
@pytest.mark.parametrize('prec,tol', [('f64', 1e-10), ('f32', 2e-4)])
def test_backward_and_backward_y_are_one_walk_that_keeps_no_state(built_lib, prec, tol):
    """On a trainable DAE (gradient layers off the Winograd form; the small model: pad 3, so the first layer's data
    gradient is the crop at offset 2): backward, backward_y, backward again leave the same gradient buffer, and
    backward_y is dE/dy of E = sum (r - y)^2 through the DAE (oracle/dae_grad.py)."""
    from oracle import dae_grad as G
    from iterative_inference_segm_amd import ops
    dt = DT[prec]
    params, hs, y = _model_case('small')[:3]
    dae = _std_dae('small', params, dt)
    yd = _dev(y, dt)
    score = dae.forward_train([_dev(h, dt) for h in hs], yd)
    g = ops.sqerr_softmax_bwd(score, yd, off=(0, 0))
    dae.backward(g)
    first = dae.gflat.clone()
    g_thr = dae.backward_y(g, yd.shape)
    dae.backward(g)
    assert torch.equal(dae.gflat, first) and bool(first.any())
    r = ops.crop_softmax(score, y.shape[2], y.shape[3], off=(0, 0))
    torch.cuda.synchronize()
    got = g_thr.cpu().numpy().astype(np.float64) - 2.0 * (r.cpu().numpy().astype(np.float64) - y)
    g_ref, r_ref = G.dae_sqerr_grad(params, hs, y, **MODELS['small'][3])
    err, scale = np.abs(got - g_ref).max(), 1 + np.abs(g_ref).max()
    print('trainable standard DAE backward_y %s: max|g - ref| = %.3g (bound %.3g)' % (prec, err, tol * scale))
    assert tuple(g_thr.shape) == y.shape and np.abs(g_ref).max() > 0
    assert err <= tol * scale


# ---- 4. training end to end (the second model) ----
def _trainer(dt, noise=0.1, seed=1, **kw):
    from iterative_inference_segm_amd.train import DAETrainer
    params = _model_case('second')[0]
    return DAETrainer(None, _std_dae('second', params, dt), 11, [11], noise=noise, seed=seed, **kw)


def test_first_five_steps_match_the_restatement_f64(built_lib):
    cfg = R.SECOND[3]
    params, hs, y, T = _model_case('second')[:4]
    dt = torch.float64
    tr = _trainer(dt, learning_rate=1e-4)
    hd, yd, Td = [_dev(h, dt) for h in hs], _dev(y, dt), _dev(T, dt)
    gen = torch.Generator(device='cuda')
    gen.manual_seed(5)
    order = R.order_of(cfg)
    flat = R.flatten(params, order)
    a = np.zeros_like(flat)
    for step in range(5):
        eps = torch.randn(yd.shape, generator=gen, device='cuda', dtype=dt)           # the same noise to both
        loss = float(tr.train_step(hd, yd, Td, eps=eps))
        yn = y + 0.1 * eps.cpu().numpy()
        loss_ref, grads, _ = R.loss_and_param_grads(R.unflatten(flat, params, order), hs, yn, T, cfg)
        flat, a = R.rmsprop_step(flat, R.flatten(grads, order), a, 1e-4)
        print('step %d: loss %.12f restatement %.12f' % (step, loss, loss_ref))
        assert abs(loss - loss_ref) <= 1e-12 * abs(loss_ref)


def test_train_step_is_deterministic_and_every_path_sees_the_new_weights(built_lib, tmp_path):
    from iterative_inference_segm_amd.dae import param_order
    from iterative_inference_segm_amd.weights import load_param_list, save_param_list
    cfg = R.SECOND[3]
    params, hs, y, T = _model_case('second')[:4]
    dt = torch.float32
    hd, yd, Td = [_dev(h, dt) for h in hs], _dev(y, dt), _dev(T, dt)
    flats = []
    for _ in range(2):
        tr = _trainer(dt, seed=3, learning_rate=1e-2)
        before = tr.dae.scores(hd, yd).clone()       # packed weights exist BEFORE the step, and are stale after it
        tr.train_step(hd, yd, Td)
        torch.cuda.synchronize()
        flats.append(tr.dae.flat.clone())
    assert torch.equal(flats[0], flats[1])
    assert not torch.equal(flats[0], _dev(R.flatten(params, R.order_of(cfg)), dt))
    order = param_order(cfg['concat_h'], 1, cfg['additional_pool'])
    assert order == R.order_of(cfg)
    path = str(tmp_path / 'dae_model_best.npz')
    save_param_list(path, tr.dae.state_arrays(), order)
    fresh = _std_dae('second', load_param_list(path, order), dt)
    assert torch.equal(fresh.flat, tr.dae.flat)
    eager = tr.dae.scores(hd, yd).clone()
    assert not torch.equal(eager, before)
    assert torch.equal(eager, tr.dae.scores(hd, yd, session=tr.dae.new_session(hd, yd)))
    assert torch.equal(eager, fresh.scores(hd, yd))
    # the data-gradient layers too: a second step on both gives the same bits
    fresh_tr = _trainer(dt, seed=3, learning_rate=1e-2)
    fresh_tr.dae.flat.copy_(tr.dae.flat)
    fresh_tr.dae.refresh()
    for t in (tr, fresh_tr):
        t.s1.zero_()
        t.train_step(hd, yd, Td, eps=torch.zeros_like(yd))
    assert torch.equal(tr.dae.flat, fresh_tr.dae.flat)


def test_loss_goes_down_over_40_steps_f32(built_lib):
    hs, T = _model_case('second')[1], _model_case('second')[3]
    dt = torch.float32
    tr = _trainer(dt, seed=2, learning_rate=1e-4)
    hd, Td = [_dev(h, dt) for h in hs], _dev(T, dt)
    yd = Td[:, :11].contiguous()                                 # from_gt
    losses = [tr.train_step(hd, yd, Td) for _ in range(40)]
    losses = [float(v) for v in torch.stack(losses).cpu()]
    print('standard DAE loss, steps 0-9: %.5f, steps 30-39: %.5f' % (np.mean(losses[:10]), np.mean(losses[-10:])))
    assert np.all(np.isfinite(losses))
    assert np.mean(losses[-10:]) < np.mean(losses[:10])


# ---- 5. the driver end to end ----
def test_driver_end_to_end(built_lib, tmp_path):
    import json
    from iterative_inference_segm_amd.dae import buildDAE
    from iterative_inference_segm_amd.helpers import build_experiment_name
    save, load, out = str(tmp_path / 'save'), str(tmp_path / 'load'), str(tmp_path / 'out')
    dd = {'kind': 'standard', 'dropout': 0, 'skip': True, 'unpool_type': 'trackind', 'noise': 0.1,
          'concat_h': ['pool2'], 'from_gt': True, 'n_filters': 8, 'conv_before_pool': 1, 'additional_pool': 2,
          'temperature': 1.0, 'path_weights': '', 'layer': 'probs_dimshuffle', 'exp_name': 't_', 'bn': 0}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_dae.py'), '--synthetic', '--num_epochs', '1',
                        '--n_images', '4', '--image_size', '40', '36', '--savepath', save, '--loadpath', load,
                        '-segmentation_net', 'fcn8', '-train_dict', '{"batch_size": [2, 2, 2]}',
                        '-dae_dict', json.dumps(dd)], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    exp, = os.listdir(os.path.join(save, 'camvid'))
    # the folder iterative_inference.py reads for the same dictionaries
    assert exp == build_experiment_name('fcn8', data_aug=True, ae_h=False, training_loss=['crossentropy'],
                                        learning_rate=0.0001, lr_anneal=0.99, weight_decay=0.0001,
                                        optimizer='rmsprop', **dd)
    folder = os.path.join(load, 'camvid', exp)
    assert os.path.exists(os.path.join(folder, 'dae_model_best.npz'))
    dae = buildDAE(n_classes=11, concat_h=dd['concat_h'], n_filters=8, additional_pool=2, skip=True,
                   unpool_type='trackind', path_weights=folder, model_name='dae_model_best.npz', load_weights=True)
    assert dae.enc['conv3_1'].Cin == 16 + 128                    # h: pool2 of the FCN-8
    assert bool(torch.isfinite(dae.enc['conv1_1'].W).all())
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'iterative_inference.py'), '--synthetic', '--n_images', '2',
                        '--image_size', '40', '36', '--batch_size', '2', '--num_iter', '2', '-segmentation_net',
                        'fcn8', '--savepath', out, '--loadpath', load, '-dae_dict', json.dumps(dd)],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
