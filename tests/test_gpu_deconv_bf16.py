"""GPU: deconv='bf16'  -- the gradients of the K = 3, stride-2 transposed convolution on the
16-bit matrix pipe (csrc/deconv_grad_bf16.hip; ops.deconv_wgrad / ops.deconv_dgrad with mma='bf16') and the switch
through FCDenseNet, the trainer and train_fcdensenet.py.  The kernels: exact on data bf16 holds exactly, over every
descriptor feature, with nothing written outside their outputs; on real data within the any-order fp32 accumulation
bound of the float64 sum over operands rounded on the CPU with .to(torch.bfloat16) (tests/deconv_bf16_ref.py), ties
and direction included, db from the unrounded g, the same bits twice.  The module: nothing but the TransitionUp
gradients (and what is walked after them) changes between the modes.

Measured on an MI355X (for the record; the assertions are the derived bounds): see DESIGN.md section 23."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import deconv_bf16_ref as D
import densenet_train_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = torch.float32
U = 2.0 ** -24
GUARD, SENTINEL = 64, -77.0


def _dev(a, dt=F32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda().contiguous()


def _carve(shape):
    """(buffer, view): a tensor of `shape` in the middle of a larger buffer filled with the sentinel."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=F32, device='cuda')
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_intact(buf):
    b = buf.cpu().numpy()
    return bool((b[:GUARD] == SENTINEL).all() and (b[-GUARD:] == SENTINEL).all())


def _run(x, g, W, window, want_db=True):
    """(dW, db, gx, gx through the C entry into a carved buffer) as float64 numpy, guards checked."""
    from iterative_inference_segm_amd import _lib, ops
    xd, gd, Wd = (_dev(v) for v in (x, g, W))
    (bW, dW), (bb, db) = _carve(W.shape), _carve((W.shape[1],))
    ops.deconv_wgrad(xd, gd, dW, db if want_db else None, 2, window=window, mma='bf16')
    gx = ops.deconv_dgrad(gd, Wd, 2, x.shape[2:], window=window, mma='bf16')
    bx, gx2 = _carve(x.shape)
    d = ops.deconv_desc(x.shape, W.shape[1], 3, 2, window)
    st = _lib.load().iiseg_deconv_dgrad_bf16(ops._stream(), C.byref(d), ops._ptr(gd), ops._ptr(Wd), None, ops._ptr(gx2))
    assert st == 0
    torch.cuda.synchronize()
    assert _guards_intact(bW) and _guards_intact(bb) and _guards_intact(bx)
    if not want_db:
        assert bool((bb == SENTINEL).all())                      # nothing written for it
    assert tuple(gx.shape) == x.shape and gx.dtype == F32
    assert torch.equal(gx, gx2)
    return dW.cpu().double().numpy(), db.cpu().double().numpy(), gx.cpu().double().numpy()


# ---- 1. exact on small integers ----
GEOMETRY = [(1, 1), (2, 3), (7, 7), (6, 9), (13, 18), (37, 50)]
CHANNELS = [(1, 1), (4, 4), (8, 12), (12, 8), (16, 16), (33, 20), (80, 80)]
DEEP = [(240, 240), (70, 130)]                                   # several channel blocks / k-tiles: the small maps only
INT_CASES = [(ci, co, h, w) for ci, co in CHANNELS for h, w in GEOMETRY] + \
            [(ci, co, h, w) for ci, co in DEEP for h, w in ((7, 7), (6, 9))]


def _windows(H, W):
    """full; DenseNet's; one more row; odd offsets (where non-empty); (3, 2, ., .) cut to fit on two geometries."""
    wins = [None, (0, 0, 2 * H, 2 * W), (0, 0, 2 * H + 1, 2 * W)]
    if 2 * H - 1 > 0 and 2 * W - 1 > 0:
        wins.append((1, 1, 2 * H - 1, 2 * W - 1))
    if (H, W) in ((7, 7), (13, 18)):
        wins.append((3, 2, min(9, 2 * H + 1 - 3), min(20, 2 * W + 1 - 2)))
    return wins


def _int_case(Cin, Cout, B, H, W, window, k):
    rng = np.random.default_rng(Cin * 1000 + Cout + 7 * B + 31 * H + W + 977 * k)
    win = D.full_window(H, W) if window is None else window
    x = rng.integers(-2, 3, size=(B, Cin, H, W)).astype(np.float32)
    Wt = rng.integers(-2, 3, size=(Cin, Cout, 3, 3)).astype(np.float32)
    g = rng.integers(-2, 3, size=(B, Cout, win[2], win[3])).astype(np.float32)
    g[rng.integers(0, 2, size=g.shape) == 0] = 0                 # as behind a dropout mask
    ref = D.grads(x, g, Wt, window)
    assert all(r.dtype == np.float64 and np.abs(r).max(initial=0) < 2 ** 24 for r in ref)
    return x, g, Wt, ref


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('Cin,Cout,H,W', INT_CASES)
def test_gradients_are_exact_on_integers_and_write_nothing_else(built_lib, Cin, Cout, B, H, W):
    from iterative_inference_segm_amd import _lib, ops
    for k, window in enumerate(_windows(H, W)):
        x, g, Wt, (dW_ref, gx_ref, db_ref) = _int_case(Cin, Cout, B, H, W, window, k)
        nslab = _lib.load().iiseg_deconv_wgrad_bf16_slabs(C.byref(ops.deconv_desc(x.shape, Cout, 3, 2, window)))
        if (H, W) == (37, 50) and B == 3:
            assert nslab >= 2                                    # slabs + the finalize launch
        if (H, W) == (1, 1):
            assert nslab == 1                                    # straight into dW and db
        dW, db, gx = _run(x, g, Wt, window, want_db=(k % 2 == 0))
        assert np.array_equal(dW, dW_ref), (window, np.abs(dW - dW_ref).max())
        assert np.array_equal(gx, gx_ref), (window, np.abs(gx - gx_ref).max())
        if k % 2 == 0:
            assert np.array_equal(db, db_ref), window


# ---- 2. the rounding point ----
def _bounds(x, g, W, window):
    """Per output (ref, bound): the float64 sums over operands rounded to bf16 on the CPU (db: over the unrounded g)
    and (n + 1) 2^-24 sum|a b|, the bound of n fp32 additions of exact products in ANY order."""
    xr, gr, Wr = D.rounded(x), D.rounded(g), D.rounded(W)
    dW, gx, _ = D.grads(xr, gr, Wr, window)
    mW, mx, _ = D.mags(xr, gr, Wr, window)
    g64 = g.double().numpy()
    nW, nx, nb = x.shape[0] * x.shape[2] * x.shape[3], 9 * W.shape[1], g.shape[0] * g.shape[2] * g.shape[3]
    return {'dW': (dW, (nW + 1) * U * mW), 'gx': (gx, (nx + 1) * U * mx),
            'db': (g64.sum(axis=(0, 2, 3)), (nb + 1) * U * np.abs(g64).sum(axis=(0, 2, 3)))}


def _check_bounds(got, x, g, W, window, what):
    """got: {'dW', 'gx', 'db'} float64 arrays of the kernel.  Returns {name: worst error / bound}."""
    fr = {}
    for name, (ref, bound) in _bounds(x, g, W, window).items():
        if got.get(name) is None:
            continue
        err = np.abs(got[name] - ref)
        fr[name] = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
        assert (err <= bound).all(), '%s %s: worst error / bound %.3g' % (what, name, fr[name])
    return fr


def test_operands_are_rounded_to_nearest_once_and_db_is_not(built_lib):
    rng = np.random.default_rng(5)
    B, Cin, Cout, H, W = 1, 24, 16, 7, 7
    window = (0, 0, 14, 14)
    x = torch.from_numpy(rng.standard_normal((B, Cin, H, W)).astype(np.float32))
    g = torch.from_numpy(rng.standard_normal((B, Cout, 14, 14)).astype(np.float32))
    Wt = torch.from_numpy(rng.standard_normal((Cin, Cout, 3, 3)).astype(np.float32))
    dW, db, gx = _run(x.numpy(), g.numpy(), Wt.numpy(), window)
    fr = _check_bounds(dict(dW=dW, gx=gx, db=db), x, g, Wt, window, 'rounding point')
    # (the statement discriminates: against the sums over the UNROUNDED operands the same bounds fail)
    eW, ex, _ = D.grads(x.numpy(), g.numpy(), Wt.numpy(), window)
    b = _bounds(x, g, Wt, window)
    missW = float((np.abs(dW - eW) > b['dW'][1]).mean())
    missx = float((np.abs(gx - ex) > b['gx'][1]).mean())
    print('bf16 deconv 24 -> 16 at 7x7: worst error / bound %.3g (dW), %.3g (gx), %.3g (db); outside the bound of '
          'the unrounded sums: %.3f (dW), %.3f (gx)' % (fr['dW'], fr['gx'], fr['db'], missW, missx))
    assert missW > 0.9 and missx > 0.9


# ---- 3. ties and direction ----
VALS = [1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -10, -(1 + 2.0 ** -8 + 2.0 ** -10),
        1 + 2.0 ** -7 - 2.0 ** -10]
WANT = [1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, -(1 + 2.0 ** -7), 1 + 2.0 ** -7]
TH, TW = 6, 20                  # two row tiles (4 rows each) and two column tiles (16 columns each) of input pixels
# positions of the single non-zero g inside the 13 x 41 full output: the four (row, column) parities; the last
# columns of the first tile's piece (31, and 32, which the second tile shares); the second row tile
G_POS = [(0, 0), (0, 1), (1, 0), (1, 1), (2, 31), (3, 32), (5, 33), (9, 4), (10, 35), (12, 40)]
X_POS = [(0, 0), (1, 15), (2, 16), (5, 19)]


def _exact(x, g, W):
    """The kernel's outputs equal the products of the CPU-rounded operands exactly (every sum has one term)."""
    dW, db, gx = _run(x.numpy(), g.numpy(), W.numpy(), None, want_db=False)
    rW, rx, _ = D.grads(D.rounded(x), D.rounded(g), D.rounded(W), None)
    assert np.array_equal(dW, rW) and np.array_equal(gx, rx)
    return rW, rx


def test_vals_are_ties_and_torch_rounds_them_to_even():
    v32 = torch.tensor(VALS, dtype=F32)
    assert v32.double().tolist() == VALS                         # float32 holds them
    assert v32.to(torch.bfloat16).double().tolist() == WANT      # torch's rounding on the CPU


@pytest.mark.parametrize('i,j', X_POS)
def test_ties_in_x(built_lib, i, j):
    # channel c of x holds value c at one pixel, g and W are 1: dW[c, 0, tap] = bf16(value c) for all nine taps
    x = torch.zeros((1, 5, TH, TW))
    x[0, :, i, j] = torch.tensor(VALS, dtype=F32)
    rW, _ = _exact(x, torch.ones((1, 1, 2 * TH + 1, 2 * TW + 1)), torch.ones((5, 1, 3, 3)))
    for c in range(5):
        assert (rW[c, 0] == WANT[c]).all()


@pytest.mark.parametrize('Y,X', G_POS)
def test_ties_in_g(built_lib, Y, X):
    # channel c of g holds value c at one position: with x = 1, dW[0, c, tap] is bf16(value c) at the taps that reach
    # it; with W = 1 and one value at a time, gx is bf16(value) at the pixels that reach it
    g = torch.zeros((1, 5, 2 * TH + 1, 2 * TW + 1))
    g[0, :, Y, X] = torch.tensor(VALS, dtype=F32)
    rW, _ = _exact(torch.ones((1, 1, TH, TW)), g, torch.ones((1, 5, 3, 3)))
    for c in range(5):
        assert set(np.unique(rW[0, c])) <= {0.0, WANT[c]} and (rW[0, c] == WANT[c]).any()
    for c in range(5):
        g1 = torch.zeros((1, 1, 2 * TH + 1, 2 * TW + 1))
        g1[0, 0, Y, X] = VALS[c]
        _, rx = _exact(torch.ones((1, 2, TH, TW)), g1, torch.ones((2, 1, 3, 3)))
        assert set(np.unique(rx)) == {0.0, WANT[c]}


@pytest.mark.parametrize('co,ky,kx', [(0, 0, 0), (0, 1, 2), (9, 2, 1), (39, 2, 2)])
def test_ties_in_W(built_lib, co, ky, kx):
    # input channel c of W holds value c at one (co, ky, kx), g is 1: gx[c] is bf16(value c) wherever that tap
    # reaches a position inside the full output -- everywhere
    W = torch.zeros((5, 40, 3, 3))
    W[:, co, ky, kx] = torch.tensor(VALS, dtype=F32)
    _, rx = _exact(torch.ones((1, 5, TH, TW)), torch.ones((1, 40, 2 * TH + 1, 2 * TW + 1)), W)
    for c in range(5):
        assert (rx[0, c] == WANT[c]).all()


# ---- 4. several slabs, twice ----
def test_several_slabs_give_the_same_bits_twice_within_the_bound(built_lib):
    from iterative_inference_segm_amd import _lib, ops
    rng = np.random.default_rng(5)
    B, Cin, Cout, H, W = 3, 20, 24, 37, 50
    window = (0, 0, 2 * H, 2 * W)
    x = torch.from_numpy(rng.standard_normal((B, Cin, H, W)).astype(np.float32))
    g = torch.from_numpy(rng.standard_normal((B, Cout, 2 * H, 2 * W)).astype(np.float32))
    Wt = torch.from_numpy(rng.standard_normal((Cin, Cout, 3, 3)).astype(np.float32))
    assert _lib.load().iiseg_deconv_wgrad_bf16_slabs(C.byref(ops.deconv_desc(x.shape, Cout, 3, 2, window))) >= 2
    runs = [_run(x.numpy(), g.numpy(), Wt.numpy(), window) for _ in range(2)]
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    dW, db, gx = runs[0]
    fr = _check_bounds(dict(dW=dW, gx=gx, db=db), x, g, Wt, window, 'several slabs')
    print('bf16 deconv 3x20x37x50 -> 24: worst error / bound %.3g (dW), %.3g (gx), %.3g (db)'
          % (fr['dW'], fr['gx'], fr['db']))


# ---- 5. the module ----
class _Recorder:
    """ops.deconv_wgrad and ops.deconv_dgrad, recording every call's operands (copied), targets and mode."""

    def __init__(self, ops):
        self.ops, self.wgrad, self.dgrad, self.w, self.d = ops, ops.deconv_wgrad, ops.deconv_dgrad, [], []

    def _wgrad(self, x, g, dW, db, stride, window=None, mma='f32'):
        self.w.append(dict(x=x.detach().cpu().clone(), g=g.detach().cpu().clone(), dW=dW, db=db, stride=stride,
                           window=window, mma=mma))
        return self.wgrad(x, g, dW, db, stride, window=window, mma=mma)

    def _dgrad(self, g, W, stride, x_hw, window=None, mma='f32'):
        gx = self.dgrad(g, W, stride, x_hw, window=window, mma=mma)
        self.d.append(dict(g=g.detach().cpu().clone(), W=W.detach().cpu().clone(), gx=gx.detach().cpu().clone(),
                           Wptr=W.data_ptr(), stride=stride, x_hw=tuple(x_hw), window=window, mma=mma))
        return gx

    def __enter__(self):
        self.ops.deconv_wgrad, self.ops.deconv_dgrad = self._wgrad, self._dgrad
        return self

    def __exit__(self, *exc):
        self.ops.deconv_wgrad, self.ops.deconv_dgrad = self.wgrad, self.dgrad


CASES = {'thin': R.THIN, 'wide': R.WIDE}
_CASES = {}


def _model_case(name):
    if name not in _CASES:
        _CASES[name] = R.make_case(CASES[name], seed=3)
    return _CASES[name]


def _net(name, deconv, **kw):
    from iterative_inference_segm_amd.densenet import FCDenseNet
    cfg = CASES[name]
    return FCDenseNet(_model_case(name)[0], cfg['n_classes'], layer=[], n_layers_per_block=cfg['nlpb'],
                      n_pool=cfg['n_pool'], growth=cfg['growth'], dtype=F32, mma='f32', trainable=True, deconv=deconv,
                      **kw)


def _same(a, b):
    if torch.is_tensor(a):
        return torch.equal(a, b)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)
    return a == b


def _clone(v):
    if torch.is_tensor(v):
        return v.clone()
    if isinstance(v, (list, tuple)):
        return [_clone(u) for u in v]
    if isinstance(v, dict):
        return {k: _clone(u) for k, u in v.items()}
    return v


@pytest.mark.parametrize('name', list(CASES))
def test_module_changes_only_what_the_transition_up_gradients_reach(built_lib, name):
    from iterative_inference_segm_amd import ops
    cfg = CASES[name]
    params, x, T, keeps = _model_case(name)
    xd, Td, kd = _dev(x), _dev(T), [_dev(k) for k in keeps]
    dead = {li for li, _ in R.dead_arrays(cfg)}
    out = {}
    for mode in ('f32', 'bf16'):
        net = _net(name, mode)
        assert net.deconv == mode and net.wgrad == 'f32'
        score = net.forward_train(xd, kd)
        res, g, _ = ops.ctx_loss(score, Td, ('crossentropy',), 1.0)
        prof = []
        ops.CONV_PROFILE = prof
        try:
            with _Recorder(ops) as rec:
                grads = net.backward(g)
            torch.cuda.synchronize()
        finally:
            ops.CONV_PROFILE = None
        launched = [k for k, _, _, _ in prof if k.startswith('deconv_')]
        tus = [e for e in reversed(net._steps) if e['kind'] == 'tu']      # in the order `backward` walks them
        assert len(rec.w) == len(rec.d) == len(tus) == cfg['n_pool']      # one call of each per TransitionUp
        new = ['deconv_wgrad_bf16_kernel', 'deconv_dgrad_bf16_kernel']
        assert launched == (new if mode == 'bf16' else ['deconv_wgrad_kernel', 'deconv_dgrad_kernel']) * len(tus)
        worst = {}
        for k, (cw, cd, e) in enumerate(zip(rec.w, rec.d, tus)):
            L = net.layers[e['li']]
            dW, db = grads['conv%03d' % e['li']]
            win = tuple(net.saved_maps()['win'][e['li']])
            assert cw['mma'] == cd['mma'] == mode and cw['stride'] == cd['stride'] == 2
            assert tuple(cw['window']) == tuple(cd['window']) == win
            assert cw['dW'].data_ptr() == dW.data_ptr() and cw['db'].data_ptr() == db.data_ptr()
            assert cd['Wptr'] == L['conv'].W.data_ptr()                    # the layer's own fp32 parameter
            assert cw['x'].shape[1] == e['n'] - e['block0'] and cw['g'].shape[1] == e['keep']
            assert torch.equal(cw['g'], cd['g']) and cd['x_hw'] == tuple(cw['x'].shape[2:])
            if mode == 'bf16':
                got = dict(dW=dW.cpu().double().numpy(), db=db.cpu().double().numpy(),
                           gx=cd['gx'].double().numpy())
                fr = _check_bounds(got, cw['x'], cw['g'], cd['W'], win, '%s tu %d' % (name, k))
                worst = {n: max(worst.get(n, 0.0), v) for n, v in fr.items()}
            if e['li'] in dead:
                mag = cw['g'].double().abs().sum(dim=(0, 2, 3))
                assert bool((db.cpu().double().abs() <= 1e-6 * mag).all()), (mode, k)
        loss = res.clone()
        out[mode] = dict(score=score.clone(), loss=loss, saved=_clone(net.saved_maps()), worst=worst,
                         grads={n: (a.clone(), b.clone()) for n, (a, b) in grads.items()},
                         last_tu=max(e['li'] for e in tus), tus=['conv%03d' % e['li'] for e in tus])
    a, b = out['f32'], out['bf16']
    assert torch.equal(a['score'], b['score']) and torch.equal(a['loss'], b['loss'])
    assert _same(a['saved'], b['saved'])
    after = [n for n in a['grads'] if int(n[-3:]) > a['last_tu']]         # the last dense block, the score layer
    assert len(after) == 2 * cfg['nlpb'][-1] + 1
    for n in after:
        assert torch.equal(a['grads'][n][0], b['grads'][n][0]) and torch.equal(a['grads'][n][1], b['grads'][n][1]), n
    assert any(not torch.equal(a['grads'][n][0], b['grads'][n][0]) for n in a['tus'])
    cos, rel = {}, {}
    for n in a['grads']:
        for k in (0, 1):
            assert bool(torch.isfinite(b['grads'][n][k]).all()) and bool(torch.isfinite(a['grads'][n][k]).all()), n
            u, v = b['grads'][n][k].double().reshape(-1), a['grads'][n][k].double().reshape(-1)
            if n in a['tus'] and k == 1 and int(n[-3:]) in dead:
                continue                                                   # a sum that cancels: no direction
            cos[(n, k)] = float(u @ v / (u.norm() * v.norm()))
            rel[(n, k)] = float((u - v).abs().max() / v.abs().max())
    print('FC-DenseNet (%s) deconv bf16 against f32: worst error / bound %s; over %d arrays: lowest cosine %.6f, '
          'max relative difference %.3g; TransitionUp dW: %s'
          % (name, {n: '%.3g' % v for n, v in b['worst'].items()}, len(cos), min(cos.values()), max(rel.values()),
             {n: 'cos %.6f rel %.3g' % (cos[(n, 0)], rel[(n, 0)]) for n in a['tus']}))


# ---- 6. training ----
def _trainer(deconv, **kw):
    from iterative_inference_segm_amd.train import DenseNetTrainer
    C_ = R.THIN['n_classes']
    return DenseNetTrainer(_net('thin', deconv), C_, [C_], **kw)


def test_loss_goes_down_over_40_steps_with_bf16_transition_up_gradients(built_lib):
    x, T = _model_case('thin')[1:3]
    tr = _trainer('bf16', learning_rate=1e-3, seed=2)
    xd, Td = _dev(x), _dev(T)
    losses = [tr.train_step(xd, Td) for _ in range(40)]
    losses = [float(v) for v in torch.stack(losses).cpu()]
    print('FC-DenseNet loss, deconv bf16, steps 0-9: %.5f, steps 30-39: %.5f'
          % (np.mean(losses[:10]), np.mean(losses[-10:])))
    assert np.all(np.isfinite(losses))
    assert np.mean(losses[-10:]) < np.mean(losses[:10])


def test_two_runs_are_identical_and_one_step_differs_from_the_f32_mode(built_lib):
    x, T, keeps = _model_case('thin')[1:4]
    xd, Td, kd = _dev(x), _dev(T), [_dev(k) for k in keeps]
    flats = {}
    for key, mode in (('a', 'bf16'), ('b', 'bf16'), ('f32', 'f32')):
        tr = _trainer(mode, learning_rate=1e-2, weight_decay=1e-4, seed=3)
        tr.train_step(xd, Td, kd)
        torch.cuda.synchronize()
        flats[key + '1'] = tr.net.flat.clone()
        tr.train_step(xd, Td)                                    # masks from the seeded generator
        torch.cuda.synchronize()
        flats[key + '2'] = tr.net.flat.clone()
    assert torch.equal(flats['a1'], flats['b1']) and torch.equal(flats['a2'], flats['b2'])
    assert bool(torch.isfinite(flats['a2']).all())
    assert not torch.equal(flats['a1'], flats['f321'])           # the mode took effect in ONE step


# ---- 7. the driver ----
def test_driver_end_to_end_with_bf16_wgrad_and_deconv(built_lib, tmp_path):
    from iterative_inference_segm_amd.densenet import build_fcdensenet
    save = str(tmp_path / 'save')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_fcdensenet.py'), '--synthetic', '--num_epochs', '2',
                        '--n_images', '2', '--image_size', '16', '16', '--batch_size', '[2, 2, 2]', '--savepath', save,
                        '--layers_per_block', '[2, 3, 2, 3, 2]', '--growth', '4', '--n_first', '8',
                        '--max_batches', '1', '--wgrad', 'bf16', '--deconv', 'bf16'], capture_output=True, text=True,
                       cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert os.listdir(os.path.join(save, 'camvid')) == ['fc_densenet']       # the fp32 run's folder
    folder = os.path.join(save, 'camvid', 'fc_densenet')
    config = open(os.path.join(folder, 'config.txt')).read().splitlines()
    assert 'deconv = bf16' in config and 'wgrad = bf16' in config
    assert 'FC-DenseNet103_weights_best.npz' in os.listdir(folder)           # ... and its checkpoint name
    net = build_fcdensenet(layer=[], n_classes=11, weight_path=os.path.join(folder, 'FC-DenseNet103_weights_best.npz'))
    x = _dev(np.random.default_rng(1).random((2, 3, 16, 16)))
    probs = net(x)[-1]
    assert tuple(probs.shape) == (2, 11, 16, 16) and bool(torch.isfinite(probs).all())
