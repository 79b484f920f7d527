"""GPU: training FCN-8 -- the 'valid' K x K weight gradient (csrc/conv_wgrad_kxk.hip: float32
on the matrix pipe, float64 on the vector ALU), the transposed convolution's data and weight gradients
(csrc/deconv_grad.hip), relu_gate and the L2 term (csrc/fcn8_train.hip), bit for bit on data where every sum is
exact; FCN8.forward_train / backward / refresh, the trainer and train_fcn8.py against the float64 restatement
(tests/fcn8_train_ref.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fcn8_train_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {'f32': torch.float32, 'f64': torch.float64}


def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda().contiguous()


# ---- 1. K x K weight gradient, exact on small-integer data ----
def _wgrad_ref(x, gz, K):
    """dW[co, ci, ky, kx] = sum gz[b, co, y, x] x[b, ci, y + ky, x + kx], db[co] = sum gz (in the dtype handed in)."""
    OH, OW = gz.shape[2:]
    dW = np.zeros((gz.shape[1], x.shape[1], K, K), dtype=x.dtype)
    for ky in range(K):
        for kx in range(K):
            dW[:, :, ky, kx] = np.tensordot(gz, x[:, :, ky:ky + OH, kx:kx + OW], axes=([0, 2, 3], [0, 2, 3]))
    return dW, gz.sum(axis=(0, 2, 3))


CHANNELS = [(5, 3), (64, 11), (33, 130), (130, 64)]
# (K, H, W of x): K = 7 from one output pixel up; K = 1 from one pixel to a map that needs several slabs; K = 3
GEOMETRY = [(7, 7, 7), (7, 8, 9), (7, 13, 13), (7, 20, 37), (1, 1, 1), (1, 7, 7), (1, 26, 27), (1, 37, 150), (3, 14, 13)]
OFF = (2, 3)                # the window's origin inside the larger map x is read from
MARGIN = (5, 7)             # ... which is this much larger


@pytest.mark.parametrize('K,H,W', GEOMETRY)
@pytest.mark.parametrize('Cin,Cout', CHANNELS)
def test_kxk_weight_gradient_is_exact_on_integers(built_lib, Cin, Cout, K, H, W):
    from iterative_inference_segm_amd import _lib, ops
    lo, hi = 3, 5
    for B in (1, 3):
        rng = np.random.default_rng(Cin * 1000 + Cout + 7 * B + H + 3 * K)
        x = rng.integers(-2, 3, size=(B, Cin, H, W))
        gz = rng.integers(-2, 3, size=(B, Cout, H - K + 1, W - K + 1))
        if gz.size > 4:
            gz[rng.integers(0, 2, size=gz.shape) == 0] = 0       # as behind a ReLU mask
        dW_ref, db_ref = _wgrad_ref(x, gz, K)
        assert np.abs(dW_ref).max() < 2 ** 24 and np.abs(db_ref).max() < 2 ** 24
        xmap = np.full((B, Cin, H + MARGIN[0], W + MARGIN[1]), 777)
        xmap[:, :, OFF[0]:OFF[0] + H, OFF[1]:OFF[1] + W] = x
        win = OFF + (H, W)
        for prec in ('f32', 'f64'):
            dt = DT[prec]
            xd, gzd = _dev(xmap, dt), _dev(gz, dt)
            d = ops.conv_wgrad_kxk_desc(xd, Cout, K, win)
            nslab = _lib.load().iiseg_conv_wgrad_kxk_slabs(C.byref(d), 4 if prec == 'f32' else 8)
            if (H, W) == (37, 150):
                assert nslab >= 2                                # slabs + the finalize launch
            if (H, W) in ((1, 1), (7, 7)) and B == 1:
                assert nslab == 1                                # straight into dW
            # the layer's own array, W[out, in, K, K], with db
            dW = torch.full(dW_ref.shape, 7.0, dtype=dt, device='cuda')
            db = torch.full((Cout,), 7.0, dtype=dt, device='cuda')
            ops.conv_wgrad_kxk(xd, gzd, dW, db, window=win)
            # the middle of a larger parameter, in both layouts: with db, and once with db = NULL
            big = torch.full((Cout, lo + Cin + hi, K, K), -9.0, dtype=dt, device='cuda')
            db2 = torch.full((Cout,), 7.0, dtype=dt, device='cuda')
            ops.conv_wgrad_kxk(xd, gzd, big, db2, window=win, ci0=lo)
            bigT = torch.full((lo + Cin + hi, Cout, K, K), -9.0, dtype=dt, device='cuda')
            ops.conv_wgrad_kxk(xd, gzd, bigT, None, window=win, ci0=lo, layout='iohw')
            torch.cuda.synchronize()
            assert np.array_equal(dW.cpu().numpy(), dW_ref.astype(np.float64)), (B, prec)
            assert np.array_equal(db.cpu().numpy(), db_ref.astype(np.float64)), (B, prec)
            assert np.array_equal(db2.cpu().numpy(), db_ref.astype(np.float64)), (B, prec)
            want = np.full(tuple(big.shape), -9.0)
            want[:, lo:lo + Cin] = dW_ref
            assert np.array_equal(big.cpu().numpy(), want), (B, prec)              # every sentinel intact
            assert np.array_equal(bigT.cpu().numpy(), want.transpose(1, 0, 2, 3)), (B, prec)
            assert np.array_equal(xd.cpu().numpy(), xmap.astype(np.float64))


@pytest.mark.parametrize('prec', ['f32', 'f64'])
@pytest.mark.parametrize('K,H,W', [(7, 20, 37), (1, 37, 150)])
def test_kxk_weight_gradient_real_data(built_lib, prec, K, H, W):
    """No atomics, fixed slab order: two runs give the same bits.  float32 against float64 numpy: the bound is 4 x
    the error numpy float32 makes on the same operands (DESIGN.md section 12's rule).  float64 has no finer
    reference to measure numpy's own error against: there the bound is that of ANY summation order of the n fused
    multiply-adds, n u sum|a b| per entry."""
    from iterative_inference_segm_amd import ops
    dt = DT[prec]
    rng = np.random.default_rng(5 + K)
    B, Cin, Cout = 3, 33, 20
    x = rng.standard_normal((B, Cin, H, W)).astype(np.float32)
    gz = rng.standard_normal((B, Cout, H - K + 1, W - K + 1)).astype(np.float32)
    xd, gzd = _dev(x, dt), _dev(gz, dt)
    runs = []
    for _ in range(2):
        dW = torch.zeros((Cout, Cin, K, K), dtype=dt, device='cuda')
        db = torch.zeros(Cout, dtype=dt, device='cuda')
        ops.conv_wgrad_kxk(xd, gzd, dW, db)
        runs.append((dW.cpu().numpy(), db.cpu().numpy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    ref = _wgrad_ref(x.astype(np.float64), gz.astype(np.float64), K)
    if prec == 'f32':
        np32 = _wgrad_ref(x, gz, K)
        assert np32[0].dtype == np.float32
        for got, r, n32, what in zip(runs[0], ref, np32, ('dW', 'db')):
            err, ref_err = np.abs(got - r).max(), np.abs(n32.astype(np.float64) - r).max()
            print('K x K wgrad f32 K=%d %s: max error %.3g, numpy float32 %.3g' % (K, what, err, ref_err))
            assert err <= 4 * ref_err
    else:
        n = B * (H - K + 1) * (W - K + 1)
        mag = _wgrad_ref(np.abs(x).astype(np.float64), np.abs(gz).astype(np.float64), K)
        for got, r, m in zip(runs[0], ref, mag):
            assert (np.abs(got - r) <= (n + 1) * 2.0 ** -53 * m).all()


# ---- 2. transposed-convolution gradients, exact on small-integer data ----
def _windows(fullH, fullW, s):
    """The full output, the centred crop, a crop at an offset that is no multiple of the stride, a window
    narrower than one stride -- each cut to what the full output holds."""
    ch, cw = max(1, fullH - s - 1), max(1, fullW - s - 1)
    wins = [(0, 0, fullH, fullW), ((fullH - ch) // 2, (fullW - cw) // 2, ch, cw)]
    oy, ox = min(s + 1, fullH - 1), min(1, fullW - 1)
    wins.append((oy, ox, fullH - oy, max(1, fullW - ox - 1)))
    wins.append((min(1, fullH - 1), min(s + 1, fullW - 1), 1, max(1, min(s - 1, fullW - min(s + 1, fullW - 1)))))
    return wins


@pytest.mark.parametrize('K,s', [(4, 2), (16, 8), (3, 2)])
@pytest.mark.parametrize('Cin,Cout', [(4, 7), (11, 11), (21, 21)])
def test_deconv_gradients_are_exact_on_integers(built_lib, K, s, Cin, Cout):
    from iterative_inference_segm_amd import ops
    rng = np.random.default_rng(K * 100 + s + Cin)
    W = rng.integers(-2, 3, size=(Cin, Cout, K, K))
    offs = set()
    for H, Wd in ((1, 1), (2, 3), (7, 6)):
        for B in (1, 3):
            x = rng.integers(-2, 3, size=(B, Cin, H, Wd))
            for win in _windows((H - 1) * s + K, (Wd - 1) * s + K, s):
                offs.add((win[0] % s, win[1] % s, win[3] < s))
                g = rng.integers(-2, 3, size=(B, Cout, win[2], win[3]))
                gx_ref, dW_ref, db_ref = R.deconv_bwd(x, W, g, s, win)
                assert max(np.abs(gx_ref).max(), np.abs(dW_ref).max(), np.abs(db_ref).max()) < 2 ** 24
                for prec in ('f32', 'f64'):
                    dt = DT[prec]
                    xd, gd, Wdv = _dev(x, dt), _dev(g, dt), _dev(W, dt)
                    gx = ops.deconv_dgrad(gd, Wdv, s, (H, Wd), window=win)
                    dW = torch.full((Cin, Cout, K, K), 7.0, dtype=dt, device='cuda')
                    db = torch.full((Cout,), 7.0, dtype=dt, device='cuda')
                    ops.deconv_wgrad(xd, gd, dW, db, s, window=win)
                    dW2 = torch.full((Cin, Cout, K, K), 7.0, dtype=dt, device='cuda')
                    ops.deconv_wgrad(xd, gd, dW2, None, s, window=win)
                    torch.cuda.synchronize()
                    tag = (H, Wd, B, win, prec)
                    assert np.array_equal(gx.cpu().numpy(), gx_ref.astype(np.float64)), tag
                    assert np.array_equal(dW.cpu().numpy(), dW_ref.astype(np.float64)), tag
                    assert np.array_equal(dW2.cpu().numpy(), dW_ref.astype(np.float64)), tag
                    assert np.array_equal(db.cpu().numpy(), db_ref.astype(np.float64)), tag
    assert any(o[0] or o[1] for o in offs) and any(o[2] for o in offs)    # the windows the docstring names occur


@pytest.mark.parametrize('K,s', [(4, 2), (16, 8), (3, 2)])
def test_deconv_dgrad_is_the_adjoint_of_the_forward_kernel(built_lib, K, s):
    """<g_x, x'> = <g, deconv(x')> in float64 against the existing forward kernel, both sides in the window."""
    from iterative_inference_segm_amd import ops
    dt = torch.float64
    rng = np.random.default_rng(K + s)
    Cin, Cout, B, H, Wd = 11, 11, 3, 7, 6
    W = _dev(rng.standard_normal((Cin, Cout, K, K)), dt)
    fwd = ops.Deconv(W, None, s, dtype=dt)
    for win in _windows((H - 1) * s + K, (Wd - 1) * s + K, s):
        g = _dev(rng.standard_normal((B, Cout, win[2], win[3])), dt)
        x2 = _dev(rng.standard_normal((B, Cin, H, Wd)), dt)
        gx = ops.deconv_dgrad(g, W, s, (H, Wd), window=win)
        lhs, rhs = float((gx * x2).sum()), float((g * fwd(x2, window=win)).sum())
        scale = float(g.abs().sum()) * float(x2.abs().max()) * float(W.abs().max())
        print('deconv adjoint K=%d s=%d window %s: %.15g vs %.15g' % (K, s, win, lhs, rhs))
        assert abs(lhs - rhs) <= 1e-12 * max(1.0, scale)
        # and the weight gradient against the same forward: <dW, W'> + <db, b'> = <g, deconv_{W', b'}(x)>
        W2, b2 = _dev(rng.standard_normal((Cin, Cout, K, K)), dt), _dev(rng.standard_normal(Cout), dt)
        dW, db = torch.zeros_like(W2), torch.zeros_like(b2)
        ops.deconv_wgrad(x2, g, dW, db, s, window=win)
        lhs = float((dW * W2).sum() + (db * b2).sum())
        rhs = float((g * ops.Deconv(W2, b2, s, dtype=dt)(x2, window=win)).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(1.0, scale * K * K)


# ---- 3. relu_gate and the L2 term ----
@pytest.mark.parametrize('prec', ['f32', 'f64'])
def test_relu_gate_and_l2_term_are_exact_on_integers(built_lib, prec):
    from iterative_inference_segm_amd import ops
    dt = DT[prec]
    rng = np.random.default_rng(3)
    for shape in ((1, 1, 1, 1), (2, 5, 7, 9), (3, 33, 65, 67)):
        g, out = rng.integers(-3, 4, size=shape), rng.integers(-2, 3, size=shape)   # zeros in `out`: relu'(0) = 0
        want = np.where(out > 0, g, 0).astype(np.float64)
        gd, od = _dev(g, dt), _dev(out, dt)
        assert np.array_equal(ops.relu_gate(gd, od).cpu().numpy(), want)
        assert np.array_equal(gd.cpu().numpy(), g.astype(np.float64))
        assert ops.relu_gate(gd, od, dst=gd) is gd and np.array_equal(gd.cpu().numpy(), want)    # in place
    # the L2 term: W ranges of odd sizes, one longer than a workgroup's stride, biases between them
    sizes = [(27, 4), (1, 1), (70001, 130), (9, 3)]
    n = sum(a + b for a, b in sizes)
    p, g0 = rng.integers(-3, 4, size=n), rng.integers(-5, 6, size=n)
    ranges, off = [], 0
    for a, b in sizes:
        ranges.append((off, off + a))
        off += a + b
    wd = 0.25                                                   # 2 wd W is exact
    pd, gd = _dev(p, dt), _dev(g0, dt)
    pen = ops.l2_term(pd, gd, ranges, wd)
    torch.cuda.synchronize()
    want, sq = g0.astype(np.float64), 0.0
    for lo, hi in ranges:
        want[lo:hi] += 2 * wd * p[lo:hi]
    sq = np.sum(np.concatenate([p[lo:hi] for lo, hi in ranges]).astype(np.float64) ** 2)
    assert np.array_equal(gd.cpu().numpy(), want)               # biases untouched
    assert np.array_equal(pd.cpu().numpy(), p.astype(np.float64))
    assert pen.dtype == torch.float64 and float(pen[0]) == float(sq)             # to the last bit


# ---- 4. the module on the small net ----
GEOMS = {'26x30': (3, 26, 30), '64x58': (2, 64, 58)}
_CASES = {}


def _model_case(geom):
    """(params, x, T, keep6, keep7, float64 loss, float64 gradients, float64 maps): computed once, shared."""
    if geom not in _CASES:
        B, H, W = GEOMS[geom]
        params, x, T, k6, k7 = R.make_case(B, H, W, seed=5)
        loss, grads, net = R.loss_and_param_grads(params, x, T, k6, k7)
        _CASES[geom] = (params, x, T, k6, k7, loss, grads, net)
    return _CASES[geom]


def _fcn8(params, dt, **kw):
    from iterative_inference_segm_amd.fcn8 import FCN8
    return FCN8(params, R.SMALL['n_classes'], layer=['score'], dtype=dt, mma='f32', trainable=True, **kw)


def _gpu_backward(geom, dt):
    from iterative_inference_segm_amd import ops
    params, x, T, k6, k7 = _model_case(geom)[:5]
    net = _fcn8(params, dt)
    score = net.forward_train(_dev(x, dt), _dev(k6, dt), _dev(k7, dt))
    res, g, _ = ops.ctx_loss(score, _dev(T, dt), ('crossentropy',), 1.0)
    grads = net.backward(g)
    torch.cuda.synchronize()
    return net, res, g, {n: (a.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64))
                         for n, (a, b) in grads.items()}


def _ref_maps(saved, dtype):
    """FCN8.saved_maps() as the dict tests/fcn8_train_ref.backward reads."""
    s = {k: (v.cpu().numpy().astype(dtype) if torch.is_tensor(v) else v) for k, v in saved.items()}
    for sname, pool in (('score_pool4', 'pool4'), ('score_pool3', 'pool3')):
        oy, ox, H, W = s['win_' + sname]
        s['in_' + sname] = np.ascontiguousarray(s[pool][:, :, oy:oy + H, ox:ox + W])
    s['p'], s['pad'] = 0.5, 100
    return s


def _rel_err(got, ref):
    """max over the arrays of max|got - ref| / max|ref|"""
    worst = 0.0
    for n in ref:
        for a, b in zip(got[n], ref[n]):
            assert a.shape == b.shape, n
            worst = max(worst, float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max()))
    return worst


F64_BOUND = 1e-13          # rounding only: DESIGN.md section 12's bound


@pytest.mark.parametrize('geom', list(GEOMS))
def test_whole_backward_f64(built_lib, geom):
    """Measured on an MI355X (26x30 / 64x58): max relative error 5.3e-15 / 3.7e-15."""
    loss_ref, ref, net64 = _model_case(geom)[5:8]
    net, res, _, got = _gpu_backward(geom, torch.float64)
    B, H, W = GEOMS[geom]
    assert tuple(net.saved_maps()['fc6'].shape[2:]) == R.fc6_hw(H, W) == ((1, 1) if geom == '26x30' else (2, 2))
    if geom == '64x58':
        assert net.saved_maps()['conv2_2'].shape[2] == 131 and net.saved_maps()['pool2'].shape[2] == 65   # odd maps
    assert sorted(got) == sorted(R.PARAM_ORDER)
    for n in ref:
        assert np.abs(ref[n][0]).max() > 0 and np.abs(ref[n][1]).max() > 0, n       # every layer is alive
    err = _rel_err(got, ref)
    print('FCN-8 backward f64 (%s): max relative error %.3g (loss %.12f / %.12f)' % (geom, err, float(res[0]), loss_ref))
    assert abs(float(res[0]) - loss_ref) <= 1e-12 * abs(loss_ref)
    assert err <= F64_BOUND


@pytest.mark.parametrize('geom', list(GEOMS))
def test_whole_backward_f32(built_lib, geom):
    """Teacher-forced: the restatement ON the float32 forward's saved maps, masks and g_score (the same ReLU / pool
    decisions, rounding only).  The bound is 4 x the error numpy float32 makes on the same maps against float64.
    Free-running float32 against free-running float64: the number of differing decisions and every array's cosine
    are reported (DESIGN.md section 14 holds the figures); nothing beyond finiteness is asserted on them.
    Measured on an MI355X (26x30 / 64x58): teacher-forced 8.1e-07 / 2.09e-06, numpy float32 5.9e-07 / 9.7e-07, no
    differing decision, cosine 1.000000 on every array."""
    params, x, T, k6, k7, _, free, net64 = _model_case(geom)
    net, res, g, got = _gpu_backward(geom, torch.float32)
    saved = net.saved_maps()
    g32 = g.cpu().numpy()
    ref = R.backward(params, _ref_maps(saved, np.float64), g32.astype(np.float64))
    p32 = {k: tuple(a.astype(np.float32) for a in v) for k, v in params.items()}
    np32 = R.backward(p32, _ref_maps(saved, np.float32), g32)
    assert all(a.dtype == np.float32 for v in np32.values() for a in v)
    ref_err, err = _rel_err(np32, ref), _rel_err(got, ref)
    flips = sum(int((a != b).sum()) for a, b in zip(R.decisions(_ref_maps(saved, np.float64)), R.decisions(net64)))
    cat = lambda v: np.concatenate([a.ravel() for a in v])
    cos = {n: float(cat(got[n]) @ cat(free[n]) / (np.linalg.norm(cat(got[n])) * np.linalg.norm(cat(free[n]))))
           for n in free}
    print('FCN-8 backward f32 (%s): teacher-forced max relative error %.3g, numpy float32 %.3g; free-running: %d '
          'differing decisions, gradient cosine per array %s'
          % (geom, err, ref_err, flips, {n: '%.6f' % c for n, c in cos.items()}))
    assert err <= 4 * ref_err
    assert all(np.isfinite(a).all() for v in got.values() for a in v) and np.isfinite(list(cos.values())).all()


def _trainer(geom, dt, **kw):
    from iterative_inference_segm_amd.train import FCN8Trainer
    C_ = R.SMALL['n_classes']
    return FCN8Trainer(_fcn8(_model_case(geom)[0], dt), C_, [C_], **kw)


def test_first_five_steps_match_the_restatement_f64(built_lib):
    """Adam, weight_decay 1e-4, fixed dropout masks; bound: a relative 1e-9 (DESIGN.md section 12 measured 1e-12 on
    twelve layers, this net is 21 deep).  Measured on an MI355X: 2.4e-16."""
    params, x, T, k6, k7 = _model_case('26x30')[:5]
    dt = torch.float64
    wd, lr = 1e-4, 1e-4
    tr = _trainer('26x30', dt, learning_rate=lr, weight_decay=wd)
    xd, Td, k6d, k7d = _dev(x, dt), _dev(T, dt), _dev(k6, dt), _dev(k7, dt)
    flat = R.flatten(params)
    m, v, state = np.zeros_like(flat), np.zeros_like(flat), (0, 1.0, 1.0)
    worst = 0.0
    for step in range(5):
        loss = float(tr.train_step(xd, Td, k6d, k7d))
        loss_ref, grads, _ = R.loss_and_param_grads(R.unflatten(flat, params), x, T, k6, k7, wd)
        flat, m, v, state = R.adam_step(flat, R.flatten(grads), m, v, state, lr)
        worst = max(worst, abs(loss - loss_ref) / abs(loss_ref))
        print('step %d: loss %.12f restatement %.12f' % (step, loss, loss_ref))
        assert abs(loss - loss_ref) <= 1e-9 * abs(loss_ref)
    print('FCN-8 five float64 steps: worst relative loss difference %.3g' % worst)
    assert float(tr.state[0]) == 5.0


def test_train_step_is_deterministic_and_every_path_sees_the_new_weights(built_lib, tmp_path):
    from iterative_inference_segm_amd.fcn8 import FCN8, PARAM_ORDER, buildFCN8
    from iterative_inference_segm_amd.weights import load_param_list, save_param_list
    params, x, T, k6, k7 = _model_case('26x30')[:5]
    dt = torch.float32
    xd, Td, k6d, k7d = _dev(x, dt), _dev(T, dt), _dev(k6, dt), _dev(k7, dt)
    flats = []
    for _ in range(2):
        tr = _trainer('26x30', dt, learning_rate=1e-2, weight_decay=1e-4, seed=3)
        before = tr.net.forward_train(xd, deterministic=True).clone()    # packed weights exist BEFORE the steps
        tr.train_step(xd, Td, k6d, k7d)
        tr.train_step(xd, Td)                                            # masks from the seeded generator
        torch.cuda.synchronize()
        flats.append(tr.net.flat.clone())
    assert torch.equal(flats[0], flats[1])                               # two identical runs: identical bits
    assert not torch.equal(flats[0], _dev(R.flatten(params), dt))
    assert bool(torch.isfinite(flats[0]).all())
    # after refresh(): the trained module, a fresh inference module on the direct kernels, and one built from
    # the saved checkpoint compute the same bits
    after = tr.net.forward_train(xd, deterministic=True).clone()
    assert not torch.equal(after, before)
    C_ = R.SMALL['n_classes']
    fresh = FCN8(tr.net.state_arrays(), C_, layer=['score'], dtype=dt, mma='f32')
    path = str(tmp_path / 'new_fcn8_model_best.npz')
    save_param_list(path, tr.net.state_arrays(), PARAM_ORDER)
    loaded = buildFCN8(3, path_weights=path, n_classes=C_, layer=['score'], dtype=dt)
    for net in (fresh, loaded):
        for conv in net.convs.values():
            conv.wino = conv.wino_f64 = False                            # the direct kernels only
        assert torch.equal(net(xd)[0], after)
    again = _fcn8(load_param_list(path, PARAM_ORDER), dt)
    assert torch.equal(again.flat, tr.net.flat)
    assert torch.equal(again.forward_train(xd, deterministic=True), after)
    # the data-gradient layers too: one more step on the trained module and on the one from the checkpoint
    from iterative_inference_segm_amd.train import FCN8Trainer
    tr2 = FCN8Trainer(again, C_, [C_], learning_rate=1e-2, weight_decay=1e-4)
    for t in (tr, tr2):
        t.s1.zero_()
        t.s2.zero_()
        t.state.copy_(torch.tensor([0.0, 1.0, 1.0]))
        t.train_step(xd, Td, k6d, k7d)
    assert torch.equal(tr.net.flat, tr2.net.flat)


def test_loss_goes_down_over_40_steps_f32(built_lib):
    x, T = _model_case('26x30')[1:3]
    dt = torch.float32
    tr = _trainer('26x30', dt, learning_rate=1e-3, seed=2)
    xd, Td = _dev(x, dt), _dev(T, dt)
    losses = [tr.train_step(xd, Td) for _ in range(40)]
    losses = [float(v) for v in torch.stack(losses).cpu()]
    print('FCN-8 loss, steps 0-9: %.5f, steps 30-39: %.5f' % (np.mean(losses[:10]), np.mean(losses[-10:])))
    assert np.all(np.isfinite(losses))
    assert np.mean(losses[-10:]) < np.mean(losses[:10])


# ---- 5. the driver end to end ----
def test_driver_end_to_end(built_lib, tmp_path):
    from iterative_inference_segm_amd import ops
    from iterative_inference_segm_amd.fcn8 import FCN8, PARAM_ORDER, buildFCN8
    from iterative_inference_segm_amd.weights import load_param_list
    save = str(tmp_path / 'save')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_fcn8.py'), '--synthetic', '--num_epochs', '2',
                        '--n_images', '2', '--image_size', '26', '30', '-batch_size', '[2, 2, 2]', '--savepath', save,
                        '--width_div', '16', '--fc_channels', '32', '--max_batches', '1', '-penal_cst', '1e-4'],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    folder = os.path.join(save, 'camvid', 'fcn8_data_aug')               # the reference's exp_name, kept
    files = os.listdir(folder)
    models = [f for f in files if f in ('new_fcn8_model_best.npz', 'new_fcn8_model_last.npz')]
    assert models and 'fcn8_output.log' in files and 'config.txt' in files
    assert any(f.startswith('fcn8_errors_') for f in files)              # inside the folder, not next to it
    assert os.listdir(os.path.join(save, 'camvid')) == ['fcn8_data_aug']
    assert len(open(os.path.join(folder, 'fcn8_output.log')).read().splitlines()) == 2
    path = os.path.join(folder, models[0])
    net = buildFCN8(3, path_weights=path, n_classes=11)
    x = _dev(np.random.default_rng(1).random((2, 3, 26, 30)), torch.float32)
    probs = net(x)[0]
    assert tuple(probs.shape) == (2, 11, 26, 30) and bool(torch.isfinite(probs).all())
    # the trainer's deterministic forward on the same weights
    tnet = FCN8(load_param_list(path, PARAM_ORDER), 11, dtype=torch.float32, mma='f32', trainable=True)
    score = tnet.forward_train(x, deterministic=True)
    for conv in net.convs.values():
        conv.wino = conv.wino_f64 = False
    net._border = {}
    assert torch.equal(net(x)[0], ops.crop_softmax(score, 26, 30, off=(0, 0)))
    assert not torch.equal(tnet.flat, torch.zeros_like(tnet.flat))
