"""GPU: true-gradient refinement through the context-module DAE (csrc/ctx_grad.hip, ContextModDAE.backward_y /
sqerr_backward, api._refine(mode='gradient')) against the float64 restatement tests/ctx_grad_ref.py, which
tests/test_ctx_grad_ref.py pins by finite differences."""
import functools
import os

import numpy as np
import pytest
import torch

import ctx_grad_ref as G
import ctx_train_ref as R
from iterative_inference_segm_amd import synthetic as S

pytestmark = pytest.mark.gpu
DT = {'f32': torch.float32, 'f64': torch.float64}
TOL = {'f32': 2e-4, 'f64': 1e-10}          # x (1 + max|g|): the bounds of test_gpu_e2e.py::test_true_gradient_mode


def _dev(a, dt):
    return torch.from_numpy(np.array(a)).to(dt).cuda().contiguous()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ---- 1. masked data gradient, exact on small-integer data ----
# (B, Cin, ci = (first, count) or None, Cout, OH, OW of the gradient map, K, dil, layout, window or None)
Y_HALF = (3, 11)                            # conv1: the y channels 3..13 of [image, y]
DG_CASES = [
    (1, 11, None, 11, 37, 150, 3, 1, 'iohw', None),       # odd width, crosses a 64-column tile
    (3, 11, None, 11, 37, 150, 3, 2, 'iohw', None),
    (1, 11, None, 11, 84, 82, 3, 4, 'iohw', None),        # crosses 16-row tiles
    (3, 11, None, 11, 84, 82, 3, 8, 'oihw', None),
    (1, 11, None, 11, 37, 150, 3, 16, 'oihw', None),
    (3, 11, None, 11, 20, 18, 3, 16, 'iohw', None),       # the map is smaller than the tap span
    (1, 14, Y_HALF, 11, 20, 18, 3, 16, 'oihw', None),
    (3, 14, Y_HALF, 11, 37, 150, 3, 1, 'oihw', (1, 1, 37, 150)),      # conv1: the interior of its pad
    (1, 14, Y_HALF, 11, 84, 82, 3, 2, 'iohw', None),
    (3, 11, None, 11, 84, 82, 1, 1, 'iohw', None),        # dilconv7
    (1, 11, None, 11, 37, 150, 1, 1, 'oihw', None),
    (1, 14, Y_HALF, 11, 84, 82, 1, 1, 'oihw', None),
    (1, 11, None, 11, 37, 150, 3, 16, 'iohw', (32, 32, 37, 118)),     # PadLayer(32)'s adjoint: a window
    (3, 11, None, 11, 84, 82, 3, 1, 'iohw', (32, 32, 50, 40)),
    (1, 16, (2, 13), 16, 37, 150, 3, 4, 'iohw', (5, 3, 30, 131)),     # 16 channels either side, 13 of them asked
    # off 11 classes: conv_small_dgrad_kernel<T, K, CIP> is compiled for CIP = the channels asked padded to 4, 8, 12,
    # 16; the cases above reach CIP 12 and 16, and Cout 11 and 16, only
    (1, 1, None, 1, 2, 3, 3, 1, 'iohw', None),            # K 3, CIP 4: one channel either side
    (3, 3, None, 2, 17, 65, 3, 2, 'oihw', None),          # K 3, CIP 4, Cout 2: crosses a tile edge both ways
    (1, 7, (3, 4), 4, 16, 62, 3, 4, 'oihw', None),        # K 3, CIP 4 exactly: conv1 of 4 classes
    (2, 8, (3, 5), 5, 20, 18, 3, 1, 'oihw', (1, 1, 20, 18)),          # K 3, CIP 8, windowed: conv1 of 5 classes
    (1, 8, None, 8, 9, 63, 1, 1, 'iohw', None),           # K 1, CIP 8 exactly
    (1, 16, (3, 13), 13, 33, 70, 3, 1, 'oihw', (1, 1, 33, 70)),       # K 3, CIP 16: conv1 of 13 classes
    (1, 16, (15, 1), 16, 12, 10, 3, 16, 'iohw', (3, 5, 7, 4)),        # K 3, CIP 4: only the last input channel, a
    #                                                                   window one thread wide
    (2, 2, None, 3, 5, 7, 1, 1, 'iohw', None),            # K 1, CIP 4, and
    (1, 16, None, 13, 5, 66, 1, 1, 'oihw', None),         # K 1, CIP 16: the two instantiations left (K 1, CIP 12: above)
]
# the 2 x 3 map has six mask values: the seed's offset at which they hold a zero, a negative and a positive one
DG_SEED_OFFSET = {(2, 3): 2}


@pytest.mark.parametrize('prec', ['f32', 'f64'])
@pytest.mark.parametrize('B,Cin,ci,Cout,OH,OW,K,d,layout,window', DG_CASES)
def test_masked_data_gradient_is_exact_on_integers(built_lib, prec, B, Cin, ci, Cout, OH, OW, K, d, layout, window):
    from iterative_inference_segm_amd import ops
    dt = DT[prec]
    rng = np.random.default_rng(OH * 7 + d + K + Cin + B + DG_SEED_OFFSET.get((OH, OW), 0))
    gout = rng.integers(-2, 3, size=(B, Cout, OH, OW)).astype(np.float64)
    out = rng.integers(-2, 3, size=(B, Cout, OH, OW)).astype(np.float64)        # zeros and negatives: masked
    assert (out == 0).any() and (out < 0).any() and (out > 0).any()
    W_iohw = rng.integers(-2, 3, size=(Cin, Cout, K, K)).astype(np.float64)
    Wp = W_iohw if layout == 'iohw' else np.ascontiguousarray(np.transpose(W_iohw, (1, 0, 2, 3)))
    ref = R._bwd_data(np.where(out > 0, gout, 0.0), W_iohw, d)
    ref_lin = R._bwd_data(gout, W_iohw, d)
    assert ref.shape == (B, Cin, OH + d * (K - 1), OW + d * (K - 1)) and np.abs(ref_lin).max() < 2 ** 24
    c0, nc = ci if ci is not None else (0, Cin)
    y0, x0, wh, ww = window if window is not None else (0, 0) + ref.shape[2:]
    want = ref[:, c0:c0 + nc, y0:y0 + wh, x0:x0 + ww]
    # `out` inside larger planes (conv1's map lives inside PadLayer(32)'s buffer), the destination inside a
    # sentinel that must stay as it is
    outp = rng.integers(-2, 3, size=(B, Cout, OH + 7, OW + 5)).astype(np.float64)
    outp[:, :, 4:4 + OH, 3:3 + OW] = out
    gx = torch.full((B, nc + 2, wh + 5, ww + 3), -9.0, dtype=dt, device='cuda')
    ret = ops.conv_small_dgrad(_dev(gout, dt), _dev(outp, dt), _dev(Wp, dt), dil=d, layout=layout, out_off=(4, 3),
                               window=window, ci=ci, gx=gx, gx_off=(1, 2, 1))
    assert ret is gx
    gxh = host(gx).astype(np.float64)
    assert np.array_equal(gxh[:, 1:1 + nc, 2:2 + wh, 1:1 + ww], want)
    gxh[:, 1:1 + nc, 2:2 + wh, 1:1 + ww] = -9.0
    assert np.all(gxh == -9.0)                               # nothing else was written
    # dense destination, `out` as its own tensor; and a linear layer (out = None)
    got = ops.conv_small_dgrad(_dev(gout, dt), _dev(out, dt), _dev(Wp, dt), dil=d, layout=layout, window=window, ci=ci)
    assert tuple(got.shape) == want.shape and np.array_equal(host(got), want)
    lin = ops.conv_small_dgrad(_dev(gout, dt), None, _dev(Wp, dt), dil=d, layout=layout, window=window, ci=ci)
    assert np.array_equal(host(lin), ref_lin[:, c0:c0 + nc, y0:y0 + wh, x0:x0 + ww])


# ---- 2. head ----
HEAD_CASES = [  # (C of the score map, Cin of dilconv7 = channels of out6, H, W): a block is 256 pixels of one image
    (11, 11, 37, 50),      # 1850 pixels: 8 blocks, the last one ragged
    (2, 16, 1, 1),         # one pixel; C at the lower end, Cin at the upper: the two parameter strides differ
    (5, 9, 5, 51),         # 255 pixels
    (16, 3, 16, 16),       # 256 pixels; C at the upper end, Cin < C
    (13, 13, 1, 257),      # 257 pixels
]


@pytest.mark.parametrize('prec', ['f32', 'f64'])
@pytest.mark.parametrize('Cc,Cin,H,W', HEAD_CASES)
def test_head_matches_softmax_backward_bits_and_the_restatement(built_lib, prec, Cc, Cin, H, W):
    from iterative_inference_segm_amd import ops
    dt = DT[prec]
    rng = np.random.default_rng(17)
    B = 3
    score = rng.standard_normal((B, Cc, H, W)) * 3
    y = rng.random((B, Cc, H, W))
    y /= y.sum(1, keepdims=True)
    out6 = np.maximum(rng.standard_normal((B, Cin, H, W)), 0.0)          # about half exact zeros
    W7 = rng.standard_normal((Cin, Cc, 1, 1))                            # 'iohw': W[in, out, 1, 1]
    sd, yd, od, Wd = (_dev(a, dt) for a in (score, y, out6, W7))
    g6, gs = ops.ctx_grad_head(sd, yd, od, Wd, layout='iohw', want_gs=True)
    assert torch.equal(gs, ops.sqerr_softmax_bwd(sd, yd, off=(0, 0)))
    assert torch.equal(g6, ops.ctx_grad_head(sd, yd, od, Wd, layout='iohw'))             # without the g_s store
    # the restatement on the inputs as the device holds them
    to = lambda t: host(t).astype(np.float64)
    g6_ref, gs_ref = G.head(to(sd), to(yd), to(od), to(Wd))
    err = np.abs(to(g6) - g6_ref).max() / np.abs(g6_ref).max()
    print('head %s %s: max|g6 - ref| / max|ref| = %.3g' % (prec, (Cc, Cin, H, W), err))
    assert tuple(g6.shape) == (B, Cin, H, W) and (to(g6)[to(od) <= 0] == 0).all() and np.abs(g6_ref).max() > 0
    if out6.size >= 1000:                                    # (statistics of the inputs: not of 3 x 16 values)
        assert 0.4 < (out6 == 0).mean() < 0.6 and np.abs(g6_ref).max() > 1e-2
    # float64: the issue's bound.  float32: exp and C-term FMA chains in fp32 (C <= 16), each term below max|g_s|
    # max|W|: 1e-5 of the largest entry is an order above 16 x 2^-24 x that.
    assert err <= (1e-13 if prec == 'f64' else 1e-5)
    # the other parameter layout, and no mask
    Wt = _dev(np.ascontiguousarray(np.transpose(W7, (1, 0, 2, 3))), dt)
    assert torch.equal(ops.ctx_grad_head(sd, yd, od, Wt, layout='oihw'), g6)
    un = ops.ctx_grad_head(sd, yd, None, Wd, layout='iohw')
    assert torch.equal(torch.where(od > 0, un, torch.zeros_like(un)), g6)
    # ... which is the 1x1 adjoint of the masked data gradient kernel, bit for bit
    assert torch.equal(ops.conv_small_dgrad(gs, None, Wd, dil=1, layout='iohw'), un)


# ---- 3 - 5: the whole network ----
PARAM_SEED = 31


@functools.lru_cache(maxsize=None)
def _case():
    """2 x 11 x 40 x 36, h = a 3-channel image; the restatement's gradient and two-step loop, computed once."""
    B, H, W = 2, 40, 36
    rng = np.random.default_rng(11)
    params = S.make_contextmod_params(11, 3, seed=PARAM_SEED)
    h = S.make_images(B, H, W, seed=11).astype(np.float64)
    T = S.make_labels(B, H, W, n_classes=11, void_frac=0.1, seed=12)
    y = np.clip(T[:, :11] + 0.1 * rng.standard_normal((B, 11, H, W)), 0, 1).astype(np.float64)
    p64 = R.to64(params)
    g, r = G.ctx_sqerr_grad(p64, h, y)
    yy, last = G.refine_gradient(p64, h, y, 0.05, 2)
    for a in (h, y, g, r, yy, last):
        a.setflags(write=False)
    return dict(params=params, p64=p64, h=h, y=y, g=g, r=r, yy=yy, last=last,
                e0=G.sqerr(p64, h, y), e2=G.sqerr(p64, h, yy))


def _dae(dt, params=None):
    from iterative_inference_segm_amd.contextmod import ContextModDAE
    return ContextModDAE(params if params is not None else _case()['params'], 11, dtype=dt)


@pytest.mark.parametrize('prec', ['f32', 'f64'])
def test_whole_gradient_against_the_restatement(built_lib, prec):
    from iterative_inference_segm_amd import ops
    c, dt = _case(), DT[prec]
    hd, yd = _dev(c['h'], dt), _dev(c['y'], dt)
    dae = _dae(dt)
    dae.keep_pre = True
    score = dae.scores([hd], yd)
    g_thr = dae.sqerr_backward(score, yd)
    assert tuple(g_thr.shape) == tuple(yd.shape)
    r = ops.crop_softmax(score, 40, 36, off=(0, 0))
    got = host(g_thr).astype(np.float64) - 2.0 * (host(r).astype(np.float64) - c['y'])
    scale = 1 + np.abs(c['g']).max()
    err = np.abs(got - c['g']).max()
    print('whole gradient %s: max|g - ref| = %.3g, max|ref| = %.3g' % (prec, err, scale - 1))
    assert np.abs(c['g']).max() > 1e-2
    assert err <= TOL[prec] * scale
    # through a session (the cached image half, conv1's map inside PadLayer(32)'s buffer): identical bits
    sess = dae.new_session([hd], yd)
    score_s = dae.scores([hd], yd, session=sess)
    assert torch.equal(score_s, score)
    assert torch.equal(dae.sqerr_backward(score_s, yd), g_thr)
    # any upstream gradient through backward_y; with the softmax backward it is the fused head's result
    g_by = dae.backward_y(ops.sqerr_softmax_bwd(score_s, yd, off=(0, 0)), yd.shape)
    if prec == 'f64':
        assert torch.equal(g_by, g_thr)
    else:
        assert np.abs(host(g_by) - host(g_thr)).max() <= TOL[prec] * scale
    # without keep_pre nothing is kept, and the backward says so
    dae.keep_pre = False
    dae.scores([hd], yd)
    with pytest.raises(RuntimeError, match='keep_pre'):
        dae.backward_y(g_by, yd.shape)


@pytest.mark.parametrize('prec', ['f32', 'f64'])
def test_gradient_mode_loop(built_lib, prec):
    from iterative_inference_segm_amd.api import IterativeInference
    c, dt = _case(), DT[prec]
    hd, yd = _dev(c['h'], dt), _dev(c['y'], dt)
    ii = IterativeInference(None, _dae(dt), 11, [11], dtype=dt)
    Yii, iters, norms = ii.refine([hd], yd, 0.05, 2, mode='gradient')
    scale = 1 + np.abs(c['g']).max()
    assert list(host(iters)) == [2, 2]
    dy, dn = np.abs(host(Yii) - c['yy']).max(), np.abs(host(norms) - c['last']).max()
    print('gradient loop %s: max|Y - ref| = %.3g, max|norm - ref| = %.3g' % (prec, dy, dn))
    assert dy <= TOL[prec] * scale and dn <= TOL[prec] * scale
    assert torch.equal(yd, _dev(c['y'], dt))                 # the caller's y is not changed
    # the descent direction lowers the reconstruction error
    assert c['e2'] < c['e0']
    assert G.sqerr(c['p64'], c['h'], host(Yii).astype(np.float64)) < c['e0']


def test_gradient_mode_leaves_no_state_behind(built_lib):
    """A residual refinement after a gradient-mode call on the same DAE equals a fresh DAE's, eager and replayed
    from the captured graph."""
    from iterative_inference_segm_amd.api import IterativeInference
    c, dt = _case(), torch.float32
    hd, yd = _dev(c['h'], dt), _dev(c['y'], dt)
    used, fresh = _dae(dt), _dae(dt)
    ii_u, ii_f = IterativeInference(None, used, 11, [11]), IterativeInference(None, fresh, 11, [11])
    ii_u.refine([hd], yd, 0.05, 2, mode='gradient')
    assert used.keep_pre is True
    for graph, n in ((False, 4), (True, 12)):
        a = ii_u.refine([hd], yd, 0.1, n, graph=graph, early_stop=False)
        b = ii_f.refine([hd], yd, 0.1, n, graph=graph, early_stop=False)
        assert all(torch.equal(x, z) for x, z in zip(a, b)), graph
        assert used.keep_pre is False and used._pre is None   # residual mode keeps no layer outputs
        ii_u.refine([hd], yd, 0.05, 2, mode='gradient')      # ... and again in between: the graph still holds
    a = ii_u.refine([hd], yd, 0.1, 12, graph=True, early_stop=False)
    assert all(torch.equal(x, z) for x, z in zip(a, b))


def test_gradient_mode_after_a_training_step_sees_the_new_weights(built_lib, tmp_path):
    from iterative_inference_segm_amd.api import IterativeInference
    from iterative_inference_segm_amd.contextmod import PARAM_ORDER, buildDAE_contextmod
    from iterative_inference_segm_amd.train import DAETrainer
    from iterative_inference_segm_amd.weights import save_param_list
    c, dt = _case(), torch.float32
    hd, yd = _dev(c['h'], dt), _dev(c['y'], dt)
    Td = _dev(S.make_labels(2, 40, 36, n_classes=11, void_frac=0.1, seed=12), dt)
    tr = DAETrainer(None, _dae(dt), 11, [11], noise=0.1, seed=3, learning_rate=1e-2)
    ii = IterativeInference(None, tr.dae, 11, [11])
    before = ii.refine([hd], yd, 0.05, 2, mode='gradient')[0].clone()     # the backward's operands exist, stale
    tr.train_step(hd, yd, Td)
    after = ii.refine([hd], yd, 0.05, 2, mode='gradient')
    save_param_list(str(tmp_path / 'dae_model_best.npz'), tr.dae.state_arrays(), PARAM_ORDER)
    fresh = buildDAE_contextmod(path_weights=str(tmp_path), model_name='dae_model_best.npz', load_weights=True)
    assert torch.equal(fresh.flat, tr.dae.flat)
    ref = IterativeInference(None, fresh, 11, [11]).refine([hd], yd, 0.05, 2, mode='gradient')
    assert all(torch.equal(x, z) for x, z in zip(after, ref))
    assert not torch.equal(after[0], before)


# ---- 6. driver ----
def test_driver_runs_gradient_mode_with_the_context_module(built_lib, tmp_path):
    import iterative_inference as drv
    dd = {'kind': 'contextmod', 'concat_h': ['input'], 'from_gt': False}
    out = drv.inference('camvid', 'fcn8', 0.05, 2, dae_dict_updates=dd, savepath=str(tmp_path / 's'),
                        loadpath=str(tmp_path / 'l'), weights_path=str(tmp_path / 'w'), synthetic=True, n_images=2,
                        image_size=(64, 48), batch_size=2, verbose=False, update='gradient', early_stop=False,
                        in_flight=1)
    assert out['ii']['batches'] == 1 and np.isfinite(out['ii']['loss'])
    files = sorted((tmp_path / 's').rglob('batch0.npz'))
    assert len(files) == 1 and (files[0].parent / 'config.txt').exists()
    with np.load(str(files[0])) as f:
        assert sorted(f.files) == ['L', 'X', 'Y_fcn', 'Y_ii'] and f['Y_ii'].shape == (2, 11, 64, 48)
        assert np.isfinite(f['Y_ii']).all() and not np.array_equal(f['Y_ii'], f['Y_fcn'])     # two steps were taken


def test_refine_refuses_the_fcn8_dae_and_launches_nothing(built_lib):
    from iterative_inference_segm_amd import ops
    from iterative_inference_segm_amd.api import IterativeInference
    from iterative_inference_segm_amd.fcn8 import FCN8DAE
    dp = S.make_fcn8_dae_params(11, ['input'], (3,), seed=555, width_div=16, fc_channels=32)
    dae = FCN8DAE(dp, 11, concat_h=['input'])
    ii = IterativeInference(None, dae, 11, [11])
    h = torch.rand((1, 3, 32, 32), device='cuda')
    y = torch.rand((1, 11, 32, 32), device='cuda')
    torch.cuda.synchronize()
    ops.profile_begin()
    try:
        with pytest.raises(NotImplementedError, match='fcn8'):
            ii.refine([h], y, 0.05, 2, mode='gradient')
    finally:
        n = ops.profile_end()
    assert n == 0                                            # not one launch of the library
