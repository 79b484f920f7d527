"""GPU: the context-module DAE off 11 classes.  Its kernels (csrc/conv_small.hip, ctx_train.hip, ctx_grad.hip) are
compiled per channel count padded to 4, 8, 12 and 16, and every other GPU test of the module runs 11 classes + 3 image
channels.  Here the whole module -- training backward, gradient mode, the inference paths with their bit identities,
the 16-bit leg, one trainer step -- runs at class counts that reach every padded width at both ends, conv1 from 3 to 16
input channels and both sides of the fused tail's 9-class threshold, against the float64 restatements
(tests/ctx_train_ref.py, ctx_grad_ref.py, ctx_c8_ref.py, oracle/contextmod.py), which are generic in the class count.
And at 14 classes + 3 image channels (17 into conv1, one past the gradient kernels' limit) inference still runs while
training and gradient mode refuse before a launch."""
import functools

import numpy as np
import pytest
import torch

import ctx_c8_ref as R8
import ctx_grad_ref as G
import ctx_train_ref as R
from oracle import contextmod as octx, refine as orefine
from iterative_inference_segm_amd import synthetic as S
from _parity_helpers import TOL as TOL_F32                   # 1e-4 on the refined map: test_config5_contextmod_50_steps
from test_gpu_ctx_c8 import SCORE_ERR_BOUND
from test_gpu_ctx_grad import TOL as TOL_GRAD
from test_gpu_ctx_train import F64_BOUND, _rel_err

pytestmark = pytest.mark.gpu
DT = {'f32': torch.float32, 'f64': torch.float64}

# (classes, h channels): padded widths 4 (2, 4), 8 (5, 8), 12 (9, 12), 16 (13); conv1 reads 3, 7, 8, 9, 12, 15, 16
# channels; the fused tail (ops.ctx_tail) takes 9 classes and more
CLASSES = [(2, 1), (4, 3), (5, 3), (8, 1), (9, 3), (12, 3), (13, 3)]
FUSED_FROM = 9
# one 64-column tile + a ragged one, one 16-row tile + a ragged one; the dilated layers run on 84 x 134
B, H, W = 2, 20, 70

# float32 training backward, teacher-forced (the restatement evaluated on the float32 forward's saved outputs: same
# masks, rounding only), max over the arrays of max|got - ref| / max|ref|.  F32_BOUND of test_gpu_ctx_train.py was
# measured at 11 classes.  Measured on an MI355X over CLASSES at 2 x 20 x 70 (the figures the test prints): 1.74e-07
# at 2 classes + 1, 1.03e-07 .. 1.25e-07 at 4, 5, 8, 9 and 12 classes, 8.09e-08 at 13; DESIGN.md section 9 holds the
# same figures.  Asserted with the same margin for the same reason: 4 x the maximum, another tile count means a
# different summation split.  (A figure above 1e-6 would not be one to record: it would be a bug.)
F32_CLASSES_MEASURED = 1.74e-07
F32_CLASSES_BOUND = 4 * F32_CLASSES_MEASURED


def _dev(a, dt):
    return torch.from_numpy(np.array(a)).to(dt).cuda().contiguous()      # (a copy: the cases are read-only)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(C, ch):
    """The inputs of test_gpu_ctx_train.py's `_net_case` at C classes and ch image channels, read-only, once."""
    rng = np.random.default_rng(11)
    params = S.make_contextmod_params(C, ch, seed=31)
    h = S.make_images(B, H, W, seed=11)[:, :ch].astype(np.float64)
    T = S.make_labels(B, H, W, n_classes=C, void_frac=0.1, seed=12).astype(np.float64)
    y = np.clip(T[:, :C] + 0.1 * rng.standard_normal((B, C, H, W)), 0, 1)
    for a in (h, T, y):
        a.setflags(write=False)
    return dict(params=params, p64=R.to64(params), h=h, T=T, y=y)


def _dae(C, ch, dt, **kw):
    from iterative_inference_segm_amd.contextmod import ContextModDAE
    return ContextModDAE(_case(C, ch)['params'], C, dtype=dt, **kw)


def _backward(C, ch, dt, losses, lmb):
    from iterative_inference_segm_amd import ops
    c = _case(C, ch)
    dae = _dae(C, ch, dt)
    score = dae.forward_train([_dev(c['h'], dt)], _dev(c['y'], dt))
    res, g, _ = ops.ctx_loss(score, _dev(c['T'], dt), losses, lmb)
    grads = dae.backward(g)
    torch.cuda.synchronize()
    return dae, res, g, {n: (a.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64))
                         for n, (a, b) in grads.items()}


# ---- 7. float64 training backward ----
@pytest.mark.parametrize('C,ch', CLASSES)
def test_training_backward_f64(built_lib, C, ch):
    c = _case(C, ch)
    # both losses on one class count, the reference's default on the others
    losses, lmb = (('crossentropy', 'squared_error'), 0.5) if C == 5 else (('crossentropy',), 1.0)
    cat, outs = R.forward(c['p64'], c['h'], c['y'])
    loss_ref, _, _, g_ref, _ = R.loss_and_grad(outs[-1], c['T'], losses, lmb)
    ref = R.backward(c['p64'], cat, outs, g_ref)
    dae, res, _, got = _backward(C, ch, torch.float64, losses, lmb)
    saved = [host(o) for o in dae.saved_outputs()]
    assert [s.shape for s in saved] == [o.shape for o in outs]
    # rounding only, as the gradients below: F64_BOUND of each layer's largest output
    fwd = max(float(np.abs(s - o).max() / np.abs(o).max()) for s, o in zip(saved, outs))
    err = _rel_err(got, ref)
    print('training backward f64, %d classes + %d: forward %.3g, gradients %.3g (loss %.6f / %.6f)'
          % (C, ch, fwd, err, float(res[0]), loss_ref))
    assert all(np.abs(b).max() > 0 for n in R.PARAM_ORDER for b in ref[n])       # no array's gradient vanishes
    assert fwd <= F64_BOUND
    assert abs(float(res[0]) - loss_ref) <= 1e-12 * loss_ref
    assert err <= F64_BOUND


# ---- 8. float32 training backward, teacher-forced ----
@pytest.mark.parametrize('C,ch', CLASSES)
def test_training_backward_f32_teacher_forced(built_lib, C, ch):
    c = _case(C, ch)
    dae, _, g, got = _backward(C, ch, torch.float32, ('crossentropy',), 1.0)
    outs = [host(o).astype(np.float64) for o in dae.saved_outputs()]
    cat = host(dae._saved['buf']['cat']).astype(np.float64)
    ref = R.backward(c['p64'], cat, outs, host(g).astype(np.float64))
    err = _rel_err(got, ref)
    print('training backward f32 teacher-forced, %d classes + %d: max relative error %.3g' % (C, ch, err))
    assert err <= F32_CLASSES_BOUND


# ---- 9. gradient mode ----
@pytest.mark.parametrize('prec', ['f32', 'f64'])
@pytest.mark.parametrize('C,ch', CLASSES)
def test_gradient_mode(built_lib, C, ch, prec):
    from iterative_inference_segm_amd import ops
    c, dt = _case(C, ch), DT[prec]
    g_ref, _ = G.ctx_sqerr_grad(c['p64'], c['h'], c['y'])
    hd, yd = _dev(c['h'], dt), _dev(c['y'], dt)
    dae = _dae(C, ch, dt)
    dae.keep_pre = True
    score = dae.scores([hd], yd)
    g_thr = dae.sqerr_backward(score, yd)
    assert tuple(g_thr.shape) == tuple(yd.shape)
    r = ops.crop_softmax(score, H, W, off=(0, 0))
    got = host(g_thr).astype(np.float64) - 2.0 * (host(r).astype(np.float64) - c['y'])
    scale = 1 + np.abs(g_ref).max()
    err = np.abs(got - g_ref).max()
    print('gradient mode %s, %d classes + %d: max|g - ref| = %.3g, max|ref| = %.3g' % (prec, C, ch, err, scale - 1))
    assert np.abs(g_ref).max() > 1e-2
    assert err <= TOL_GRAD[prec] * scale
    # any upstream gradient through backward_y: with the softmax backward it is the fused head's result
    g_by = dae.backward_y(ops.sqerr_softmax_bwd(score, yd, off=(0, 0)), yd.shape)
    if prec == 'f64':
        assert torch.equal(g_by, g_thr)
    else:
        assert np.abs(host(g_by) - host(g_thr)).max() <= TOL_GRAD[prec] * scale


# ---- 10. inference paths ----
@functools.lru_cache(maxsize=None)
def _oracle_loop(C, ch):
    """Six residual steps of step 0.5 in the oracle, per image; eps between the norms the images pass through, so
    that one of them stops on the way: 1 % above the smallest norm any image has at its third step."""
    c = _case(C, ch)
    fn = lambda hh, yy: octx.contextmod_forward(c['p64'], hh, yy)
    traces = []
    for im in range(B):
        traces.append([])
        orefine.refine_image(fn, [c['h'][im:im + 1]], c['y'][im:im + 1], 0.5, 6, eps=-1.0, trace=traces[-1])
    eps = 1.01 * min(t[2] for t in traces)
    yii, iters = orefine.refine_batch(fn, [c['h']], c['y'], 0.5, 6, eps=eps)
    # no norm within 1e-3 of eps: the stop decisions are the same in float32
    assert all(abs(v - eps) > 1e-3 * eps for t in traces for v in t)
    assert iters.min() <= 3 and iters.min() < 6
    return eps, yii, iters


@pytest.mark.parametrize('C,ch', CLASSES)
def test_inference_paths_are_bit_identical_and_match_the_oracle(built_lib, C, ch, monkeypatch):
    """test_contextmod_fused_tail_is_bit_identical (tests/test_gpu_configs.py) without an FCN-8: the fused tail on and
    off (below 9 classes `fused_step` returns None and the loop takes the unfused route by itself), the cached image
    half of conv1 on and off, eager and replayed -- the refined map bit for bit, the same iteration counts, the norms
    to rounding; float32 against the float64 module, the float64 module against the oracle."""
    from iterative_inference_segm_amd import contextmod as CM, ops
    from iterative_inference_segm_amd.api import IterativeInference
    c = _case(C, ch)
    eps, y_ref, it_ref = _oracle_loop(C, ch)

    def run(dt, fused, graph, hsplit):
        monkeypatch.setattr(ops, 'CTX_TAIL', fused)
        monkeypatch.setattr(CM, 'CTX_HSPLIT', hsplit)
        ii = IterativeInference(None, _dae(C, ch, dt), C, [C], dtype=dt)
        r = ii.refine([_dev(c['h'], dt)], _dev(c['y'], dt), 0.5, 6, eps=eps, graph=graph)
        return [host(t) for t in r]
    y0, it0, n0 = run(torch.float32, False, False, False)
    for fused, graph, hsplit in ((True, False, True), (True, True, True), (False, False, True), (True, True, False),
                                 (False, True, True)):
        y1, it1, n1 = run(torch.float32, fused, graph, hsplit)
        assert np.array_equal(y0, y1), (fused, graph, hsplit, np.abs(y0 - y1).max())
        assert list(it0) == list(it1), (fused, graph, hsplit)
        assert np.allclose(n0, n1, rtol=1e-9, atol=0), (fused, graph, hsplit)
    # the fused step itself: a count of norm partials (one per 16 x 64 tile) from 9 classes on, None below
    monkeypatch.setattr(ops, 'CTX_TAIL', True)
    monkeypatch.setattr(CM, 'CTX_HSPLIT', True)
    dae = _dae(C, ch, torch.float32)
    hd, yy = _dev(c['h'], torch.float32), _dev(c['y'], torch.float32)
    before = yy.clone()
    nblk = dae.fused_step([hd], yy, ops.RefineState(B, H, W, 'cuda'), 0.5, dae.new_session([hd], yy))
    if C >= FUSED_FROM:
        assert nblk == ((H + 15) // 16) * ((W + 63) // 64) and not torch.equal(yy, before)
    else:
        assert nblk is None and torch.equal(yy, before)
    # float32 against the float64 module, the float64 module against the oracle
    y64, it64, _ = run(torch.float64, True, False, True)
    e32, e64 = np.abs(y0 - y64).max(), np.abs(y64 - y_ref).max()
    print('inference, %d classes + %d: eps %.4g, iterations %s; fp32 vs float64 HIP %.3g, float64 HIP vs oracle %.3g'
          % (C, ch, eps, list(it_ref), e32, e64))
    assert list(it64) == list(it_ref) == list(it0)
    assert e64 <= 1e-9
    assert e32 <= TOL_F32


# ---- 11. the 16-bit leg ----
@pytest.mark.parametrize('C,ch', [(5, 3), (13, 3)])
def test_16bit_leg_against_the_restatement(built_lib, C, ch):
    """test_whole_module_against_the_restatement (tests/test_gpu_ctx_c8.py) at 5 and 13 classes, with that test's
    inputs (y0 a softmax of random logits, h in [0, 1]) and its bound."""
    rng = np.random.default_rng(21)
    p = _case(C, ch)['params']
    h = rng.random((B, ch, H, W)).astype(np.float32)
    z = rng.standard_normal((B, C, H, W)) * 2.0
    y = np.exp(z - z.max(1, keepdims=True))
    y = (y / y.sum(1, keepdims=True)).astype(np.float32)
    ref = R8.forward(R.to64(p), h.astype(np.float64), y.astype(np.float64))
    dae = _dae(C, ch, torch.float32, mma='bf16c8')
    assert dae.c8 is True
    score = host(dae.scores([_dev(h, torch.float32)], _dev(y, torch.float32))).astype(np.float64)
    err = float(np.abs(score - ref).max())
    print('C8 context module vs its restatement, %d classes + %d: max |score err| %.4e (score range %.3f); asserted '
          'bound %.4e' % (C, ch, err, float(np.abs(ref).max()), SCORE_ERR_BOUND))
    assert score.shape == ref.shape == (B, C, H, W)
    assert err <= SCORE_ERR_BOUND


# ---- 12. one trainer step ----
@pytest.mark.parametrize('C,ch', CLASSES)
def test_one_trainer_step_f64(built_lib, C, ch):
    """The first iteration of test_first_five_steps_match_the_restatement_f64 (y from the ground truth, noise 0.1
    from the caller's sample, rmsprop at 1e-4) with that test's bound on the loss -- and the parameters after the
    step against one R.rmsprop_step on the restatement's gradients."""
    from iterative_inference_segm_amd.train import DAETrainer
    c, dt = _case(C, ch), torch.float64
    y = c['T'][:, :C].copy()
    tr = DAETrainer(None, _dae(C, ch, dt), C, [C], noise=0.1, learning_rate=1e-4)
    gen = torch.Generator(device='cuda')
    gen.manual_seed(5)
    eps = torch.randn((B, C, H, W), generator=gen, device='cuda', dtype=dt)
    loss = float(tr.train_step(_dev(c['h'], dt), _dev(y, dt), _dev(c['T'], dt), eps=eps))
    loss_ref, grads = R.loss_and_param_grads(c['p64'], c['h'], y + 0.1 * host(eps), c['T'])
    flat0, gflat = R.flatten(c['p64']), R.flatten(grads)
    flat_ref, _ = R.rmsprop_step(flat0, gflat, np.zeros_like(flat0), 1e-4)
    got = host(tr.dae.flat)
    print('trainer step f64, %d classes + %d: loss %.12f restatement %.12f, max|p - ref| %.3g'
          % (C, ch, loss, loss_ref, np.abs(got - flat_ref).max()))
    assert abs(loss - loss_ref) <= F64_BOUND * abs(loss_ref)
    # p' = p - lr g / sqrt(0.1 g^2 + 1e-6): |dp'/dg| <= lr / sqrt(1e-6) = 0.1, and g is within F64_BOUND of its
    # array's largest entry; the step's own roundings (a few ulp of |p| <= 2) are the 1e-15
    assert got.shape == flat_ref.shape and np.abs(flat_ref - flat0).max() > 1e-5
    assert np.abs(got - flat_ref).max() <= 0.1 * F64_BOUND * np.abs(gflat).max() + 1e-15


# ---- 13. one channel past the gradient kernels ----
def test_17_input_channels_infer_and_refuse_the_backward_passes(built_lib):
    """14 classes + 3 image channels: conv1 reads 17 channels.  Inference runs (the layer is not on the <= 16-channel
    kernel then): float64 against the oracle, float32 against float64.  forward_train / backward, keep_pre /
    backward_y / sqerr_backward, gradient-mode refinement and a trainer step refuse up front -- conv1 is the last
    layer their backward passes would reach -- and launch nothing."""
    from iterative_inference_segm_amd import ops
    from iterative_inference_segm_amd.api import IterativeInference
    from iterative_inference_segm_amd.train import DAETrainer
    C, ch = 14, 3
    c = _case(C, ch)
    res = {}
    for prec, dt in DT.items():
        dae = _dae(C, ch, dt)
        assert dae.conv1.Cin == 17
        hd, yd = _dev(c['h'], dt), _dev(c['y'], dt)
        score = host(dae.scores([hd], yd)).astype(np.float64)
        ii = IterativeInference(None, dae, C, [C], dtype=dt)
        yii, iters, _ = ii.refine([hd], yd, 0.5, 4, early_stop=False)
        res[prec] = (score, host(yii).astype(np.float64), dae, ii, hd, yd)
        assert list(host(iters)) == [4] * B
    s_ref = octx.contextmod_forward(c['p64'], [c['h']], c['y'], out_softmax=False)
    y_ref, _ = orefine.refine_batch(lambda hh, yy: octx.contextmod_forward(c['p64'], hh, yy), [c['h']], c['y'], 0.5, 4,
                                    eps=-1.0)
    smax = 1 + np.abs(s_ref).max()
    print('14 classes + 3: score float64 HIP vs oracle %.3g, fp32 vs float64 HIP %.3g (max|score| %.3g); 4 steps: '
          '%.3g, %.3g' % (np.abs(res['f64'][0] - s_ref).max(), np.abs(res['f32'][0] - res['f64'][0]).max(), smax - 1,
                          np.abs(res['f64'][1] - y_ref).max(), np.abs(res['f32'][1] - res['f64'][1]).max()))
    assert np.abs(res['f64'][0] - s_ref).max() <= 1e-9 * smax and np.abs(res['f64'][1] - y_ref).max() <= 1e-9
    assert np.abs(res['f32'][0] - res['f64'][0]).max() <= TOL_F32 * smax
    assert np.abs(res['f32'][1] - res['f64'][1]).max() <= TOL_F32
    limit = r'classes \+ h channels <= 16 for training and gradient mode'
    for prec, dt in DT.items():
        _, _, dae, ii, hd, yd = res[prec]
        Td = _dev(c['T'], dt)
        tr = DAETrainer(None, dae, C, [C], noise=0.0, learning_rate=1e-4)
        flat = dae.flat.clone()
        torch.cuda.synchronize()
        ops.profile_begin()
        try:
            with pytest.raises(NotImplementedError, match=limit):
                dae.forward_train([hd], yd)
            with pytest.raises(NotImplementedError, match=limit):
                dae.backward(yd)
            with pytest.raises(NotImplementedError, match=limit):
                dae.keep_pre = True
            with pytest.raises(NotImplementedError, match=limit):
                dae.backward_y(yd, yd.shape)
            with pytest.raises(NotImplementedError, match=limit):
                dae.sqerr_backward(yd, yd)
            with pytest.raises(NotImplementedError, match=limit):
                ii.refine([hd], yd, 0.05, 2, mode='gradient')
            with pytest.raises(NotImplementedError, match=limit):
                tr.train_step(hd, yd, Td)
            with pytest.raises(NotImplementedError, match=limit):
                tr.val_step(hd, yd, Td)
        finally:
            n = ops.profile_end()
        assert n == 0                                        # not one launch of the library
        assert dae.keep_pre is False and torch.equal(dae.flat, flat)
