"""GPU: training the context-module DAE (csrc/ctx_train.hip, contextmod.py, train.py, train_dae.py) against
the float64 restatement tests/ctx_train_ref.py, which tests/test_ctx_train_ref.py pins by finite differences."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ctx_train_ref as R
from iterative_inference_segm_amd import synthetic as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {'f32': torch.float32, 'f64': torch.float64}


def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda().contiguous()


# ---- 1. weight gradient, exact on integer data ----
WG_CASES = [  # (B, Cin, Cout, H, W of the OUTPUT, K, dil, layout)
    (1, 14, 11, 37, 150, 3, 1, 'oihw'), (3, 11, 11, 37, 150, 3, 2, 'iohw'), (1, 11, 11, 84, 82, 3, 4, 'iohw'),
    (3, 14, 11, 84, 82, 3, 8, 'oihw'), (1, 11, 11, 37, 150, 3, 16, 'iohw'), (3, 11, 11, 84, 82, 1, 1, 'iohw'),
    (1, 14, 11, 37, 150, 1, 1, 'oihw'), (1, 11, 11, 288, 288, 3, 1, 'iohw'), (1, 14, 11, 288, 288, 3, 16, 'oihw'),
    (3, 11, 11, 84, 82, 3, 16, 'oihw'), (1, 11, 11, 288, 288, 1, 1, 'oihw'), (1, 14, 16, 37, 150, 3, 2, 'iohw'),
    # off 11 classes: conv_small_wgrad_kernel<T, K, CP> is compiled for CP = Cout padded to 4, 8, 12, 16; the cases
    # above reach CP 12 and 16 only.  (Tile: 64 columns x 16 rows in fp32, x 8 rows in float64.)
    (1, 1, 1, 1, 1, 3, 1, 'oihw'),       # K 3, CP 4: one pixel, one channel either side, three of the four waves idle
    (3, 3, 2, 17, 65, 3, 2, 'iohw'),     # K 3, CP 4: Cin < 4 waves; a row and a column past the fp32 tile; 12 fp32 slabs
    #                                      (18 in float64): fewer than / just past the finalize kernel's 16 segments
    (1, 7, 4, 16, 64, 3, 4, 'oihw'),     # K 3, CP 4 exactly: one fp32 tile, two float64 tiles; conv1 of 4 classes
    (3, 8, 5, 9, 63, 1, 1, 'iohw'),      # K 1, CP 8
    (1, 9, 8, 8, 128, 3, 16, 'oihw'),    # K 3, CP 8 exactly
    (2, 15, 12, 24, 130, 3, 8, 'iohw'),  # K 3, CP 12 exactly
    (1, 16, 13, 33, 70, 3, 1, 'oihw'),   # K 3, CP 16 with three padding planes, Cin at its maximum: conv1 of 13 classes
    (1, 16, 16, 5, 3, 1, 1, 'iohw'),     # K 1, CP 16: both sides at the maximum on a tiny map
    (2, 2, 3, 5, 7, 1, 1, 'oihw'),       # K 1, CP 4 (dilconv7 of a 3-class module): the one instantiation left
    #                                      (K 1, CP 12: the 11 -> 11 cases above)
]


@pytest.mark.parametrize('prec', ['f32', 'f64'])
@pytest.mark.parametrize('B,Cin,Cout,OH,OW,K,d,layout', WG_CASES)
def test_weight_gradient_is_exact_on_integers(built_lib, prec, B, Cin, Cout, OH, OW, K, d, layout):
    from iterative_inference_segm_amd import ops
    dt = DT[prec]
    rng = np.random.default_rng(OH * 7 + d + K + Cin)
    H, W = OH + d * (K - 1), OW + d * (K - 1)
    x = rng.integers(-2, 3, size=(B, Cin, H, W))
    gout = rng.integers(-2, 3, size=(B, Cout, OH, OW))
    act = rng.integers(0, 2, size=(B, Cout, OH, OW))
    gz_ref = gout * act
    dW_ref = np.zeros((Cin, Cout, K, K), dtype=np.int64)
    for ky in range(K):
        for kx in range(K):
            xs = x[:, :, ky * d:ky * d + OH, kx * d:kx * d + OW]
            dW_ref[:, :, ky, kx] = np.tensordot(xs, gz_ref, axes=([0, 2, 3], [0, 2, 3]))
    if layout == 'oihw':
        dW_ref = np.transpose(dW_ref, (1, 0, 2, 3))
    db_ref = gz_ref.sum(axis=(0, 2, 3))
    assert np.abs(dW_ref).max() < 2 ** 24
    dW = torch.full(dW_ref.shape, 7.0, dtype=dt, device='cuda')
    db = torch.full((Cout,), 7.0, dtype=dt, device='cuda')
    # g_z inside a border that must stay as it is
    gz = torch.full((B, Cout, OH + 5, OW + 3), -9.0, dtype=dt, device='cuda')
    ops.conv_small_wgrad(_dev(x, dt), _dev(gout, dt), _dev(act, dt), dW, db, dil=d, layout=layout, gz=gz,
                         gz_off=(2, 1))
    torch.cuda.synchronize()
    assert np.array_equal(dW.cpu().numpy(), dW_ref.astype(np.float64))
    assert np.array_equal(db.cpu().numpy(), db_ref.astype(np.float64))
    gzh = gz.cpu().numpy()
    assert np.array_equal(gzh[:, :, 2:2 + OH, 1:1 + OW], gz_ref.astype(np.float64))
    gzh[:, :, 2:2 + OH, 1:1 + OW] = -9.0
    assert np.all(gzh == -9.0)
    # a linear layer (no mask), g_z not stored
    dW2, db2 = torch.empty_like(dW), torch.empty_like(db)
    ops.conv_small_wgrad(_dev(x, dt), _dev(gz_ref, dt), None, dW2, db2, dil=d, layout=layout)
    assert torch.equal(dW2, dW) and torch.equal(db2, db)


# ---- 2. loss kernel ----
LOSS_SHAPES = [  # (B, C, H, W): a block is 256 pixels of one image
    (3, 11, 37, 50),       # 8 blocks per image, the last one ragged
    (1, 2, 1, 1),          # one pixel, C at the lower end of its range
    (2, 5, 5, 51),         # 255 pixels: one short of a block
    (1, 16, 16, 16),       # 256 pixels: one block exactly, C at the upper end
    (3, 13, 1, 257),       # one pixel past a block
    (9, 4, 90, 90),        # 9 x 32 = 288 partials: the strided loop of `columns2` takes a second trip
]


def _loss_case(B, Cc, H, W, void):
    # (the one-pixel map from a seed of its own: seed 3 puts its two logits 13.8 apart, r = [1 - 1e-6, 1e-6], and the
    # whole gradient map -- r0 r1 (gr0 - gr1) -- is 2e-6, below the float32 rounding 2^-24 |gr| of the `gr - dot`
    # it is the difference of: a bound relative to max|g| says nothing on a map whose ONLY pixel is saturated)
    rng = np.random.default_rng(3 if H * W > 1 else 4)
    score = rng.standard_normal((B, Cc, H, W)) * 3
    if void:                                                 # (the one-pixel map cannot hold both kinds of pixel)
        T = np.zeros((B, Cc + 1, H, W))
        T[:, Cc] = 1
    else:
        # (label and void blobs of 16 x 16 pixels; 4 x 4 on the maps that are no larger than one such blob)
        T = S.make_labels(B, H, W, n_classes=Cc, void_frac=0.0 if H * W == 1 else 0.2, seed=5,
                          block=16 if min(H, W) > 16 else 4).astype(np.float64)
        assert 0 < T[:, Cc].sum() < B * H * W or H * W == 1  # void and labelled pixels
    if B > 1:
        T[1] = 0
        T[1, Cc] = 1                                         # an all-void image in the batch
    if H >= 4:
        score[0, :, :4] = -60.0                              # probabilities driven into the clip, both ends
        score[0, min(3, Cc - 1), :4] = 60.0
    return score, T


@pytest.mark.parametrize('losses,lmb', [(('crossentropy',), 1.0), (('squared_error',), 1.0),
                                        (('crossentropy', 'squared_error'), 0.5)])
@pytest.mark.parametrize('B,Cc,H,W,void', [s + (False,) for s in LOSS_SHAPES] + [(1, 2, 1, 1, True)])
def test_loss_kernel_f64(built_lib, losses, lmb, B, Cc, H, W, void):
    from iterative_inference_segm_amd import ops
    score, T = _loss_case(B, Cc, H, W, void)
    loss, ce, se, g, (n_ce, n_se) = R.loss_and_grad(score, T, losses, lmb)
    sd, Td = _dev(score, torch.float64), _dev(T, torch.float64)
    res, gd, cnt = ops.ctx_loss(sd, Td, losses, lmb)
    # the validation pass's call (no gradient stored): the same loss and counts, bit for bit
    res_v, g_v, cnt_v = ops.ctx_loss(sd, Td, losses, lmb, grad=False)
    torch.cuda.synchronize()
    assert g_v is None and torch.equal(res_v, res) and torch.equal(cnt_v, cnt)
    res, cnt, gd = res.cpu().numpy(), cnt.cpu().numpy(), gd.cpu().numpy()
    assert cnt[0] == n_ce and cnt[1] == n_se
    if void:
        assert n_ce == 0 and n_se == 0 and loss == 0.0 and not g.any()
        assert float(res[0]) == 0.0 and not gd.any() and cnt[2] == 0.0 and cnt[3] == 0.0
    else:
        # (the bounds below are relative to max|g|: some pixel's softmax is not saturated, so that its gradient
        # entry, before the division by the pixel count, is of the order of the terms it is the difference of)
        assert n_ce > 0 and n_se > 0 and np.abs(g).max() * n_ce > 1e-2
        print('loss kernel f64 %s: |dloss| %.3g  max|dg| / max|g| %.3g' %
              ((B, Cc, H, W), abs(res[0] - loss), np.abs(gd - g).max() / np.abs(g).max()))
        # sums of at most ~73000 terms in double: 1e-12 relative is two orders above the rounding
        assert abs(res[0] - loss) <= 1e-12 * abs(loss) and abs(res[1] - ce) <= 1e-12 * ce and abs(res[2] - se) <= 1e-12 * se
        assert np.abs(gd - g).max() <= 1e-12 * np.abs(g).max()
    if B > 1:
        assert not gd[1].any()                               # the all-void image
    # a batch without a single non-void pixel: zero loss and gradient, no NaN (documented in iiseg.h)
    Tv = np.zeros_like(T)
    Tv[:, Cc] = 1
    res, gd, cnt = ops.ctx_loss(sd, _dev(Tv, torch.float64), losses, lmb)
    assert float(res[0]) == 0.0 and not bool(gd.any()) and float(cnt[2]) == 0.0
    # float32 runs and agrees to float32 accuracy
    s32, T32 = _dev(score, torch.float32), _dev(T, torch.float32)
    res32, g32, cnt32 = ops.ctx_loss(s32, T32, losses, lmb)
    res32_v, _, cnt32_v = ops.ctx_loss(s32, T32, losses, lmb, grad=False)
    assert torch.equal(res32_v, res32) and torch.equal(cnt32_v, cnt32)
    assert abs(float(res32[0]) - loss) <= 1e-5 * abs(loss)
    assert np.abs(g32.cpu().numpy() - g).max() <= 1e-5 * np.abs(g).max()


# ---- 3 / 4. whole backward ----
def _net_case(B, H, W, seed=11):
    rng = np.random.default_rng(seed)
    params = S.make_contextmod_params(11, 3, seed=31)
    h = S.make_images(B, H, W, seed=seed)
    T = S.make_labels(B, H, W, n_classes=11, void_frac=0.1, seed=seed + 1)
    y = np.clip(T[:, :11] + 0.1 * rng.standard_normal((B, 11, H, W)), 0, 1)
    return params, h.astype(np.float64), y.astype(np.float64), T.astype(np.float64)


def _gpu_backward(params, h, y, T, dt, losses=('crossentropy',)):
    from iterative_inference_segm_amd import ops
    from iterative_inference_segm_amd.contextmod import ContextModDAE
    dae = ContextModDAE(params, 11, dtype=dt)
    score = dae.forward_train([_dev(h, dt)], _dev(y, dt))
    res, g, _ = ops.ctx_loss(score, _dev(T, dt), losses, 1.0)
    grads = dae.backward(g)
    torch.cuda.synchronize()
    return dae, res, g, {n: (a.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64))
                         for n, (a, b) in grads.items()}


def test_forward_train_takes_the_list_of_h_and_still_the_bare_tensor(built_lib):
    from iterative_inference_segm_amd.contextmod import ContextModDAE
    params, h, y, _ = _net_case(1, 40, 36)                  # one image: a bare (1, 3, H, W) tensor has len 1 too
    dt = torch.float32
    dae = ContextModDAE(params, 11, dtype=dt)
    hd, yd = _dev(h, dt), _dev(y, dt)
    as_list = dae.forward_train([hd], yd).clone()
    assert torch.equal(dae.forward_train(hd, yd), as_list) and bool(as_list.any())
    with pytest.raises(ValueError, match='expected 1 h tensor'):
        dae.forward_train([hd, hd], yd)


def _rel_err(got, ref):
    """max over the arrays of max|got - ref| / max|ref|"""
    worst = 0.0
    for n in R.PARAM_ORDER:
        for a, b in zip(got[n], ref[n]):
            assert a.shape == b.shape, n
            worst = max(worst, float(np.abs(a - b).max() / np.abs(b).max()))
    return worst


BACKWARD_CASES = [(2, 40, 36), (1, 224, 224)]
# Measured on an MI355X (the figures these tests print), maximum over BACKWARD_CASES of max|got - ref| / max|ref|
# per array:  float64 3.24e-15 (2 x 40 x 36; 1.04e-15 at 224^2),  float32 teacher-forced 8.16e-08 (2 x 40 x 36;
# 4.83e-08 at 224^2).  DESIGN.md section 9 holds the same figures.
# float64: rounding only; first power of ten above 4 x 3.24e-15 = 1.3e-14 (anything above 1e-9 would be a bug)
F64_BOUND = 1e-13
# float32, teacher-forced (the restatement on the float32 forward's saved outputs: same masks, rounding only):
# 4 x the measured maximum; the margin covers a different summation split on another tile count
F32_BOUND = 4 * 8.16e-08


@pytest.mark.parametrize('B,H,W', BACKWARD_CASES)
def test_whole_backward_f64(built_lib, B, H, W):
    params, h, y, T = _net_case(B, H, W)
    loss_ref, ref = R.loss_and_param_grads(R.to64(params), h, y, T)
    _, res, _, got = _gpu_backward(params, h, y, T, torch.float64)
    err = _rel_err(got, ref)
    print('whole backward f64 %dx%dx%d: max relative error %.3g (loss %.6f / %.6f)'
          % (B, H, W, err, float(res[0]), loss_ref))
    assert abs(float(res[0]) - loss_ref) <= 1e-12 * loss_ref
    assert err <= F64_BOUND


@pytest.mark.parametrize('B,H,W', BACKWARD_CASES)
def test_whole_backward_f32_teacher_forced(built_lib, B, H, W):
    params, h, y, T = _net_case(B, H, W)
    p64 = R.to64(params)
    dae, res, g, got = _gpu_backward(params, h, y, T, torch.float32)
    # the restatement ON the float32 forward's saved layer outputs and its g_score: same masks, rounding only
    outs = [o.cpu().numpy().astype(np.float64) for o in dae.saved_outputs()]
    cat = dae._saved['buf']['cat'].cpu().numpy().astype(np.float64)
    ref = R.backward(p64, cat, outs, g.cpu().numpy().astype(np.float64))
    err = _rel_err(got, ref)
    # free-running float32 against free-running float64: reported, not asserted
    cat64, outs64 = R.forward(p64, h, y)
    _, free = R.loss_and_param_grads(p64, h, y, T)
    flips = [float(((a > 0) != (b > 0)).mean()) for a, b in zip(outs[:7], outs64[:7])]
    cos = [float(R.flatten({m: got[m] if m == n else (np.zeros(0), np.zeros(0)) for m in R.PARAM_ORDER}) @
                 R.flatten({m: free[m] if m == n else (np.zeros(0), np.zeros(0)) for m in R.PARAM_ORDER}) /
                 (np.linalg.norm(np.concatenate([a.ravel() for a in got[n]])) *
                  np.linalg.norm(np.concatenate([a.ravel() for a in free[n]])))) for n in R.PARAM_ORDER]
    print('whole backward f32 %dx%dx%d: teacher-forced max relative error %.3g; free-running: differing ReLU '
          'decisions per layer %s, gradient cosine per layer %s'
          % (B, H, W, err, ['%.2g' % f for f in flips], ['%.6f' % c for c in cos]))
    assert err <= F32_BOUND


# ---- 5. optimizer ----
@pytest.mark.parametrize('kind', ['rmsprop', 'adam'])
@pytest.mark.parametrize('prec', ['f32', 'f64'])
def test_optimizer_steps(built_lib, kind, prec):
    from iterative_inference_segm_amd import ops
    dt, npdt = DT[prec], {'f32': np.float32, 'f64': np.float64}[prec]
    rng = np.random.default_rng(9)
    p = R.flatten(S.make_contextmod_params(11, 3, seed=31)).astype(npdt)        # the real parameter buffer
    assert p.size == 8129
    pd, s1d = _dev(p, dt), torch.zeros(p.size, dtype=dt, device='cuda')
    s2d = torch.zeros_like(s1d) if kind == 'adam' else None
    std = torch.tensor([0.0, 1.0, 1.0], dtype=dt, device='cuda') if kind == 'adam' else None
    lr = torch.full((1,), 1e-3, dtype=dt, device='cuda')
    lr_host = npdt(lr.cpu().numpy()[0])
    a, m, v, st = np.zeros_like(p), np.zeros_like(p), np.zeros_like(p), (0, npdt(1), npdt(1))
    for step in range(3):
        g = (rng.standard_normal(p.size) * 10.0 ** rng.integers(-6, 1, size=p.size)).astype(npdt)
        g[rng.integers(0, p.size, size=50)] = 0
        ops.opt_step(kind, pd, _dev(g, dt), s1d, s2d, lr, std)
        if kind == 'rmsprop':
            p, a = R.rmsprop_step(p, g, a, lr_host, npdt)
        else:
            p, m, v, st = R.adam_step(p, g, m, v, st, lr_host, npdt)
        got = pd.cpu().numpy()
        ulp = np.abs(got.astype(np.float64) - p.astype(np.float64)) / np.spacing(np.abs(p)).astype(np.float64)
        print('%s %s step %d: max distance %.2f ulp, %d of %d parameters differ'
              % (kind, prec, step, ulp.max(), int((got != p).sum()), p.size))
        if prec == 'f32':
            # no FMA contraction in the kernel (clang fp contract(off)), correctly rounded sqrt and division:
            # EQUAL to numpy's float32 arithmetic
            assert np.array_equal(got, p)
        else:
            assert ulp.max() <= 4
        lr.mul_(0.5)                                          # annealed on the device between steps
        lr_host = npdt(lr.cpu().numpy()[0])
    if kind == 'adam':
        assert std.cpu().numpy().tolist() == [3.0, float(st[1]), float(st[2])]


# opt_step_kernel: ONE workgroup of 1024 threads strides over the buffer; opt_step_grid_kernel: blocks of 256 threads,
# at most 2048 of them, grid-stride beyond 2048 x 256 = 524288 scalars
OPT_SIZES = [(False, n) for n in (1, 2, 1023, 1024, 1025)] + \
            [(True, n) for n in (1, 255, 256, 257, 524288, 524289)]
OPT_BORDER, OPT_SENTINEL = 67, -77.0


@pytest.mark.parametrize('kind', ['rmsprop', 'adam'])
@pytest.mark.parametrize('prec', ['f32', 'f64'])
@pytest.mark.parametrize('grid,n', OPT_SIZES)
def test_optimizer_step_at_the_block_edges(built_lib, kind, prec, grid, n):
    """Both forms against numpy (R.rmsprop_step / R.adam_step) below, at and just past their block sizes, two steps;
    p, s1 and s2 live inside sentinel buffers whose borders must stay as they are."""
    from iterative_inference_segm_amd import ops
    dt, npdt = DT[prec], {'f32': np.float32, 'f64': np.float64}[prec]
    rng = np.random.default_rng(9 + n)
    lo, hi = OPT_BORDER, OPT_BORDER + n

    def bordered(inner=None):
        t = torch.full((n + 2 * OPT_BORDER,), OPT_SENTINEL, dtype=dt, device='cuda')
        if inner is None:
            t[lo:hi].zero_()
        else:
            t[lo:hi].copy_(_dev(inner, dt))
        return t
    p = rng.standard_normal(n).astype(npdt)
    bufs = {'p': bordered(p), 's1': bordered()}
    if kind == 'adam':
        bufs['s2'] = bordered()
    pd, s1d = bufs['p'][lo:hi], bufs['s1'][lo:hi]
    s2d = bufs['s2'][lo:hi] if kind == 'adam' else None
    std = torch.tensor([0.0, 1.0, 1.0], dtype=dt, device='cuda') if kind == 'adam' else None
    lr = torch.full((1,), 1e-3, dtype=dt, device='cuda')
    lr_host = npdt(lr.cpu().numpy()[0])
    a, m, v, st = np.zeros_like(p), np.zeros_like(p), np.zeros_like(p), (0, npdt(1), npdt(1))

    def same(got, ref, what, step):
        got = got.cpu().numpy()
        ulp = np.abs(got.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref)).astype(np.float64)
        if prec == 'f32':                                     # the criteria of test_optimizer_steps
            assert np.array_equal(got, ref), (what, step, float(ulp.max()))
        else:
            assert ulp.max() <= 4, (what, step, float(ulp.max()))
    for step in range(2):
        g = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 1, size=n)).astype(npdt)
        if n > 2:
            g[rng.integers(0, n, size=max(1, n // 100))] = 0
        ops.opt_step(kind, pd, _dev(g, dt), s1d, s2d, lr, std, grid=grid)
        if kind == 'rmsprop':
            p, a = R.rmsprop_step(p, g, a, lr_host, npdt)
            same(s1d, a, 'a', step)
        else:
            p, m, v, st = R.adam_step(p, g, m, v, st, lr_host, npdt)
            same(s1d, m, 'm', step)
            same(s2d, v, 'v', step)
        same(pd, p, 'p', step)
        lr.mul_(0.5)
        lr_host = npdt(lr.cpu().numpy()[0])
    for name, t in bufs.items():
        th = t.cpu().numpy()
        assert np.all(th[:lo] == OPT_SENTINEL) and np.all(th[hi:] == OPT_SENTINEL), name
    if kind == 'adam':
        # the powers as running products, each rounded in the step's own type
        assert std.cpu().numpy().tolist() == [2.0, float(npdt(0.9) * npdt(0.9)), float(npdt(0.999) * npdt(0.999))]
        assert (float(st[1]), float(st[2])) == (float(npdt(0.9) * npdt(0.9)), float(npdt(0.999) * npdt(0.999)))


# ---- 6. determinism and refresh ----
def _trainer(params, dt, noise=0.0, seed=1, **kw):
    from iterative_inference_segm_amd.contextmod import ContextModDAE
    from iterative_inference_segm_amd.train import DAETrainer
    dae = ContextModDAE(params, 11, dtype=dt)
    return DAETrainer(None, dae, 11, [11], noise=noise, seed=seed, **kw)


def test_train_step_is_deterministic_and_every_path_sees_the_new_weights(built_lib, tmp_path):
    from iterative_inference_segm_amd import ops
    from iterative_inference_segm_amd.api import IterativeInference
    from iterative_inference_segm_amd.contextmod import PARAM_ORDER, buildDAE_contextmod
    from iterative_inference_segm_amd.weights import save_param_list
    params, h, y, T = _net_case(2, 40, 36)
    dt = torch.float32
    hd, yd, Td = _dev(h, dt), _dev(y, dt), _dev(T, dt)
    flats = []
    for _ in range(2):
        tr = _trainer(params, dt, noise=0.1, seed=3, learning_rate=1e-2)
        # inference paths exercised BEFORE the step, so their packed weights and split halves exist and are stale
        ii = IterativeInference(None, tr.dae, 11, [11])
        ii.refine([hd], yd.clone(), 0.1, 5, graph=True)
        tr.dae(hd, yd)
        held = tr.dae.new_session([hd], yd)                     # a session obtained BEFORE the step ...
        tr.train_step(hd, yd, Td)
        held_score = tr.dae.scores([hd], yd, session=held).clone()      # ... and used after it
        torch.cuda.synchronize()
        flats.append(tr.dae.flat.clone())
    assert torch.equal(flats[0], flats[1])
    assert not torch.equal(flats[0], _dev(R.flatten(params), dt))
    save_param_list(str(tmp_path / 'dae_model_best.npz'), tr.dae.state_arrays(), PARAM_ORDER)
    fresh = buildDAE_contextmod(path_weights=str(tmp_path), model_name='dae_model_best.npz', load_weights=True)
    assert torch.equal(fresh.flat, tr.dae.flat)
    assert torch.equal(tr.dae(hd, yd), fresh(hd, yd))                                  # eager
    assert torch.equal(held_score, fresh.scores([hd], yd, session=fresh.new_session([hd], yd)))
    outs = []
    for dae in (tr.dae, fresh):
        sess = dae.new_session([hd], yd)
        eager_session = dae.scores([hd], yd, session=sess).clone()                     # session step
        yy = yd.clone()
        state = ops.RefineState(2, 40, 36, 'cuda')
        sess = dae.new_session([hd], yy)
        nblk = dae.fused_step([hd], yy, state, 0.1, sess)                              # fused tail
        assert nblk is not None
        outs.append((eager_session, yy))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # a refinement loop long enough to replay its captured step
    res = []
    for dae, engine in ((tr.dae, ii), (fresh, IterativeInference(None, fresh, 11, [11]))):
        Y, iters, _ = engine.refine([hd], yd.clone(), 0.1, 12, graph=True)
        res.append((Y.clone(), iters.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_backward_after_a_training_step_runs_on_the_new_adjoint_filters(built_lib):
    """The data-gradient layers are built by the first `backward` and rewritten by `refresh()` from the same
    filters: after one train_step, the backward of a second step equals that of a module rebuilt from
    `state_arrays()`, bit for bit (the `sqerr_backward` half: tests/test_gpu_ctx_grad.py,
    test_gradient_mode_after_a_training_step_sees_the_new_weights)."""
    from iterative_inference_segm_amd import ops
    from iterative_inference_segm_amd.contextmod import ContextModDAE
    params, h, y, T = _net_case(2, 40, 36)
    dt = torch.float32
    hd, yd, Td = _dev(h, dt), _dev(y, dt), _dev(T, dt)
    tr = _trainer(params, dt, noise=0.1, seed=3, learning_rate=1e-2)
    tr.train_step(hd, yd, Td)
    assert tr.dae._adj is not None                           # built by that step, stale until refresh()
    fresh = ContextModDAE(tr.dae.state_arrays(), 11, dtype=dt)
    assert torch.equal(fresh.flat, tr.dae.flat)
    assert not torch.equal(fresh.flat, _dev(R.flatten(params), dt))
    grads = []
    for dae in (tr.dae, fresh):
        score = dae.forward_train([hd], yd)
        _, g, _ = ops.ctx_loss(score, Td, ('crossentropy',), 1.0)
        gv = dae.backward(g)
        assert gv['conv1'][0].data_ptr() == dae.gflat.data_ptr()
        grads.append(dae.gflat.clone())
    assert torch.equal(grads[0], grads[1]) and bool(grads[0].any())


# ---- 7. training works ----
def test_first_five_steps_match_the_restatement_f64(built_lib):
    params, h, y, T = _net_case(2, 40, 36, seed=21)
    y = T[:, :11].copy()                                     # from_gt
    dt = torch.float64
    tr = _trainer(params, dt, noise=0.1, learning_rate=1e-4)
    hd, yd, Td = _dev(h, dt), _dev(y, dt), _dev(T, dt)
    gen = torch.Generator(device='cuda')
    gen.manual_seed(5)
    p = R.to64(params)
    flat, a = R.flatten(p), np.zeros(8129)
    for step in range(5):
        eps = torch.randn(yd.shape, generator=gen, device='cuda', dtype=dt)           # the same noise to both
        loss = float(tr.train_step(hd, yd, Td, eps=eps))
        yn = y + 0.1 * eps.cpu().numpy()
        loss_ref, grads = R.loss_and_param_grads(R.unflatten(flat, p), h, yn, T)
        flat, a = R.rmsprop_step(flat, R.flatten(grads), a, 1e-4)
        print('step %d: loss %.12f restatement %.12f' % (step, loss, loss_ref))
        assert abs(loss - loss_ref) <= F64_BOUND * (step + 1) * abs(loss_ref)      # item 3's bound x steps


def test_loss_goes_down_over_60_steps_f32(built_lib):
    from iterative_inference_segm_amd.data_loader import SyntheticSegmentationIterator
    params = S.make_contextmod_params(11, 3, seed=777)
    tr = _trainer(params, torch.float32, noise=0.1, seed=2, learning_rate=1e-4)
    it = SyntheticSegmentationIterator(n_images=20, image_size=(224, 224), batch_size=10)
    batches = []
    for _ in range(2):
        X, L = it.next()
        Ld = _dev(L, torch.float32)
        batches.append((_dev(X, torch.float32), Ld[:, :11].contiguous(), Ld))
    losses = []
    for step in range(60):
        losses.append(tr.train_step(*batches[step % 2]))
    losses = [float(v) for v in torch.stack(losses).cpu()]
    print('loss, steps 0-9: %.5f, steps 50-59: %.5f' % (np.mean(losses[:10]), np.mean(losses[-10:])))
    assert np.all(np.isfinite(losses))
    assert np.mean(losses[-10:]) < np.mean(losses[:10])


# ---- 8. the driver end to end ----
def test_driver_end_to_end(built_lib, tmp_path):
    from iterative_inference_segm_amd.api import IterativeInference
    from iterative_inference_segm_amd.contextmod import buildDAE_contextmod
    save, load = str(tmp_path / 'save'), str(tmp_path / 'load')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_dae.py'), '--synthetic', '--num_epochs', '2',
                        '--n_images', '20', '--image_size', '40', '36', '--savepath', save, '--loadpath', load,
                        '-segmentation_net', 'fcn8', '-dae_dict', '{"from_gt": true, "noise": 0.1}'],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    exp, = os.listdir(os.path.join(save, 'camvid'))
    assert exp.startswith('flip_final_fcn8_contextmod_input_crossentropy_fromgt_z0.1_data_aug_rmsprop_lr0.0001')
    folder = os.path.join(save, 'camvid', exp)
    for name in ('dae_model_best.npz', 'dae_model_last.npz', 'dae_errors_last.npz', 'output.log', 'config.txt'):
        assert os.path.exists(os.path.join(folder, name)), name
        assert os.path.exists(os.path.join(load, 'camvid', exp, name)), name
    lines = open(os.path.join(folder, 'output.log')).read().splitlines()
    assert len(lines) == 2 and lines[0].startswith('EPOCH 0: Avg epoch training cost train ')
    with np.load(os.path.join(folder, 'dae_errors_last.npz')) as f:
        assert all(len(f['arr_%d' % i]) == 2 and np.all(np.isfinite(f['arr_%d' % i])) for i in range(4))
    dae = buildDAE_contextmod(path_weights=folder, model_name='dae_model_best.npz', load_weights=True)
    ii = IterativeInference(None, dae, 11, [11])
    X = _dev(S.make_images(2, 40, 36, seed=3), torch.float32)
    Y0 = _dev(S.make_labels(2, 40, 36, seed=4)[:, :11], torch.float32)
    Y, iters, _ = ii.refine([X], Y0.clone(), 0.1, 5)
    assert bool(torch.isfinite(Y).all()) and Y.shape == Y0.shape


def test_driver_default_configuration_from_the_segmentation_net(built_lib, tmp_path):
    """The reference's defaults: -segmentation_net densenet, from_gt false (y = the net's prediction)."""
    save = str(tmp_path / 'save')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_dae.py'), '--synthetic', '--num_epochs', '1',
                        '--n_images', '4', '--image_size', '64', '64', '--savepath', save,
                        '--loadpath', str(tmp_path / 'load'), '--weights_path', str(tmp_path / 'w')],
                       capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    exp, = os.listdir(os.path.join(save, 'camvid'))
    assert exp.startswith('flip_final_densenet_contextmod_input_crossentropy_fromfcn8_z0_data_aug_T1.0_rmsprop')
    folder = os.path.join(save, 'camvid', exp)
    line, = open(os.path.join(folder, 'output.log')).read().splitlines()
    vals = [float(v) for v in line.replace(',', ' ').split() if v.replace('.', '', 1).replace('-', '', 1).isdigit()]
    assert line.startswith('EPOCH 0:') and all(np.isfinite(vals))
    for name in ('dae_model_best.npz', 'dae_model_last.npz'):
        assert os.path.exists(os.path.join(folder, name)), name
