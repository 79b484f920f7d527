"""GPU: the 16-bit mode of the 'valid' K x K layers (kxk='bf16'; csrc/conv_kxk_bf16.hip).
The two kernels: exact on data bf16 holds exactly (channel tails, every K edge, channel slices in both layouts, a
window of larger planes, accumulate, gate); on real data within the any-order fp32 accumulation bound of the float64
sum over operands rounded on the CPU with .to(torch.bfloat16), ties and direction included; the same bits twice with
several slabs.  The module: between kxk='f32' and 'bf16' the forward, the saved maps and every gradient no rounded
operand reaches keep their bits, every call of the two ops meets its bound on its own operands, no fp32 flipped copy
of fc6 / fc7 is built, and the chain's cosine to the fp32 gradients is that of the float64 restatement with the same
rounding points (tests/kxk_bf16_ref.py).  Training and the driver run in the mode.

Measured on an MI355X (for the record; the assertions are the derived bounds): see DESIGN.md section 17."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fcn8_train_ref as RF
import kxk_bf16_ref as KR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = torch.float32
U = 2.0 ** -24


def _dev(a, dt=F32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda().contiguous()


# ---- 1., 2. exact on small integers ----
CHANNELS = [(11, 64), (24, 16), (64, 130), (130, 33)]            # no multiples of the 64 blocks or the 16 k-tile
# (K, h, w) of the input window; the output is (h - K + 1, w - K + 1)
SHAPES = [(7, 7, 7), (7, 8, 9), (7, 13, 13), (1, 1, 1), (1, 7, 7), (1, 37, 150), (3, 5, 4), (2, 4, 4)]
_REF = {}


def _int_case(Cin, Cout, B, K, h, w):
    key = (Cin, Cout, B, K, h, w)
    if key not in _REF:
        rng = np.random.default_rng(Cin * 1000 + Cout + 7 * B + 31 * K + h)
        OH, OW = h - K + 1, w - K + 1
        x = rng.integers(-2, 3, size=(B, Cin, h, w))
        Wt = rng.integers(-2, 3, size=(Cout, Cin, K, K))
        gz = rng.integers(-2, 3, size=(B, Cout, OH, OW))
        gz[rng.integers(0, 2, size=gz.shape) == 0] = 0           # as behind a ReLU mask
        old = rng.integers(-2, 3, size=(B, Cin, h, w))           # what `accumulate` adds to
        gate = rng.integers(-1, 2, size=(B, Cin, h, w))          # zeros and negatives close the gate
        dW = KR.wgrad_kxk(x.astype(np.int64), gz.astype(np.int64))
        gx = KR.dgrad_kxk(gz.astype(np.int64), Wt.astype(np.int64))
        db = gz.astype(np.int64).sum(axis=(0, 2, 3))
        assert dW.dtype == gx.dtype == np.int64
        assert max(np.abs(dW).max(), np.abs(gx).max() + 2, np.abs(db).max()) < 2 ** 24
        _REF[key] = (x, Wt, gz, old, gate, dW, db, gx)
    return _REF[key]


SENTINEL = 777.0


@pytest.mark.parametrize('K,h,w', SHAPES)
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('Cin,Cout', CHANNELS)
def test_bf16_weight_gradient_is_exact_on_integers(built_lib, Cin, Cout, B, K, h, w):
    from iterative_inference_segm_amd import ops
    x, _, gz, _, _, ref, dbref, _ = _int_case(Cin, Cout, B, K, h, w)
    xd, gzd = _dev(x), _dev(gz)
    # the layer's own array (every entry is written: no NaN survives)
    dW = torch.full((Cout, Cin, K, K), float('nan'), dtype=F32, device='cuda')
    db = torch.full((Cout,), float('nan'), dtype=F32, device='cuda')
    ops.conv_wgrad_kxk(xd, gzd, dW, db, mma='bf16')
    # the middle channels of a wider parameter, in both layouts, with a sentinel around them
    lo, hi = 3, 5
    big = torch.full((Cout, lo + Cin + hi, K, K), SENTINEL, dtype=F32, device='cuda')
    ops.conv_wgrad_kxk(xd, gzd, big, None, ci0=lo, mma='bf16')
    bigT = torch.full((lo + Cin + hi, Cout, K, K), SENTINEL, dtype=F32, device='cuda')
    ops.conv_wgrad_kxk(xd, gzd, bigT, None, ci0=lo, layout='iohw', mma='bf16')
    # through a window of larger planes, read in place (the way score_pool4 calls the fp32 op)
    planes = torch.full((B, Cin, h + 3, w + 5), float('nan'), dtype=F32, device='cuda')
    planes[:, :, 1:1 + h, 2:2 + w] = xd
    dWw = torch.full((Cout, Cin, K, K), float('nan'), dtype=F32, device='cuda')
    dbw = torch.full((Cout,), float('nan'), dtype=F32, device='cuda')
    ops.conv_wgrad_kxk(planes, gzd, dWw, dbw, window=(1, 2, h, w), mma='bf16')
    torch.cuda.synchronize()
    want = ref.astype(np.float64)
    assert np.array_equal(dW.cpu().numpy(), want)
    assert np.array_equal(db.cpu().numpy(), dbref.astype(np.float64))
    assert np.array_equal(dWw.cpu().numpy(), want)
    assert np.array_equal(dbw.cpu().numpy(), dbref.astype(np.float64))
    b = big.cpu().numpy()
    assert np.array_equal(b[:, lo:lo + Cin], want)
    assert (b[:, :lo] == SENTINEL).all() and (b[:, lo + Cin:] == SENTINEL).all()
    bT = bigT.cpu().numpy()
    assert np.array_equal(bT[lo:lo + Cin], want.transpose(1, 0, 2, 3))
    assert (bT[:lo] == SENTINEL).all() and (bT[lo + Cin:] == SENTINEL).all()


@pytest.mark.parametrize('K,h,w', SHAPES)
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('Cin,Cout', CHANNELS)
def test_bf16_data_gradient_is_exact_on_integers(built_lib, Cin, Cout, B, K, h, w):
    from iterative_inference_segm_amd import ops
    _, Wt, gz, old, gate, _, _, ref = _int_case(Cin, Cout, B, K, h, w)
    Wd, gzd = _dev(Wt), _dev(gz)
    got = ops.conv_dgrad_kxk(gzd, Wd)                            # the layer's own parameter, W[out, in, K, K]
    # the middle channels of a wider parameter, in both layouts: the other input channels hold NaN
    lo, hi = 3, 5
    big = torch.full((Cout, lo + Cin + hi, K, K), float('nan'), dtype=F32, device='cuda')
    big[:, lo:lo + Cin] = Wd
    mid = ops.conv_dgrad_kxk(gzd, big, ci0=lo, cin=Cin)
    bigT = big.transpose(0, 1).contiguous()
    midT = ops.conv_dgrad_kxk(gzd, bigT, ci0=lo, cin=Cin, layout='iohw')
    # into `out` (every entry is written), onto an integer map in place, behind a gate, both
    out = torch.full((B, Cin, h, w), float('nan'), dtype=F32, device='cuda')
    assert ops.conv_dgrad_kxk(gzd, Wd, out=out) is out
    acc = _dev(old)
    assert ops.conv_dgrad_kxk(gzd, Wd, out=acc, accumulate=True) is acc
    gated = ops.conv_dgrad_kxk(gzd, Wd, gate=_dev(gate))
    both = _dev(old)
    ops.conv_dgrad_kxk(gzd, Wd, out=both, accumulate=True, gate=_dev(gate))
    torch.cuda.synchronize()
    want = ref.astype(np.float64)
    assert tuple(got.shape) == (B, Cin, h, w)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(mid.cpu().numpy(), want)
    assert np.array_equal(midT.cpu().numpy(), want)
    assert np.array_equal(acc.cpu().numpy(), want + old)
    assert np.array_equal(gated.cpu().numpy(), np.where(gate > 0, want, 0.0))
    assert np.array_equal(both.cpu().numpy(), np.where(gate > 0, want + old, 0.0))


# ---- 3. the rounding point and the bound ----
def _rounded(t):
    """float64 numpy of a float32 tensor rounded to bf16 on the CPU"""
    return t.detach().cpu().to(torch.bfloat16).double().numpy()


def _f64(t):
    return t.detach().cpu().double().numpy()


def _wgrad_bound_check(dW, db, x, gz, what=''):
    """dW (Cout, Cin, K, K) against the float64 sum over x and gz (float32 tensors, x already cut to the window)
    rounded to bf16 on the CPU: every entry within (n + 1) 2^-24 sum|a b|, n = B OH OW -- the bound of n fp32
    additions of exact products in ANY order.  db against the float64 sum of the UNROUNDED gz, within (n + 1) 2^-24
    sum|gz|.  Returns (worst error / bound, mag)."""
    n = gz.shape[0] * gz.shape[2] * gz.shape[3]
    xr, gr = _rounded(x), _rounded(gz)
    ref, mag = KR.wgrad_kxk(xr, gr), KR.wgrad_kxk(np.abs(xr), np.abs(gr))
    err, bound = np.abs(_f64(dW) - ref), (n + 1) * U * mag
    frac = float((err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all(), '%s: dW worst error / bound %.3g over %d terms' % (what, frac, n)
    if db is not None:
        g = _f64(gz)
        errb, boundb = np.abs(_f64(db) - g.sum(axis=(0, 2, 3))), (n + 1) * U * np.abs(g).sum(axis=(0, 2, 3))
        assert (errb <= boundb).all(), '%s: db' % what
        frac = max(frac, float((errb / np.maximum(boundb, 1e-300)).max()))
    return frac, mag


def _dgrad_bound_check(gx, gz, W, old=None, gate=None, what=''):
    """gx against the float64 sum over W (Cout, Cin, K, K) and gz rounded to bf16 on the CPU: every entry within
    (n + 1) 2^-24 sum|a b|, n = K^2 Cout (+ 1 under accumulate, |old| in the magnitude).  gate: closed entries are
    exactly zero.  Returns (worst error / bound, mag)."""
    n = W.shape[2] * W.shape[3] * gz.shape[1]
    g, w = _rounded(gz), _rounded(W)
    ref, mag = KR.dgrad_kxk(g, w), KR.dgrad_kxk(np.abs(g), np.abs(w))
    if old is not None:
        o = _f64(old)
        ref, mag, n = ref + o, mag + np.abs(o), n + 1
    got = _f64(gx)
    if gate is not None:
        closed = ~(gate.detach().cpu().numpy() > 0)
        assert (got[closed] == 0).all(), what
        ref, mag = np.where(closed, 0.0, ref), np.where(closed, 0.0, mag)
    err, bound = np.abs(got - ref), (n + 1) * U * mag
    frac = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    assert (err <= bound).all(), '%s: worst error / bound %.3g over %d terms' % (what, frac, n)
    return frac, mag


# (K, Cin, Cout, h, w, B, seed)
RANDOM = {7: (7, 24, 16, 13, 13, 2, 5), 1: (1, 24, 16, 7, 7, 2, 5)}


@pytest.mark.parametrize('K', [7, 1])
def test_operands_are_rounded_to_nearest_once(built_lib, K):
    from iterative_inference_segm_amd import ops
    K, Cin, Cout, h, w, B, seed = RANDOM[K]
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.standard_normal((B, Cin, h, w)).astype(np.float32))
    gz = torch.from_numpy(rng.standard_normal((B, Cout, h - K + 1, w - K + 1)).astype(np.float32))
    W = torch.from_numpy((0.1 * rng.standard_normal((Cout, Cin, K, K))).astype(np.float32))
    # CPU only, before the GPU is looked at: the statement discriminates -- the float64 sums over the UNROUNDED
    # operands leave the bound around the sums over the rounded ones on more than half of the entries
    nw, nd = B * gz.shape[2] * gz.shape[3], K * K * Cout
    magw = KR.wgrad_kxk(np.abs(_rounded(x)), np.abs(_rounded(gz)))
    magd = KR.dgrad_kxk(np.abs(_rounded(gz)), np.abs(_rounded(W)))
    outw = np.abs(KR.wgrad_kxk(_f64(x), _f64(gz)) - KR.wgrad_kxk(_rounded(x), _rounded(gz))) > (nw + 1) * U * magw
    outd = np.abs(KR.dgrad_kxk(_f64(gz), _f64(W)) - KR.dgrad_kxk(_rounded(gz), _rounded(W))) > (nd + 1) * U * magd
    print('K = %d: the unrounded sums lie outside the bound on %.3f (dW) and %.3f (gx) of the entries'
          % (K, outw.mean(), outd.mean()))
    assert outw.mean() > 0.5 and outd.mean() > 0.5
    dW, db = torch.empty((Cout, Cin, K, K), dtype=F32, device='cuda'), torch.empty(Cout, dtype=F32, device='cuda')
    ops.conv_wgrad_kxk(x.cuda(), gz.cuda(), dW, db, mma='bf16')
    gx = ops.conv_dgrad_kxk(gz.cuda(), W.cuda())
    old = torch.from_numpy(rng.standard_normal((B, Cin, h, w)).astype(np.float32))
    acc = old.cuda()
    ops.conv_dgrad_kxk(gz.cuda(), W.cuda(), out=acc, accumulate=True)
    torch.cuda.synchronize()
    fw = _wgrad_bound_check(dW, db, x, gz, 'K = %d' % K)[0]
    fd = _dgrad_bound_check(gx, gz, W, what='K = %d' % K)[0]
    fa = _dgrad_bound_check(acc, gz, W, old=old, what='K = %d accumulate' % K)[0]
    print('K = %d, %d -> %d at %dx%d: worst error / bound dW %.3g, gx %.3g, gx accumulated %.3g' % (K, Cin, Cout, h, w, fw, fd, fa))


def test_ties_go_to_even_and_negative_values_round_symmetrically(built_lib):
    from iterative_inference_segm_amd import ops
    vals = [1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -10, -(1 + 2.0 ** -8 + 2.0 ** -10),
            1 + 2.0 ** -7 - 2.0 ** -10]
    want = [1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, -(1 + 2.0 ** -7), 1 + 2.0 ** -7]
    v32 = torch.tensor(vals, dtype=F32)
    assert v32.double().tolist() == vals                         # float32 holds them
    assert v32.to(torch.bfloat16).double().tolist() == want      # torch's rounding on the CPU
    for K in (7, 1):
        one = torch.ones((1, 1, 1, 1), dtype=F32, device='cuda')
        # data gradient, W: W[0, c] holds value c at every tap, g_z is a single 1.0: gx[0, c, y, x] = bf16(value c)
        W = v32.view(1, 5, 1, 1).expand(1, 5, K, K).contiguous().cuda()
        got = ops.conv_dgrad_kxk(one, W).cpu().double().numpy()
        for c in range(5):
            assert (got[0, c] == want[c]).all(), (K, c, got[0, c], want[c])
        # data gradient, g_z: channel c holds value c, W[co, ci] is 1.0 at every tap of co == ci
        gz = v32.view(1, 5, 1, 1).contiguous().cuda()
        W = torch.eye(5, dtype=F32).view(5, 5, 1, 1).expand(5, 5, K, K).contiguous().cuda()
        got = ops.conv_dgrad_kxk(gz, W).cpu().double().numpy()
        for c in range(5):
            assert (got[0, c] == want[c]).all(), (K, c, got[0, c], want[c])
        # weight gradient, x: channel c holds value c everywhere, g_z is a single 1.0: dW[0, c] = bf16(value c)
        x = v32.view(1, 5, 1, 1).expand(1, 5, K, K).contiguous().cuda()
        dW = torch.empty((1, 5, K, K), dtype=F32, device='cuda')
        ops.conv_wgrad_kxk(x, one, dW, None, mma='bf16')
        got = dW.cpu().double().numpy()
        for c in range(5):
            assert (got[0, c] == want[c]).all(), (K, c, got[0, c], want[c])
        # weight gradient, g_z: channel c holds value c, x is 1.0 everywhere: dW[c, 0] = bf16(value c), db[c] = value c
        dW, db = torch.empty((5, 1, K, K), dtype=F32, device='cuda'), torch.empty(5, dtype=F32, device='cuda')
        ops.conv_wgrad_kxk(torch.ones((1, 1, K, K), dtype=F32, device='cuda'), gz, dW, db, mma='bf16')
        got = dW.cpu().double().numpy()
        for c in range(5):
            assert (got[c, 0] == want[c]).all(), (K, c, got[c, 0], want[c])
        assert db.cpu().double().tolist() == vals                # not rounded


# ---- 4. several slabs: the same bits twice ----
def test_the_same_inputs_give_the_same_bits_twice_with_several_slabs(built_lib):
    from iterative_inference_segm_amd import _lib, ops
    lib = _lib.load()
    rng = np.random.default_rng(5)
    # the weight gradient at K = 1 over 3 x 37 x 150 pixels
    x = torch.from_numpy(rng.standard_normal((3, 64, 37, 150)).astype(np.float32))
    gz = torch.from_numpy(rng.standard_normal((3, 130, 37, 150)).astype(np.float32))
    d = ops.conv_wgrad_kxk_desc(x, 130, 1)
    assert lib.iiseg_conv_wgrad_kxk_bf16_slabs(C.byref(d)) >= 2
    xd, gzd = x.cuda(), gz.cuda()
    runs = []
    for _ in range(2):
        dW, db = torch.empty((130, 64, 1, 1), dtype=F32, device='cuda'), torch.empty(130, dtype=F32, device='cuda')
        ops.conv_wgrad_kxk(xd, gzd, dW, db, mma='bf16')
        runs.append((dW.cpu(), db.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    fw = _wgrad_bound_check(runs[0][0], runs[0][1], x, gz, '64 -> 130 at 37x150, K = 1')[0]
    # the data gradient 130 -> 33 at K = 7: nine k-tiles over two pixel tiles
    gz = torch.from_numpy(rng.standard_normal((2, 130, 7, 7)).astype(np.float32))
    W = torch.from_numpy((0.1 * rng.standard_normal((130, 33, 7, 7))).astype(np.float32))
    d = ops.conv_dgrad_kxk_desc(tuple(gz.shape), tuple(W.shape))
    assert lib.iiseg_conv_dgrad_kxk_bf16_slabs(C.byref(d)) >= 2
    gzd, Wd = gz.cuda(), W.cuda()
    outs = [ops.conv_dgrad_kxk(gzd, Wd).cpu() for _ in range(2)]
    assert torch.equal(outs[0], outs[1])
    fd = _dgrad_bound_check(outs[0], gz, W, what='130 -> 33 at 13x13, K = 7')[0]
    print('several slabs: worst error / bound dW %.3g, gx %.3g' % (fw, fd))


# ---- 5. the module ----
class _Recorder:
    """ops.conv_wgrad_kxk (its mma='bf16' calls) and ops.conv_dgrad_kxk, recording every call's operands (copied:
    the walk reuses its buffers) and its result."""

    def __init__(self, ops):
        self.ops, self.wg, self.dg, self.wcalls, self.dcalls = ops, ops.conv_wgrad_kxk, ops.conv_dgrad_kxk, [], []

    @staticmethod
    def _cp(t):
        return None if t is None else t.detach().cpu().clone()

    def wgrad(self, x, gz, dW, db=None, window=None, ci0=0, layout='oihw', mma='f32'):
        self.wg(x, gz, dW, db, window=window, ci0=ci0, layout=layout, mma=mma)
        if mma == 'bf16':
            self.wcalls.append(dict(x=self._cp(x), gz=self._cp(gz), dW=self._cp(dW), db=self._cp(db), window=window,
                                    ci0=ci0, layout=layout, dtypes=(x.dtype, gz.dtype, dW.dtype)))

    def dgrad(self, gz, W, ci0=0, cin=None, layout='oihw', out=None, accumulate=False, gate=None, packed=None):
        c = dict(gz=self._cp(gz), W=self._cp(W), ci0=ci0, cin=cin, layout=layout, gate=self._cp(gate), packed=packed,
                 old=self._cp(out) if accumulate else None, dtypes=(gz.dtype, W.dtype))
        res = self.dg(gz, W, ci0=ci0, cin=cin, layout=layout, out=out, accumulate=accumulate, gate=gate, packed=packed)
        c['gx'] = self._cp(res)
        self.dcalls.append(c)
        return res

    def __enter__(self):
        self.ops.conv_wgrad_kxk, self.ops.conv_dgrad_kxk = self.wgrad, self.dgrad
        return self

    def __exit__(self, *exc):
        self.ops.conv_wgrad_kxk, self.ops.conv_dgrad_kxk = self.wg, self.dg


GEOMS = {'26x30': (3, 26, 30), '64x58': (2, 64, 58)}
FCN8_3X3 = [n for names in RF.BLOCKS for n in names]
SAME = ['upsample', 'score4', 'score_pool3', 'score2', 'score_pool4', 'score_fr']
_FCN = {}


def _fcn_case(geom):
    if ('case', geom) not in _FCN:
        _FCN[('case', geom)] = RF.make_case(*GEOMS[geom], seed=5)
    return _FCN[('case', geom)]


def _fcn8(geom, kxk, wgrad='f32', dgrad='f32', params=None):
    from iterative_inference_segm_amd.fcn8 import FCN8
    return FCN8(params if params is not None else _fcn_case(geom)[0], RF.SMALL['n_classes'], layer=['score'],
                dtype=F32, mma='f32', trainable=True, wgrad=wgrad, dgrad=dgrad, kxk=kxk)


def _fcn_runs(geom):
    """Both modes' forward_train / backward on one case with the same dropout masks, once."""
    if ('runs', geom) in _FCN:
        return _FCN[('runs', geom)]
    from iterative_inference_segm_amd import ops
    params, x, T, k6, k7 = _fcn_case(geom)
    xd, Td, k6d, k7d = _dev(x), _dev(T), _dev(k6), _dev(k7)
    out = {}
    for mode in ('f32', 'bf16'):
        net = _fcn8(geom, mode)
        assert net.kxk == mode and net.wgrad == net.dgrad == 'f32'
        score = net.forward_train(xd, k6d, k7d)
        _, g, _ = ops.ctx_loss(score, Td, ('crossentropy',), 1.0)
        with _Recorder(ops) as rec:
            grads = net.backward(g)
        torch.cuda.synchronize()
        out[mode] = dict(score=score.clone(), g=g.clone(), wcalls=rec.wcalls, dcalls=rec.dcalls,
                         bwd_names=sorted(net._bwd_convs()), dpack=sorted(net._dpack),
                         saved={k: (v.clone() if torch.is_tensor(v) else v) for k, v in net.saved_maps().items()},
                         grads={n: (a.clone(), b.clone()) for n, (a, b) in grads.items()})
    _FCN[('runs', geom)] = out
    return out


@pytest.mark.parametrize('geom', list(GEOMS))
def test_fcn8_changes_nothing_but_what_fc6_and_fc7_reach(built_lib, geom):
    runs = _fcn_runs(geom)
    a, b = runs['f32'], runs['bf16']
    assert a['wcalls'] == [] and a['dcalls'] == [] and a['dpack'] == []          # the default never uses the mode
    assert len(b['wcalls']) == 2 and len(b['dcalls']) == 2 and b['dpack'] == ['fc6', 'fc7']
    worst = 0.0
    for k, c in enumerate(b['wcalls']):                          # fc7, then fc6
        assert c['dtypes'] == (F32, F32, F32) and c['layout'] == 'oihw' and c['window'] is None, k
        worst = max(worst, _wgrad_bound_check(c['dW'], c['db'], c['x'], c['gz'], 'module wgrad call %d' % k)[0])
    for k, c in enumerate(b['dcalls']):
        assert c['dtypes'] == (F32, F32) and c['layout'] == 'oihw' and c['gate'] is None and c['old'] is None, k
        assert c['packed'] is not None and c['packed'].dtype == torch.bfloat16, k
        assert c['ci0'] == 0 and c['cin'] is None
        worst = max(worst, _dgrad_bound_check(c['gx'], c['gz'], c['W'], what='module dgrad call %d' % k)[0])
    assert tuple(b['wcalls'][0]['dW'].shape[2:]) == (1, 1) and tuple(b['wcalls'][1]['dW'].shape[2:]) == (7, 7)
    # fc6's g_z goes in as it is: no zero-bordered copy
    assert tuple(b['dcalls'][1]['gz'].shape[2:]) == RF.fc6_hw(*GEOMS[geom][1:])
    assert tuple(b['dcalls'][1]['gx'].shape) == tuple(a['saved']['in_fc6'].shape)
    # no fp32 flipped copy of fc6 / fc7
    assert b['bwd_names'] == sorted(set(a['bwd_names']) - {'fc6', 'fc7'})
    assert 'fc6' in a['bwd_names'] and 'fc7' in a['bwd_names'] and 'score_fr' in b['bwd_names']
    # the forward, every saved map, and every gradient no rounded operand reaches: the same bits
    assert torch.equal(a['score'], b['score'])
    assert sorted(a['saved']) == sorted(b['saved'])
    for k, v in a['saved'].items():
        if torch.is_tensor(v):
            assert torch.equal(v, b['saved'][k]), k
    for n in SAME:
        assert torch.equal(a['grads'][n][0], b['grads'][n][0]) and torch.equal(a['grads'][n][1], b['grads'][n][1]), n
    assert torch.equal(a['grads']['fc7'][1], b['grads']['fc7'][1])               # fc7's g_z is score_fr's fp32 gradient
    for n in ('fc6', 'fc7'):
        assert not torch.equal(a['grads'][n][0], b['grads'][n][0]), n
    print('FCN-8 kxk bf16 (%s): worst error / bound over the four calls %.3g' % (geom, worst))


def _ref_maps(saved):
    """FCN8.saved_maps() as the dict tests/fcn8_train_ref.backward reads (float64)."""
    s = {k: (v.cpu().double().numpy() if torch.is_tensor(v) else v) for k, v in saved.items()}
    for sname, pool in (('score_pool4', 'pool4'), ('score_pool3', 'pool3')):
        oy, ox, H, W = s['win_' + sname]
        s['in_' + sname] = np.ascontiguousarray(s[pool][:, :, oy:oy + H, ox:ox + W])
    s['p'], s['pad'] = 0.5, 100
    return s


def _np(grads):
    return {n: tuple(a.detach().cpu().double().numpy() for a in v) for n, v in grads.items()}


@pytest.mark.parametrize('geom', list(GEOMS))
def test_fcn8_chain_error_is_the_restatements(built_lib, geom):
    params = _fcn_case(geom)[0]
    runs = _fcn_runs(geom)
    s = _ref_maps(runs['f32']['saved'])                          # teacher-forced
    g = runs['f32']['g'].cpu().double().numpy()
    ref32, ref16 = KR.fcn8_backward(params, s, g), KR.fcn8_backward(params, s, g, rounded=True)
    names = ['fc6', 'fc7'] + FCN8_3X3
    pick = lambda d: {n: d[n] for n in names}
    cg = KR.cosines(pick(_np(runs['bf16']['grads'])), pick(_np(runs['f32']['grads'])))
    cr = KR.cosines(pick(ref16), pick(ref32))
    print('FCN-8 (%s) kxk bf16 against f32, 1 - cosine per array: on the GPU %s; float64 restatement with the rounding '
          'points %s' % (geom, {n: '%.3g' % (1 - c) for n, c in cg.items()}, {n: '%.3g' % (1 - c) for n, c in cr.items()}))
    for n in cg:
        # (the factor 2: fp32 accumulation order)
        assert 1 - cg[n] <= 2 * (1 - cr[n]) + 1e-6, (geom, n, 1 - cg[n], 1 - cr[n])


# ---- 6. a step, then refresh() ----
def _trainer(geom, kxk, wgrad='f32', dgrad='f32', params=None, **kw):
    from iterative_inference_segm_amd.train import FCN8Trainer
    C_ = RF.SMALL['n_classes']
    return FCN8Trainer(_fcn8(geom, kxk, wgrad, dgrad, params), C_, [C_], **kw)


@pytest.mark.parametrize('others', ['f32', 'bf16'])
def test_a_step_then_refresh_leaves_a_module_equal_to_a_fresh_one(built_lib, others):
    params, x, T, k6, k7 = _fcn_case('26x30')
    xd, Td, k6d, k7d = _dev(x), _dev(T), _dev(k6), _dev(k7)
    kw = dict(learning_rate=1e-2, weight_decay=1e-4)
    flats = []
    for _ in range(2):
        tr = _trainer('26x30', 'bf16', others, others, **kw)
        assert (tr.net.kxk, tr.net.wgrad, tr.net.dgrad) == ('bf16', others, others)
        tr.train_step(xd, Td, k6d, k7d)                          # packs the filter images, steps, refresh()
        torch.cuda.synchronize()
        flats.append(tr.net.flat.clone())
    assert torch.equal(flats[0], flats[1]) and bool(torch.isfinite(flats[0]).all())
    f32 = _trainer('26x30', 'f32', others, others, **kw)
    f32.train_step(xd, Td, k6d, k7d)
    assert not torch.equal(f32.net.flat, flats[0])
    assert 'fc6' in f32.net._bwd and 'fc6' not in f32.net._dpack
    # the images are stale after refresh() and packed again into the buffers they have
    assert not ({'fc6', 'fc7'} & tr.net._dpack_fresh)
    ptrs = {n: tr.net._dpack[n].data_ptr() for n in ('fc6', 'fc7')}
    fresh = _trainer('26x30', 'bf16', others, others, params=tr.net.state_arrays(), **kw)
    assert torch.equal(fresh.net.flat, tr.net.flat)
    grads = []
    for t in (tr, fresh):
        from iterative_inference_segm_amd import ops
        score = t.net.forward_train(xd, k6d, k7d)
        _, g, _ = ops.ctx_loss(score, Td, ('crossentropy',), 1.0)
        t.net.backward(g)
        torch.cuda.synchronize()
        grads.append(t.net.gflat.clone())
    assert torch.equal(grads[0], grads[1])                       # the next step's gradients, bit for bit
    assert {n: tr.net._dpack[n].data_ptr() for n in ('fc6', 'fc7')} == ptrs


# ---- 7. training ----
def test_loss_goes_down_over_40_steps_with_all_three_bf16_modes(built_lib):
    x, T = _fcn_case('26x30')[1:3]
    tr = _trainer('26x30', 'bf16', 'bf16', 'bf16', learning_rate=1e-3, seed=2)
    xd, Td = _dev(x), _dev(T)
    losses = [tr.train_step(xd, Td) for _ in range(40)]
    losses = [float(v) for v in torch.stack(losses).cpu()]
    print('FCN-8 loss, wgrad, dgrad and kxk bf16, steps 0-9: %.5f, steps 30-39: %.5f'
          % (np.mean(losses[:10]), np.mean(losses[-10:])))
    assert np.all(np.isfinite(losses))
    assert np.mean(losses[-10:]) < np.mean(losses[:10])


def test_train_fcn8_driver_end_to_end_with_kxk_bf16(built_lib, tmp_path):
    from iterative_inference_segm_amd.fcn8 import buildFCN8
    save = str(tmp_path / 'save')
    # two epochs: as in the reference, the driver's first epoch only sets the best validation score and writes no
    # checkpoint (train_fcn8.py's `epoch == 0` branch), so a one-epoch run has none to load
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_fcn8.py'), '--synthetic', '-ne', '2',
                        '--n_images', '2', '--image_size', '26', '30', '-batch_size', '[2, 2, 2]', '--savepath', save,
                        '--width_div', '16', '--fc_channels', '32', '--max_batches', '1', '-penal_cst', '1e-4',
                        '--kxk', 'bf16'], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert os.listdir(os.path.join(save, 'camvid')) == ['fcn8_data_aug']     # the fp32 run's folder
    folder = os.path.join(save, 'camvid', 'fcn8_data_aug')
    lines = open(os.path.join(folder, 'config.txt')).read().splitlines()
    assert 'kxk = bf16' in lines and 'wgrad = f32' in lines and 'dgrad = f32' in lines
    models = [f for f in os.listdir(folder) if f in ('new_fcn8_model_best.npz', 'new_fcn8_model_last.npz')]
    assert models
    net = buildFCN8(3, path_weights=os.path.join(folder, models[0]), n_classes=11)
    x = _dev(np.random.default_rng(1).random((2, 3, 26, 30)))
    probs = net(x)[0]
    assert tuple(probs.shape) == (2, 11, 26, 30) and bool(torch.isfinite(probs).all())
