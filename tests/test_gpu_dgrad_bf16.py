"""GPU: the 16-bit data-gradient mode (dgrad='bf16'; csrc/conv_dgrad_bf16.hip).  The kernel:
exact on data bf16 holds exactly (channel tails, channel slices in both layouts, accumulate, gate); on real data
within the any-order fp32 accumulation bound of the float64 sum over operands rounded on the CPU with
.to(torch.bfloat16), ties and direction included; the same bits twice.  The modules: between dgrad='f32' and 'bf16'
the forward, the saved maps, backward_y and the gradients no rounded data gradient reaches keep their bits, every
ops.conv_dgrad call of `backward` meets the bound on its own operands, no fp32 flipped-filter layer of a 3x3 layer
is built, and the chain's cosine to the fp32 gradients is that of the float64 restatement with the same rounding
points (tests/dgrad_bf16_ref.py).  Training and the two drivers run in the mode.

Measured on an MI355X (for the record; the assertions are the derived bounds): see DESIGN.md section 16."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dgrad_bf16_ref as D
import fcn8_train_ref as RF
import std_train_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = torch.float32
U = 2.0 ** -24


def _dev(a, dt=F32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda().contiguous()


def _dgrad(gz, W):
    """[b, ci, y, x] = sum_{co,ky,kx} W[co, ci, ky, kx] gz[b, co, y + 1 - ky, x + 1 - kx], gz zero outside its plane"""
    H, Wd = gz.shape[2:]
    gp = np.pad(gz, ((0, 0), (0, 0), (1, 1), (1, 1)))
    out = np.zeros((gz.shape[0], W.shape[1], H, Wd), dtype=np.result_type(gz.dtype, W.dtype))
    for ky in range(3):
        for kx in range(3):
            out += np.einsum('oi,bohw->bihw', W[:, :, ky, kx], gp[:, :, 2 - ky:2 - ky + H, 2 - kx:2 - kx + Wd])
    return out


# ---- 1. exact on small integers ----
CHANNELS = [(11, 64), (24, 16), (64, 130), (130, 33)]            # no multiples of the 64 / 32 blocks; k tails
MAPS = [(1, 1), (2, 9), (7, 7), (14, 13), (37, 150)]
_REF = {}


def _int_case(Cin, Cout, B, H, W):
    key = (Cin, Cout, B, H, W)
    if key not in _REF:
        rng = np.random.default_rng(Cin * 1000 + Cout + 7 * B + H)
        Wt = rng.integers(-2, 3, size=(Cout, Cin, 3, 3))
        gz = rng.integers(-2, 3, size=(B, Cout, H, W))
        gz[rng.integers(0, 2, size=gz.shape) == 0] = 0           # as behind a ReLU mask
        old = rng.integers(-2, 3, size=(B, Cin, H, W))           # what `accumulate` adds to
        gate = rng.integers(-1, 2, size=(B, Cin, H, W))          # zeros and negatives close the gate
        gx = _dgrad(gz.astype(np.int64), Wt.astype(np.int64))
        assert gx.dtype == np.int64 and np.abs(gx).max() + 2 < 2 ** 24
        _REF[key] = (Wt, gz, old, gate, gx)
    return _REF[key]


@pytest.mark.parametrize('H,W', MAPS)
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('Cin,Cout', CHANNELS)
def test_bf16_data_gradient_is_exact_on_integers(built_lib, Cin, Cout, B, H, W):
    from iterative_inference_segm_amd import ops
    Wt, gz, old, gate, ref = _int_case(Cin, Cout, B, H, W)
    Wd, gzd = _dev(Wt), _dev(gz)
    # the layer's own parameter, W[out, in, 3, 3]
    got = ops.conv_dgrad(gzd, Wd)
    # the middle channels of a wider parameter, in both layouts: the other input channels hold NaN
    lo, hi = 3, 5
    big = torch.full((Cout, lo + Cin + hi, 3, 3), float('nan'), dtype=F32, device='cuda')
    big[:, lo:lo + Cin] = Wd
    mid = ops.conv_dgrad(gzd, big, ci0=lo, cin=Cin)
    bigT = big.transpose(0, 1).contiguous()
    midT = ops.conv_dgrad(gzd, bigT, ci0=lo, cin=Cin, layout='iohw')
    # onto an integer map, in place; behind a gate; both
    acc = _dev(old)
    assert ops.conv_dgrad(gzd, Wd, out=acc, accumulate=True) is acc
    gated = ops.conv_dgrad(gzd, Wd, gate=_dev(gate))
    both = _dev(old)
    ops.conv_dgrad(gzd, Wd, out=both, accumulate=True, gate=_dev(gate))
    torch.cuda.synchronize()
    want = ref.astype(np.float64)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(mid.cpu().numpy(), want)
    assert np.array_equal(midT.cpu().numpy(), want)
    assert np.array_equal(acc.cpu().numpy(), want + old)
    assert np.array_equal(gated.cpu().numpy(), np.where(gate > 0, want, 0.0))
    assert np.array_equal(both.cpu().numpy(), np.where(gate > 0, want + old, 0.0))


# ---- 2. the rounding point ----
def _rounded(t):
    """float64 numpy of a float32 tensor rounded to bf16 on the CPU"""
    return t.detach().cpu().to(torch.bfloat16).double().numpy()


def _truncated(t):
    """... and with the low 16 bits cut off instead"""
    bits = t.detach().cpu().contiguous().view(torch.int32) & ~0xFFFF
    return bits.view(torch.float32).double().numpy()


def _bound_check(gx, gz, W, old=None, gate=None, what=''):
    """gx (B, Cin, H, W) against the float64 sum over W (Cout, Cin, 3, 3) and gz (float32 tensors) rounded to bf16
    on the CPU: every entry within (n + 1) 2^-24 sum|a b|, n = 9 Cout -- the bound of n fp32 additions of exact
    products in ANY order, sum|a b| per entry from the rounded data.  old: what the call added to, one more term of
    the fp32 sum (n + 2, |old| in the magnitude).  gate: closed entries are exactly zero.  Returns (worst error /
    bound, ref, mag)."""
    n = 9 * gz.shape[1]
    g, w = _rounded(gz), _rounded(W)
    ref, mag = _dgrad(g, w), _dgrad(np.abs(g), np.abs(w))
    if old is not None:
        o = old.detach().cpu().double().numpy()
        ref, mag, n = ref + o, mag + np.abs(o), n + 1
    got = gx.detach().cpu().double().numpy()
    if gate is not None:
        closed = ~(gate.detach().cpu().numpy() > 0)
        assert (got[closed] == 0).all(), what
        ref, mag = np.where(closed, 0.0, ref), np.where(closed, 0.0, mag)
    err = np.abs(got - ref)
    bound = (n + 1) * U * mag
    frac = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    assert (err <= bound).all(), '%s: worst error / bound %.3g over %d terms' % (what, frac, n)
    return frac, ref, mag


def test_operands_are_rounded_to_nearest_once(built_lib):
    from iterative_inference_segm_amd import ops
    rng = np.random.default_rng(5)
    gz = torch.from_numpy(rng.standard_normal((1, 16, 7, 7)).astype(np.float32))
    W = torch.from_numpy((0.1 * rng.standard_normal((16, 24, 3, 3))).astype(np.float32))
    gx = ops.conv_dgrad(gz.cuda(), W.cuda())
    torch.cuda.synchronize()
    frac, ref, mag = _bound_check(gx, gz, W, what='rounding point')
    # (the statement discriminates: the sums over the UNROUNDED and over the TRUNCATED operands leave the bound)
    n = 9 * 16
    got = gx.cpu().double().numpy()
    exact = _dgrad(gz.double().numpy(), W.double().numpy())
    trunc = _dgrad(_truncated(gz), _truncated(W))
    out_exact = float((np.abs(got - exact) > (n + 1) * U * mag).mean())
    out_trunc = float((np.abs(got - trunc) > (n + 1) * U * mag).mean())
    print('bf16 dgrad 16 -> 24 at 7x7: worst error / bound %.3g; outside the bound of the unrounded sum %.3f, of the '
          'truncated sum %.3f of the entries' % (frac, out_exact, out_trunc))
    assert out_exact >= 0.9 and out_trunc >= 0.9


def test_ties_go_to_even_and_negative_values_round_symmetrically(built_lib):
    from iterative_inference_segm_amd import ops
    vals = [1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -10, -(1 + 2.0 ** -8 + 2.0 ** -10),
            1 + 2.0 ** -7 - 2.0 ** -10]
    want = [1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, -(1 + 2.0 ** -7), 1 + 2.0 ** -7]
    v32 = torch.tensor(vals, dtype=F32)
    assert v32.double().tolist() == vals                         # float32 holds them
    assert v32.to(torch.bfloat16).double().tolist() == want      # torch's rounding on the CPU
    # W[0, c] holds value c at every tap; g_z is a single 1.0 at the centre: every pixel of gx[0, c] meets it under
    # exactly one tap, gx[0, c, y, x] = bf16(value c)
    W = v32.view(1, 5, 1, 1).expand(1, 5, 3, 3).contiguous().cuda()
    gz = torch.zeros((1, 1, 3, 3), dtype=F32, device='cuda')
    gz[0, 0, 1, 1] = 1.0
    got = ops.conv_dgrad(gz, W).cpu().double().numpy()
    for c in range(5):
        assert (got[0, c] == want[c]).all(), (c, got[0, c], want[c])
    # and in the other operand: g_z holds value c at the centre of channel c, W[co, ci] is 1.0 at every tap of co == ci
    gz = torch.zeros((1, 5, 3, 3), dtype=F32)
    gz[0, :, 1, 1] = v32
    W = torch.eye(5, dtype=F32).view(5, 5, 1, 1).expand(5, 5, 3, 3).contiguous()
    got = ops.conv_dgrad(gz.cuda(), W.cuda()).cpu().double().numpy()
    for c in range(5):
        assert (got[0, c] == want[c]).all(), (c, got[0, c], want[c])


# ---- 3. the same bits twice ----
def test_the_same_inputs_give_the_same_bits_twice_within_the_bound(built_lib):
    from iterative_inference_segm_amd import ops
    rng = np.random.default_rng(5)
    gz = torch.from_numpy(rng.standard_normal((1, 130, 37, 150)).astype(np.float32))
    W = torch.from_numpy((0.1 * rng.standard_normal((130, 130, 3, 3))).astype(np.float32))
    gzd, Wd = gz.cuda(), W.cuda()
    runs = [ops.conv_dgrad(gzd, Wd).cpu() for _ in range(2)]
    assert torch.equal(runs[0], runs[1])
    frac = _bound_check(runs[0], gz, W, what='130 -> 130 at 37x150')[0]
    print('bf16 dgrad 130 -> 130 at 37x150: worst error / bound %.3g' % frac)


# ---- 4. the modules, 5. the chain ----
class _Recorder:
    """ops.conv_dgrad, recording every call's operands (copied: the walks reuse their buffers) and its result."""

    def __init__(self, ops):
        self.ops, self.inner, self.calls = ops, ops.conv_dgrad, []

    def __call__(self, gz, W, ci0=0, cin=None, layout='oihw', out=None, accumulate=False, gate=None, packed=None):
        cp = lambda t: None if t is None else t.detach().cpu().clone()
        c = dict(gz=cp(gz), W=cp(W), ci0=ci0, cin=cin, layout=layout, old=cp(out) if accumulate else None,
                 gate=cp(gate), packed=packed, dtypes=(gz.dtype, W.dtype))
        res = self.inner(gz, W, ci0=ci0, cin=cin, layout=layout, out=out, accumulate=accumulate, gate=gate,
                         packed=packed)
        c['gx'] = cp(res)
        self.calls.append(c)
        return res

    def __enter__(self):
        self.ops.conv_dgrad = self
        return self

    def __exit__(self, *exc):
        self.ops.conv_dgrad = self.inner


def _check_calls(calls, n_expected, what):
    """Every call is the mode's (float32 operands, the module's own packed image, W[out, in, 3, 3]) and meets the
    bound on its own operands."""
    assert len(calls) == n_expected, (what, len(calls), n_expected)
    worst = 0.0
    for k, c in enumerate(calls):
        assert c['dtypes'] == (F32, F32) and c['layout'] == 'oihw', (what, k)
        assert c['packed'] is not None and c['packed'].dtype == torch.bfloat16, (what, k)
        cin = c['W'].shape[1] - c['ci0'] if c['cin'] is None else c['cin']
        Wsl = c['W'][:, c['ci0']:c['ci0'] + cin]
        worst = max(worst, _bound_check(c['gx'], c['gz'], Wsl, c['old'], c['gate'], '%s call %d' % (what, k))[0])
    return worst


def _np(grads):
    return {n: tuple(a.detach().cpu().double().numpy() for a in v) for n, v in grads.items()}


MODELS = {'small': R.SMALL, 'second': R.SECOND}
_STD, _RUNS = {}, {}


def _std_case(which):
    if which not in _STD:
        _STD[which] = R.make_case(MODELS[which])
    return _STD[which]


def _std_dae(which, dgrad, wgrad='f32'):
    from iterative_inference_segm_amd.dae import StandardDAE
    return StandardDAE(_std_case(which)[0], MODELS[which][0], device='cuda', dtype=F32, mma='f32', trainable=True,
                       wgrad=wgrad, dgrad=dgrad, **MODELS[which][3])


def _std_runs(which):
    """Both modes' forward_train / backward / backward_y on one case, once."""
    if which in _RUNS:
        return _RUNS[which]
    from iterative_inference_segm_amd import ops
    params, hs, y, T = _std_case(which)
    hd, yd, Td = [_dev(h) for h in hs], _dev(y), _dev(T)
    out = {}
    for mode in ('f32', 'bf16'):
        dae = _std_dae(which, mode)
        assert dae.dgrad == mode and dae.wgrad == 'f32' and dae.mma == 'f32'
        score = dae.forward_train(hd, yd)
        _, g, _ = ops.ctx_loss(score, Td, ('crossentropy',), 1.0)
        with _Recorder(ops) as rec:
            grads = dae.backward(g)
        torch.cuda.synchronize()
        out[mode] = dict(score=score.clone(), saved={k: v.clone() for k, v in dae.saved_maps().items()},
                         grads={n: (a.clone(), b.clone()) for n, (a, b) in grads.items()}, calls=rec.calls,
                         bwd_after_backward=dae._bwd, g=g.clone())
        out[mode]['gy'] = dae.backward_y(g, yd.shape).clone()
    _RUNS[which] = out
    return out


@pytest.mark.parametrize('which', ['small', 'second'])
def test_standard_dae_changes_nothing_but_what_the_data_gradients_reach(built_lib, which):
    cfg = MODELS[which][3]
    runs = _std_runs(which)
    a, b = runs['f32'], runs['bf16']
    assert a['calls'] == []                                      # the default never calls the op
    worst = _check_calls(b['calls'], len(R.order_of(cfg)) - 1, 'standard DAE ' + which)
    assert b['bwd_after_backward'] is None                       # no fp32 flipped-filter layer was built
    assert torch.equal(a['score'], b['score']) and torch.equal(a['gy'], b['gy'])
    assert sorted(a['saved']) == sorted(b['saved'])
    for k in a['saved']:
        assert torch.equal(a['saved'][k], b['saved'][k]), k
    assert torch.equal(a['grads']['up_conv1'][0], b['grads']['up_conv1'][0])
    assert torch.equal(a['grads']['up_conv1'][1], b['grads']['up_conv1'][1])
    assert any(not torch.equal(a['grads'][n][0], b['grads'][n][0]) for n in a['grads'] if n != 'up_conv1')
    print('standard DAE (%s) dgrad bf16: %d calls, worst error / bound %.3g' % (which, len(b['calls']), worst))


def _chain_check(got16, got32, ref16, ref32, what):
    cg, cr = D.cosines(got16, got32), D.cosines(ref16, ref32)
    print('%s dgrad bf16 against f32, 1 - cosine per array: on the GPU %s; float64 restatement with the rounding '
          'points %s' % (what, {n: '%.3g' % (1 - c) for n, c in cg.items()}, {n: '%.3g' % (1 - c) for n, c in cr.items()}))
    for n in cg:
        # (the factor 2: fp32 accumulation order)
        assert 1 - cg[n] <= 2 * (1 - cr[n]) + 1e-6, (what, n, 1 - cg[n], 1 - cr[n])


@pytest.mark.parametrize('which', ['small', 'second'])
def test_standard_dae_chain_error_is_the_restatements(built_lib, which):
    cfg = MODELS[which][3]
    params, hs, y, T = _std_case(which)
    runs = _std_runs(which)
    saved = {k: v.cpu().double().numpy() for k, v in runs['f32']['saved'].items()}      # teacher-forced
    g = runs['f32']['g'].cpu().double().numpy()
    ref32 = D.std_backward(params, hs, saved, g, cfg)
    ref16 = D.std_backward(params, hs, saved, g, cfg, rounded=True)
    _chain_check(_np(runs['bf16']['grads']), _np(runs['f32']['grads']), ref16, ref32, 'standard DAE (%s)' % which)


FCN8_3X3 = [n for names in RF.BLOCKS for n in names]
_FCN = {}


def _fcn_case():
    if 'case' not in _FCN:
        _FCN['case'] = RF.make_case(3, 26, 30, seed=5)
    return _FCN['case']


def _fcn8(dgrad, wgrad='f32', params=None, **kw):
    from iterative_inference_segm_amd.fcn8 import FCN8
    return FCN8(params if params is not None else _fcn_case()[0], RF.SMALL['n_classes'], layer=['score'], dtype=F32,
                mma='f32', trainable=True, wgrad=wgrad, dgrad=dgrad, **kw)


def _fcn_runs():
    if 'runs' in _FCN:
        return _FCN['runs']
    from iterative_inference_segm_amd import ops
    params, x, T, k6, k7 = _fcn_case()
    xd, Td, k6d, k7d = _dev(x), _dev(T), _dev(k6), _dev(k7)
    out = {}
    for mode in ('f32', 'bf16'):
        net = _fcn8(mode)
        assert net.dgrad == mode and net.wgrad == 'f32'
        score = net.forward_train(xd, k6d, k7d)
        _, g, _ = ops.ctx_loss(score, Td, ('crossentropy',), 1.0)
        with _Recorder(ops) as rec:
            grads = net.backward(g)
        torch.cuda.synchronize()
        out[mode] = dict(score=score.clone(), g=g.clone(), calls=rec.calls, bwd_names=sorted(net._bwd),
                         saved={k: (v.clone() if torch.is_tensor(v) else v) for k, v in net.saved_maps().items()},
                         grads={n: (a.clone(), b.clone()) for n, (a, b) in grads.items()})
    _FCN['runs'] = out
    return out


def test_fcn8_changes_nothing_but_what_the_twelve_data_gradients_reach(built_lib):
    runs = _fcn_runs()
    a, b = runs['f32'], runs['bf16']
    assert a['calls'] == []
    worst = _check_calls(b['calls'], 12, 'FCN-8')
    # the gate of the block's previous layer rides on eight of them; conv*_1's go on to a pool
    assert sum(c['gate'] is not None for c in b['calls']) == 8
    assert b['bwd_names'] == sorted(['fc6', 'fc7', 'score_fr', 'score_pool3', 'score_pool4'])   # no 3x3 layer's
    assert sorted(set(a['bwd_names']) - set(b['bwd_names'])) == sorted(FCN8_3X3[1:])
    assert torch.equal(a['score'], b['score'])
    assert sorted(a['saved']) == sorted(b['saved'])
    for k, v in a['saved'].items():
        if torch.is_tensor(v):
            assert torch.equal(v, b['saved'][k]), k
    stay = [n for n in a['grads'] if n not in FCN8_3X3]
    assert sorted(stay) == sorted(['fc6', 'fc7', 'score_fr', 'score_pool3', 'score_pool4', 'score2', 'score4',
                                   'upsample'])
    for n in stay + ['conv5_3']:
        assert torch.equal(a['grads'][n][0], b['grads'][n][0]) and torch.equal(a['grads'][n][1], b['grads'][n][1]), n
    assert any(not torch.equal(a['grads'][n][0], b['grads'][n][0]) for n in FCN8_3X3 if n != 'conv5_3')
    print('FCN-8 dgrad bf16: %d calls, worst error / bound %.3g' % (len(b['calls']), worst))


def _ref_maps(saved):
    """FCN8.saved_maps() as the dict tests/fcn8_train_ref.backward reads (float64)."""
    s = {k: (v.cpu().double().numpy() if torch.is_tensor(v) else v) for k, v in saved.items()}
    for sname, pool in (('score_pool4', 'pool4'), ('score_pool3', 'pool3')):
        oy, ox, H, W = s['win_' + sname]
        s['in_' + sname] = np.ascontiguousarray(s[pool][:, :, oy:oy + H, ox:ox + W])
    s['p'], s['pad'] = 0.5, 100
    return s


def test_fcn8_chain_error_is_the_restatements(built_lib):
    params = _fcn_case()[0]
    runs = _fcn_runs()
    s = _ref_maps(runs['f32']['saved'])                          # teacher-forced
    g = runs['f32']['g'].cpu().double().numpy()
    ref32, ref16 = D.fcn8_backward(params, s, g), D.fcn8_backward(params, s, g, rounded=True)
    pick = lambda d: {n: d[n] for n in FCN8_3X3}
    _chain_check(pick(_np(runs['bf16']['grads'])), pick(_np(runs['f32']['grads'])), pick(ref16), pick(ref32), 'FCN-8')


# ---- 6. training ----
def _trainer(mode, **kw):
    from iterative_inference_segm_amd.train import DAETrainer
    return DAETrainer(None, _std_dae('second', mode, wgrad=mode), 11, [11], noise=0.1, **kw)


def test_loss_goes_down_over_40_steps_with_both_bf16_modes(built_lib):
    hs, T = _std_case('second')[1], _std_case('second')[3]
    tr = _trainer('bf16', seed=2, learning_rate=1e-4)
    assert tr.dae.dgrad == tr.dae.wgrad == 'bf16'
    hd, Td = [_dev(h) for h in hs], _dev(T)
    yd = Td[:, :11].contiguous()                                 # from_gt
    losses = [tr.train_step(hd, yd, Td) for _ in range(40)]
    losses = [float(v) for v in torch.stack(losses).cpu()]
    print('standard DAE loss, wgrad and dgrad bf16, steps 0-9: %.5f, steps 30-39: %.5f'
          % (np.mean(losses[:10]), np.mean(losses[-10:])))
    assert np.all(np.isfinite(losses))
    assert np.mean(losses[-10:]) < np.mean(losses[:10])


def test_every_path_sees_the_new_weights_after_a_step(built_lib):
    hs, y, T = _std_case('second')[1:]
    hd, yd, Td = [_dev(h) for h in hs], _dev(y), _dev(T)
    tr = _trainer('bf16', seed=3, learning_rate=1e-2)
    before = tr.dae.scores(hd, yd).clone()
    tr.train_step(hd, yd, Td)                                    # packs the filter images, steps, refresh()
    torch.cuda.synchronize()
    fresh_tr = _trainer('bf16', seed=3, learning_rate=1e-2)
    fresh_tr.dae.flat.copy_(tr.dae.flat)
    fresh_tr.dae.refresh()
    eager = tr.dae.scores(hd, yd).clone()
    assert not torch.equal(eager, before)
    assert torch.equal(eager, tr.dae.scores(hd, yd, session=tr.dae.new_session(hd, yd)))
    assert torch.equal(eager, fresh_tr.dae.scores(hd, yd))
    # the filter images too: packed again, into the buffers they had; a second step on both gives the same bits
    ptrs = {n: t.data_ptr() for n, t in tr.dae._dpack.items()}
    assert len(ptrs) == len(R.order_of(R.SECOND[3])) - 1 and not tr.dae._dpack_fresh
    for t in (tr, fresh_tr):
        t.s1.zero_()
        t.train_step(hd, yd, Td, eps=torch.zeros_like(yd))
    assert torch.equal(tr.dae.flat, fresh_tr.dae.flat) and bool(torch.isfinite(tr.dae.flat).all())
    assert {n: t.data_ptr() for n, t in tr.dae._dpack.items()} == ptrs
    f32 = _trainer('f32', seed=3, learning_rate=1e-2)
    f32.train_step(hd, yd, Td)
    assert f32.dae._dpack == {} and f32.dae._bwd is not None    # the default: the fp32 flipped-filter layers


def test_train_dae_driver_end_to_end_with_bf16_data_gradients(built_lib, tmp_path):
    from iterative_inference_segm_amd.helpers import build_experiment_name
    save, load = str(tmp_path / 'save'), str(tmp_path / 'load')
    dd = {'kind': 'standard', 'dropout': 0, 'skip': True, 'unpool_type': 'trackind', 'noise': 0.1,
          'concat_h': ['pool2'], 'from_gt': True, 'n_filters': 8, 'conv_before_pool': 1, 'additional_pool': 2,
          'temperature': 1.0, 'path_weights': '', 'layer': 'probs_dimshuffle', 'exp_name': 't_', 'bn': 0}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_dae.py'), '--synthetic', '--num_epochs', '1',
                        '--n_images', '4', '--image_size', '40', '36', '--savepath', save, '--loadpath', load,
                        '-segmentation_net', 'fcn8', '-train_dict', '{"batch_size": [2, 2, 2]}',
                        '-dae_dict', json.dumps(dd), '--dgrad', 'bf16'],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    exp, = os.listdir(os.path.join(save, 'camvid'))
    # the folder of the fp32 run: the mode stays out of the name
    assert exp == build_experiment_name('fcn8', data_aug=True, ae_h=False, training_loss=['crossentropy'],
                                        learning_rate=0.0001, lr_anneal=0.99, weight_decay=0.0001,
                                        optimizer='rmsprop', **dd)
    lines = open(os.path.join(save, 'camvid', exp, 'config.txt')).read().splitlines()
    assert 'dgrad = bf16' in lines and 'wgrad = f32' in lines
    assert os.path.exists(os.path.join(load, 'camvid', exp, 'dae_model_best.npz'))


def test_train_fcn8_driver_end_to_end_with_bf16_data_gradients(built_lib, tmp_path):
    from iterative_inference_segm_amd.fcn8 import buildFCN8
    save = str(tmp_path / 'save')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_fcn8.py'), '--synthetic', '--num_epochs', '2',
                        '--n_images', '2', '--image_size', '26', '30', '-batch_size', '[2, 2, 2]', '--savepath', save,
                        '--width_div', '16', '--fc_channels', '32', '--max_batches', '1', '-penal_cst', '1e-4',
                        '--dgrad', 'bf16'], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert os.listdir(os.path.join(save, 'camvid')) == ['fcn8_data_aug']     # the fp32 run's folder
    folder = os.path.join(save, 'camvid', 'fcn8_data_aug')
    lines = open(os.path.join(folder, 'config.txt')).read().splitlines()
    assert 'dgrad = bf16' in lines and 'wgrad = f32' in lines
    models = [f for f in os.listdir(folder) if f in ('new_fcn8_model_best.npz', 'new_fcn8_model_last.npz')]
    assert models
    net = buildFCN8(3, path_weights=os.path.join(folder, models[0]), n_classes=11)
    x = _dev(np.random.default_rng(1).random((2, 3, 26, 30)))
    probs = net(x)[0]
    assert tuple(probs.shape) == (2, 11, 26, 30) and bool(torch.isfinite(probs).all())
