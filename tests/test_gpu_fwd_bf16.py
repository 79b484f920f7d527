"""GPU: FCN-8's training forward on the 16-bit matrix pipe (fwd='bf16'; csrc/conv_kxk_bf16.hip's forward kernel and
conv_halo_bf16_kernel through ops.Conv(fwd16=True)).  The new op and the 3x3 layers: exact on
data bf16 holds exactly (channel tails, every K edge, several slabs, out=, relu, bias); on real data within the
any-order fp32 accumulation bound of the float64 sum over operands rounded on the CPU, ties and direction included;
the same bits twice with several slabs.  The module: fwd='f32' is the module without the keyword bit for bit; with
fwd='bf16' every one of the fifteen layers meets its bound on the GPU's own saved input (teacher-forced: no ReLU or
pool decision enters a comparison), the pools and the score layers are the fp32 code's, and the chain's cosine to the
fp32 gradients is that of the float64 restatement with the same rounding points (tests/fwd_bf16_ref.py).  refresh()
re-packs in place; training and the driver run in the mode.

Measured on an MI355X (for the record; the assertions are the derived bounds): see DESIGN.md section 18."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fcn8_train_ref as RF
import fwd_bf16_ref as FR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = torch.float32


def _dev(a, dt=F32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda().contiguous()


def _iconv(x, W, b=None, pad=0, relu=True):
    """The layer on integer arrays, in int64."""
    x, W = x.astype(np.int64), W.astype(np.int64)
    if pad:
        x = np.pad(x, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    K = W.shape[2]
    OH, OW = x.shape[2] - K + 1, x.shape[3] - K + 1
    out = np.zeros((x.shape[0], W.shape[0], OH, OW), dtype=np.int64)
    for ky in range(K):
        for kx in range(K):
            out += np.einsum('oi,bihw->bohw', W[:, :, ky, kx], x[:, :, ky:ky + OH, kx:kx + OW])
    if b is not None:
        out += b.astype(np.int64)[None, :, None, None]
    return np.maximum(out, 0) if relu else out


# ---- 1. conv_fwd_kxk: exact on small integers ----
# tails on both sides of the output-channel block of a workgroup (64; K = 1: 128 -- 200 output channels cross both,
# with a second block and, at K = 1, the fourth 32-channel block of the first) and of the k-tiles of 8 (K >= 4),
# 16 (K = 3), 32 (K = 2), 64 (K = 1) input channels
CHANNELS = [(3, 11), (24, 16), (70, 33), (130, 65), (130, 200)]
# (K, h, w); the last two: more than one 8 x 8 pixel tile per image in both directions (outputs 10 x 19 and 10 x 17),
# so the halo crosses tile edges and, with B = 3, a workgroup's eight tiles span images
SHAPES = [(7, 7, 7), (7, 8, 9), (7, 13, 13), (1, 1, 1), (1, 7, 7), (1, 37, 150), (3, 5, 4), (2, 4, 4), (3, 12, 21),
          (7, 16, 23)]


@pytest.mark.parametrize('K,h,w', SHAPES)
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('Cin,Cout', CHANNELS)
def test_conv_fwd_kxk_is_exact_on_integers(built_lib, Cin, Cout, B, K, h, w):
    from iterative_inference_segm_amd import _lib, ops
    rng = np.random.default_rng(Cin * 1000 + Cout + 7 * B + 31 * K + h)
    x = rng.integers(-2, 3, size=(B, Cin, h, w))
    W = rng.integers(-2, 3, size=(Cout, Cin, K, K))
    b = rng.integers(-3, 4, size=(Cout,))
    assert np.abs(_iconv(x, W, b, relu=False)).max() < 2 ** 24
    xd, Wd, bd = _dev(x), _dev(W), _dev(b)
    d = ops.conv_fwd_kxk_desc(tuple(xd.shape), tuple(Wd.shape))
    slabs = _lib.load().iiseg_conv_fwd_kxk_bf16_slabs(C.byref(d))
    assert slabs >= 1
    if Cin == 130 and K in (1, 7):
        assert slabs >= 2                                        # the workspace and the finalize run
    got = ops.conv_fwd_kxk(xd, Wd, bd)                           # relu=True is the default
    lin = ops.conv_fwd_kxk(xd, Wd, bd, relu=False)
    nob = ops.conv_fwd_kxk(xd, Wd, None, relu=False)
    out = torch.full((B, Cout, h - K + 1, w - K + 1), float('nan'), dtype=F32, device='cuda')
    assert ops.conv_fwd_kxk(xd, Wd, None, relu=True, out=out) is out     # every entry is written: no NaN survives
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), _iconv(x, W, b).astype(np.float64))
    assert np.array_equal(lin.cpu().numpy(), _iconv(x, W, b, relu=False).astype(np.float64))
    assert np.array_equal(nob.cpu().numpy(), _iconv(x, W, None, relu=False).astype(np.float64))
    assert np.array_equal(out.cpu().numpy(), _iconv(x, W, None).astype(np.float64))


# ---- 2. the 3x3 layers through the module's layer class ----
def _layer(W, b, pad, relu=True):
    from iterative_inference_segm_amd import ops
    return ops.Conv(W, b, pad=pad, relu=relu, device='cuda', dtype=F32, mma='f32', fwd16=True)


CASES_3X3 = [(3, 64, 100, 8, 6)] + [(ci, co, 1, h, w) for ci, co in ((17, 33), (64, 70))
                                    for h, w in ((5, 4), (9, 33), (37, 70))]


@pytest.mark.parametrize('Cin,Cout,pad,h,w', CASES_3X3)
def test_the_3x3_layers_are_exact_on_integers(built_lib, Cin, Cout, pad, h, w):
    rng = np.random.default_rng(Cin + 100 * Cout + h)
    x = rng.integers(-2, 3, size=(2, Cin, h, w))
    W = rng.integers(-2, 3, size=(Cout, Cin, 3, 3))
    b = rng.integers(-3, 4, size=(Cout,))
    conv = _layer(W.astype(np.float32), b.astype(np.float32), pad)
    got = conv(_dev(x))
    assert conv._W16 is not None and conv._packs == {}           # the bf16 halo kernel ran, no fp32 pack was made
    assert np.array_equal(got.cpu().numpy(), _iconv(x, W, b, pad=pad).astype(np.float64))


def test_the_layer_class_takes_the_halo_form_whatever_the_picks_say(built_lib, monkeypatch):
    from iterative_inference_segm_amd import ops
    rng = np.random.default_rng(1)
    W, b = rng.standard_normal((64, 64, 3, 3)).astype(np.float32), np.zeros(64, np.float32)
    conv = _layer(W, b, 1)
    x = _dev(rng.standard_normal((1, 64, 12, 40)))
    launch = conv._describe_call(x)
    assert conv._form(launch) == 'halo_bf16'
    monkeypatch.setattr(ops, 'BF16_FORCE', 'wino')
    assert conv._form(launch) == 'halo_bf16'
    fc = _layer(rng.standard_normal((8, 64, 7, 7)).astype(np.float32), None, 0)
    assert fc._form(fc._describe_call(x)) == 'kxk_bf16'
    with pytest.raises(RuntimeError):                            # a window: neither kernel of the mode, so an error
        fc._form(fc._describe_call(x, window=(0, 0, 2, 2), out=torch.empty((1, 8, 6, 34), device='cuda'), place=(0, 0)))


# ---- 3. the rounding point, ties and direction ----
def _check(got, W, b, x, pad, relu, what):
    got = got.detach().cpu().double().numpy()
    ref = FR.layer(W, b, x, pad, relu)
    bnd = FR.bound(W, b, x, pad)
    frac = float((np.abs(got - ref) / np.maximum(bnd, 1e-300)).max())
    print('%s: worst error / bound %.3g' % (what, frac))
    assert (np.abs(got - ref) <= bnd).all(), (what, frac)
    return frac


@pytest.mark.parametrize('name', sorted(FR.ROUNDING_CASES))
def test_every_entry_is_within_the_bound_of_the_sum_over_rounded_operands(built_lib, name):
    from iterative_inference_segm_amd import ops
    W, b, x, pad = FR.rounding_case(name)
    if W.shape[2] == 3 and pad == 1:
        got = _layer(W.astype(np.float32), b.astype(np.float32), pad, relu=False)(_dev(x))
    else:
        got = ops.conv_fwd_kxk(_dev(x), _dev(W), _dev(b), relu=False)
    _check(got, W, b, x, pad, False, name)


def _run(K, pad, W, x):
    from iterative_inference_segm_amd import ops
    if K == 3:
        return _layer(W, None, pad, relu=False)(_dev(x))
    return ops.conv_fwd_kxk(_dev(x), _dev(W), None, relu=False)


@pytest.mark.parametrize('K,pad,tap', [(1, 0, (0, 0)), (7, 0, (3, 4)), (3, 1, (1, 1)), (3, 1, (0, 2))])
def test_ties_and_direction_through_each_operand(built_lib, K, pad, tap):
    vals = FR.TIES
    n = len(vals)
    want = torch.from_numpy(vals).to(torch.bfloat16).to(torch.float64).numpy()    # torch's CPU cast: nearest even
    assert np.array_equal(want, FR.bf16(vals)) and not np.array_equal(want, vals.astype(np.float64))
    h = w = K + 1
    eye = np.zeros((n, n, K, K), np.float32)
    eye[np.arange(n), np.arange(n), tap[0], tap[1]] = 1.0
    # through x: channel c holds value c everywhere, the filter passes the tap of channel c on
    x = np.broadcast_to(vals[None, :, None, None], (2, n, h, w)).astype(np.float32)
    got = _run(K, pad, eye, x).cpu().double().numpy()
    inner = got[:, :, 1:-1, 1:-1] if pad else got                # away from the zero border
    assert inner.size and np.array_equal(inner, np.broadcast_to(want[None, :, None, None], inner.shape))
    # through W: the tap of channel c holds value c, x is one
    Wv = eye * vals[:, None, None, None]
    got = _run(K, pad, Wv, np.ones((2, n, h, w), np.float32)).cpu().double().numpy()
    inner = got[:, :, 1:-1, 1:-1] if pad else got
    assert np.array_equal(inner, np.broadcast_to(want[None, :, None, None], inner.shape))


# ---- 4. several slabs: the same bits twice ----
def test_the_same_inputs_give_the_same_bits_twice_with_several_slabs(built_lib):
    from iterative_inference_segm_amd import _lib, ops
    lib = _lib.load()
    rng = np.random.default_rng(5)
    worst = []
    for K, Cin, Cout, h, w in ((7, 130, 65, 13, 13), (1, 200, 33, 37, 150)):
        x = rng.standard_normal((3, Cin, h, w)).astype(np.float32)
        W = (0.1 * rng.standard_normal((Cout, Cin, K, K))).astype(np.float32)
        b = rng.standard_normal(Cout).astype(np.float32)
        d = ops.conv_fwd_kxk_desc(x.shape, W.shape)
        assert lib.iiseg_conv_fwd_kxk_bf16_slabs(C.byref(d)) >= 2
        xd, Wd, bd = _dev(x), _dev(W), _dev(b)
        outs = [ops.conv_fwd_kxk(xd, Wd, bd).cpu() for _ in range(2)]
        assert torch.equal(outs[0], outs[1])
        worst.append(_check(outs[0], W, b, x, 0, True, '%d -> %d at %dx%d, K = %d' % (Cin, Cout, h, w, K)))
    print('several slabs: worst error / bound %s' % worst)


# ---- 5. the module ----
GEOMS = {'26x30': (3, 26, 30), '64x58': (2, 64, 58)}
_FCN = {}


def _fcn_case(geom):
    if ('case', geom) not in _FCN:
        _FCN[('case', geom)] = RF.make_case(*GEOMS[geom], seed=5)
    return _FCN[('case', geom)]


def _fcn8(geom, params=None, **modes):
    from iterative_inference_segm_amd.fcn8 import FCN8
    return FCN8(params if params is not None else _fcn_case(geom)[0], RF.SMALL['n_classes'], layer=['score'],
                dtype=F32, mma='f32', trainable=True, **modes)


def _fcn_runs(geom):
    """forward_train / backward of a module built without the keyword, with fwd='f32' and with fwd='bf16' on one
    case with the same dropout masks, once."""
    if ('runs', geom) in _FCN:
        return _FCN[('runs', geom)]
    from iterative_inference_segm_amd import ops
    params, x, T, k6, k7 = _fcn_case(geom)
    xd, Td, k6d, k7d = _dev(x), _dev(T), _dev(k6), _dev(k7)
    out = {}
    for key, modes in (('none', {}), ('f32', {'fwd': 'f32'}), ('bf16', {'fwd': 'bf16'})):
        net = _fcn8(geom, **modes)
        assert net.fwd == ('bf16' if key == 'bf16' else 'f32') and net.wgrad == net.dgrad == net.kxk == 'f32'
        score = net.forward_train(xd, k6d, k7d)
        _, g, _ = ops.ctx_loss(score, Td, ('crossentropy',), 1.0)
        grads = net.backward(g)
        torch.cuda.synchronize()
        out[key] = dict(net=net, score=score.clone(),
                        saved={k: (v.clone() if torch.is_tensor(v) else v) for k, v in net.saved_maps().items()},
                        grads={n: (a.clone(), b.clone()) for n, (a, b) in grads.items()})
    _FCN[('runs', geom)] = out
    return out


@pytest.mark.parametrize('geom', list(GEOMS))
def test_fwd_f32_is_the_module_without_the_keyword(built_lib, geom):
    runs = _fcn_runs(geom)
    a, b = runs['none'], runs['f32']
    assert sorted(a['saved']) == sorted(b['saved'])
    for k, v in a['saved'].items():
        if torch.is_tensor(v):
            assert torch.equal(v, b['saved'][k]), k
    for n in a['grads']:
        assert torch.equal(a['grads'][n][0], b['grads'][n][0]) and torch.equal(a['grads'][n][1], b['grads'][n][1]), n
    assert all(not c.fwd16 for c in b['net'].convs.values())
    assert sorted(n for n, c in runs['bf16']['net'].convs.items() if c.fwd16) == sorted(FR.LAYERS)


@pytest.mark.parametrize('geom', list(GEOMS))
def test_fwd_bf16_every_layer_meets_its_bound_on_its_own_saved_input(built_lib, geom):
    from iterative_inference_segm_amd import ops
    params = _fcn_case(geom)[0]
    runs = _fcn_runs(geom)
    s, net = runs['bf16']['saved'], runs['bf16']['net']
    inputs = {n: 'in_' + n for n in FR.LAYERS}
    inputs['fc7'] = 'drop6'
    worst = {}
    for name in FR.LAYERS:
        W, b = params[name]
        worst[name] = _check(s[name], W, b, s[inputs[name]].cpu().double().numpy(), FR.pad_of(name), True,
                             '%s %s' % (geom, name))
        assert not torch.equal(s[name], runs['f32']['saved'][name]), name       # the mode did run
    print('FCN-8 fwd bf16 (%s), teacher-forced: worst error / bound per layer %s'
          % (geom, {n: '%.3g' % v for n, v in worst.items()}))
    # the pools are maxpool2x2 of the fp32 maps this forward stored
    for bi, names in enumerate(RF.BLOCKS):
        assert torch.equal(s['pool%d' % (bi + 1)], ops.maxpool2x2(s[names[-1]])), bi
    # the score layers: the fp32 layers' output on the inputs this forward saved
    f32 = runs['f32']['net']
    assert torch.equal(f32.convs['score_fr'](s['drop7']), s['score_fr'])
    for sname, pool in (('score_pool4', 'pool4'), ('score_pool3', 'pool3')):
        assert torch.equal(f32.convs[sname](s[pool], window=s['win_' + sname]), s[sname]), sname
    assert net.convs['score_fr']._W16 is None and not net.convs['score_fr'].fwd16


def _np(grads):
    return {n: tuple(a.detach().cpu().double().numpy() for a in v) for n, v in grads.items()}


@pytest.mark.parametrize('geom', list(GEOMS))
def test_fcn8_chain_error_is_the_restatements(built_lib, geom):
    """1 - cosine per gradient array between fwd='bf16' and fwd='f32', on the GPU and in the float64 restatement
    with the same rounding points; the figures of both geometries are in DESIGN.md section 18."""
    params, x, T, k6, k7 = _fcn_case(geom)
    runs = _fcn_runs(geom)
    ref = {}
    for key, rounded in (('f32', False), ('bf16', True)):
        s = FR.forward(params, x, k6, k7, rounded=rounded)
        g = RF.loss_and_grad(s['score'], T)[3]
        ref[key] = RF.backward(params, s, g)
    cg = FR.cosines(_np(runs['bf16']['grads']), _np(runs['f32']['grads']))
    cr = FR.cosines(ref['bf16'], ref['f32'])
    fmt = lambda cos: {n: '%.3g' % (1 - c) for n, c in cos.items()}
    print('FCN-8 (%s) fwd bf16 against f32, 1 - cosine per array: on the GPU %s; float64 restatement with the rounding '
          'points %s' % (geom, fmt(cg), fmt(cr)))
    for n in cg:
        # (the factor 2: near-tie decisions that fall differently under fp32 and float64 accumulation)
        assert 1 - cg[n] <= 2 * (1 - cr[n]) + 1e-6, (geom, n, 1 - cg[n], 1 - cr[n])


# ---- 6. a step, then refresh() ----
def _trainer(geom, modes, params=None, **kw):
    from iterative_inference_segm_amd.train import FCN8Trainer
    C_ = RF.SMALL['n_classes']
    return FCN8Trainer(_fcn8(geom, params, **modes), C_, [C_], **kw)


ALL16 = dict(fwd='bf16', wgrad='bf16', dgrad='bf16', kxk='bf16')


@pytest.mark.parametrize('modes', [dict(fwd='bf16'), ALL16], ids=['fwd', 'all'])
def test_a_step_then_refresh_leaves_a_module_equal_to_a_fresh_one(built_lib, modes):
    params, x, T, k6, k7 = _fcn_case('26x30')
    xd, Td, k6d, k7d = _dev(x), _dev(T), _dev(k6), _dev(k7)
    kw = dict(learning_rate=1e-2, weight_decay=1e-4)
    tr = _trainer('26x30', modes, **kw)
    before = tr.net.flat.clone()
    tr.train_step(xd, Td, k6d, k7d)                              # packs the images, steps, refresh()
    assert not torch.equal(before, tr.net.flat)
    names3 = FR.LAYERS[:13]
    ptrs = {n: tr.net.convs[n]._W16.data_ptr() for n in names3}
    fresh = _trainer('26x30', modes, params=tr.net.state_arrays(), **kw)
    assert torch.equal(fresh.net.flat, tr.net.flat)
    saved = []
    for t in (tr, fresh):
        t.net.forward_train(xd, k6d, k7d)
        torch.cuda.synchronize()
        saved.append({k: v.clone() for k, v in t.net.saved_maps().items() if torch.is_tensor(v)})
    assert sorted(saved[0]) == sorted(saved[1])
    for k in saved[0]:
        assert torch.equal(saved[0][k], saved[1][k]), k
    assert {n: tr.net.convs[n]._W16.data_ptr() for n in names3} == ptrs          # the buffers they had


# ---- 7. training ----
def test_loss_goes_down_over_40_steps_with_all_four_bf16_modes(built_lib):
    x, T = _fcn_case('26x30')[1:3]
    tr = _trainer('26x30', ALL16, learning_rate=1e-3, seed=2)
    xd, Td = _dev(x), _dev(T)
    losses = [tr.train_step(xd, Td) for _ in range(40)]
    losses = [float(v) for v in torch.stack(losses).cpu()]
    print('FCN-8 loss, fwd, wgrad, dgrad and kxk bf16, steps 0-9: %.5f, steps 30-39: %.5f'
          % (np.mean(losses[:10]), np.mean(losses[-10:])))
    assert np.all(np.isfinite(losses))
    assert np.mean(losses[-10:]) < np.mean(losses[:10])


def test_train_fcn8_driver_end_to_end_with_fwd_bf16(built_lib, tmp_path):
    from iterative_inference_segm_amd.fcn8 import buildFCN8
    save = str(tmp_path / 'save')
    # two epochs: the driver's first epoch only sets the best validation score and writes no checkpoint
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_fcn8.py'), '--synthetic', '-ne', '2',
                        '--n_images', '2', '--image_size', '26', '30', '-batch_size', '[2, 2, 2]', '--savepath', save,
                        '--width_div', '16', '--fc_channels', '32', '--max_batches', '1', '-penal_cst', '1e-4',
                        '--fwd', 'bf16'], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert os.listdir(os.path.join(save, 'camvid')) == ['fcn8_data_aug']     # the fp32 run's folder
    folder = os.path.join(save, 'camvid', 'fcn8_data_aug')
    lines = open(os.path.join(folder, 'config.txt')).read().splitlines()
    assert 'fwd = bf16' in lines and 'kxk = f32' in lines and 'wgrad = f32' in lines and 'dgrad = f32' in lines
    models = [f for f in os.listdir(folder) if f in ('new_fcn8_model_best.npz', 'new_fcn8_model_last.npz')]
    assert models
    net = buildFCN8(3, path_weights=os.path.join(folder, models[0]), n_classes=11)
    x = _dev(np.random.default_rng(1).random((2, 3, 26, 30)))
    probs = net(x)[0]
    assert tuple(probs.shape) == (2, 11, 26, 30) and bool(torch.isfinite(probs).all())
