"""GPU: the standard DAE's forward on the 16-bit matrix pipe (fwd='bf16'; conv_halo_bf16_kernel through
ops.Conv(fwd16=True), with the k-tile that straddles the two sources of a concat layer).
The kernel: two-source layers exact on data bf16 holds exactly, with tails on both sides of a k-tile and of the
channel block, several column tiles and tiles that span images; the aligned layer bit-equal to the instantiation it
had; every fused form of a single-source layer exact; the same bits twice.  The module: fwd='f32' is the module without
the keyword bit for bit; with fwd='bf16' every layer meets its bound on the GPU's own saved input (teacher-forced: no
ReLU, pool or DePool2D decision enters a comparison), the fused pools are the pool kernel's, and the chain's cosine to
the fp32 gradients is that of the float64 restatement with the same rounding points (tests/std_fwd_bf16_ref.py).
Sessions, refresh(), training and the driver run in the mode.

Measured on an MI355X (for the record; the assertions are the derived bounds): see DESIGN.md section 20."""
import os

import numpy as np
import pytest
import torch

import std_fwd_bf16_ref as FR
import std_train_ref as R
from oracle import nn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = torch.float32


def _dev(a, dt=F32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda().contiguous()


def _iconv(x, W, b=None, pad=0, relu=True):
    """The 3x3 layer on integer arrays, in int64."""
    x, W = x.astype(np.int64), W.astype(np.int64)
    if pad:
        x = np.pad(x, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    OH, OW = x.shape[2] - 2, x.shape[3] - 2
    out = np.zeros((x.shape[0], W.shape[0], OH, OW), dtype=np.int64)
    for ky in range(3):
        for kx in range(3):
            out += np.einsum('oi,bihw->bohw', W[:, :, ky, kx], x[:, :, ky:ky + OH, kx:kx + OW])
    if b is not None:
        out += b.astype(np.int64)[None, :, None, None]
    return np.maximum(out, 0) if relu else out


def _layer(W, b, pad, relu=True, **kw):
    from iterative_inference_segm_amd import ops
    kw = dict(dict(mma='f32', fwd16=True), **kw)
    return ops.Conv(np.asarray(W, np.float32), None if b is None else np.asarray(b, np.float32), pad=pad, relu=relu,
                    device='cuda', dtype=F32, **kw)


# ---- 1. two sources: exact on small integers ----
# C1 = 3, 17, 24: the k-tile that holds channel C1 takes channels of both sources (a tail of x1 of 3, 1 and 8 channels
# in front of x2); C1 = 16: the aligned layer.  C2 = 4, 13, 16 end the last k-tile early, or not.  Cout = 11, 33, 70:
# tails on both sides of the 32- / 64-channel block, and a second block.  Maps: one tile; two column tiles; 5 row
# tiles x 3 column tiles (with B = 3 a workgroup id's tiles span images).
SOURCES = [(c1, c2) for c1 in (3, 16, 17, 24) for c2 in (4, 13, 16)]
COUTS = (11, 33, 70)
MAPS = ((5, 4), (9, 33), (37, 70))


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('C1,C2', SOURCES)
def test_two_source_layers_are_exact_on_integers(built_lib, C1, C2, B):
    for Cout in COUTS:
        rng = np.random.default_rng(C1 * 1000 + C2 * 10 + Cout + 7 * B)
        W = rng.integers(-2, 3, size=(Cout, C1 + C2, 3, 3))
        b = rng.integers(-3, 4, size=(Cout,))
        conv = _layer(W, b, 1)
        for h, w in MAPS:
            x1 = rng.integers(-2, 3, size=(B, C1, h, w))
            x2 = rng.integers(-2, 3, size=(B, C2, h, w))
            want = _iconv(np.concatenate([x1, x2], axis=1), W, b, pad=1)
            assert np.abs(want).max() < 2 ** 24 and want.max() > 0
            out = torch.full((B, Cout, h, w), float('nan'), dtype=F32, device='cuda')
            assert conv(_dev(x1), x2=_dev(x2), out=out) is out           # every entry is written: no NaN survives
            assert np.array_equal(out.cpu().numpy(), want.astype(np.float64)), (Cout, h, w)
        assert conv._W16 is not None and conv._packs == {}               # the bf16 kernel ran, no fp32 pack was made


def test_the_aligned_layer_is_bit_equal_to_the_instantiation_it_had(built_lib):
    """16 + 16 channels of real data: a fwd16 layer, and the same layer the way a mma='bf16' module launches it
    (iiseg_conv_halo_bf16, which refuses every straddling layer)."""
    rng = np.random.default_rng(3)
    W, b = rng.standard_normal((33, 32, 3, 3)), rng.standard_normal(33)
    x1, x2 = _dev(rng.standard_normal((3, 16, 37, 70))), _dev(rng.standard_normal((3, 16, 37, 70)))
    new, old = _layer(W, b, 1), _layer(W, b, 1, mma='bf16', fwd16=False)
    assert old._form(old._describe_call(x1, x2)) == new._form(new._describe_call(x1, x2)) == 'halo_bf16'
    assert torch.equal(new(x1, x2=x2), old(x1, x2=x2))


@pytest.mark.parametrize('C1,C2', [(3, 4), (17, 13), (24, 16)])
def test_a_straddling_layer_is_bit_equal_to_the_layer_on_the_concatenated_map(built_lib, C1, C2):
    """Real data: the k-tiles hold the same channels in the same places either way, so the fp32 sums are the same."""
    rng = np.random.default_rng(C1)
    conv = _layer(rng.standard_normal((70, C1 + C2, 3, 3)), rng.standard_normal(70), 1)
    x1, x2 = _dev(rng.standard_normal((3, C1, 37, 70))), _dev(rng.standard_normal((3, C2, 37, 70)))
    two = [conv(x1, x2=x2).clone() for _ in range(2)]
    assert torch.equal(two[0], two[1])                                   # the same bits from two runs
    assert torch.equal(two[0], conv(torch.cat([x1, x2], dim=1).contiguous()))
    assert bool(torch.isfinite(two[0]).all()) and float(two[0].abs().max()) > 0


# ---- 2. single-source layers under fwd16, each fused form exact on integers ----
def test_the_pad_100_layer_is_exact(built_lib):
    rng = np.random.default_rng(100)
    x, W, b = rng.integers(-2, 3, size=(2, 3, 8, 6)), rng.integers(-2, 3, size=(64, 3, 3, 3)), rng.integers(-3, 4, 64)
    got = _layer(W, b, 100)(_dev(x))
    assert np.array_equal(got.cpu().numpy(), _iconv(x, W, b, pad=100).astype(np.float64))


def _mask_bytes(pre, pooled):
    """bit (y & 1) * 2 + (x & 1) of a window's byte: pre == pooled"""
    h2, w2 = pooled.shape[2:]
    eq = (pre[:, :, :2 * h2, :2 * w2] == np.repeat(np.repeat(pooled, 2, 2), 2, 3)).astype(np.uint8)
    return eq[:, :, 0::2, 0::2] | (eq[:, :, 0::2, 1::2] << 1) | (eq[:, :, 1::2, 0::2] << 2) | (eq[:, :, 1::2, 1::2] << 3)


@pytest.mark.parametrize('h,w', [(9, 33), (8, 34), (37, 70)])
@pytest.mark.parametrize('Cin,Cout', [(17, 33), (4, 70)])
def test_the_fused_pool_is_exact_at_odd_and_even_sizes(built_lib, Cin, Cout, h, w):
    rng = np.random.default_rng(Cin + h)
    x, W, b = rng.integers(-2, 3, size=(2, Cin, h, w)), rng.integers(-2, 3, size=(Cout, Cin, 3, 3)), \
        rng.integers(-3, 4, Cout)
    pre = _iconv(x, W, b, pad=1).astype(np.float64)
    pooled = nn.maxpool2(pre)
    conv = _layer(W, b, 1)
    pool = torch.full((2, Cout, h // 2, w // 2), float('nan'), dtype=F32, device='cuda')
    out = conv(_dev(x), pool_out=pool)
    assert np.array_equal(out.cpu().numpy(), pre) and np.array_equal(pool.cpu().numpy(), pooled)
    # outside keep_pre: pool + mask bytes, the pre-pool map is not stored
    pool2 = torch.full_like(pool, float('nan'))
    mask = torch.full(tuple(pool.shape), 255, dtype=torch.uint8, device='cuda')
    assert conv(_dev(x), pool_out=pool2, mask_out=mask, store_out=False) is None
    assert torch.equal(pool2, pool) and np.array_equal(mask.cpu().numpy(), _mask_bytes(pre, pooled))


@pytest.mark.parametrize('masked', [False, True], ids=['pre_pooled', 'mask_in'])
@pytest.mark.parametrize('Cin,Cout', [(17, 33), (70, 11)])
def test_the_fused_unpool_with_addend_crop_and_window_is_exact(built_lib, Cin, Cout, masked):
    rng = np.random.default_rng(Cin + Cout)
    B, H, Wd = 2, 19, 37                                         # odd: a trailing row and column without a window
    pre = rng.integers(-2, 3, size=(B, Cin, H, Wd)).astype(np.float64)
    pooled = nn.maxpool2(pre)
    up = rng.integers(-2, 3, size=pooled.shape).astype(np.float64)
    W, b = rng.integers(-2, 3, size=(Cout, Cin, 3, 3)), rng.integers(-3, 4, Cout)
    z = _iconv(nn.depool_eqmask(up, pre, pooled), W, b, pad=1, relu=False)
    other = rng.integers(-5, 6, size=(B, Cout, 15, 40))
    # the window (3, 2, 13, 34) of the conv's map + `other` from (1, 4), placed at (2, 1) of a 16 x 36 map
    oy, ox, OH, OW = 3, 2, 13, 34
    want = z[:, :, oy:oy + OH, ox:ox + OW] + other[:, :, 1:1 + OH, 4:4 + OW]
    out = torch.full((B, Cout, 16, 36), -7.0, dtype=F32, device='cuda')
    conv = _layer(W, b, 1, relu=False)
    kw = dict(pre=_dev(pre), pooled=_dev(pooled))
    if masked:
        kw = dict(mask_in=_dev(_mask_bytes(pre, pooled), torch.uint8), unpool_hw=(H, Wd))
    conv(_dev(up), add=_dev(other), add_off=(1, 4), window=(oy, ox, OH, OW), out=out, place=(2, 1), **kw)
    full = np.full((B, Cout, 16, 36), -7.0)
    full[:, :, 2:2 + OH, 1:1 + OW] = want
    assert np.array_equal(out.cpu().numpy(), full)


# ---- 3. the module ----
MODELS = {'small': R.SMALL, 'second': R.SECOND}
_CASES, _RUNS = {}, {}


def _model_case(which):
    """(params, [h], y, T): float32 values held in float64 arrays (what the GPU is handed is what the restatement
    reads); computed once, shared, never changed."""
    if which not in _CASES:
        f = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)
        params, hs, y, T = R.make_case(MODELS[which])
        _CASES[which] = ({n: tuple(f(a) for a in v) for n, v in params.items()}, [f(h) for h in hs], f(y), f(T))
    return _CASES[which]


def _std_dae(which, params=None, **modes):
    from iterative_inference_segm_amd.dae import StandardDAE
    return StandardDAE(params if params is not None else _model_case(which)[0], MODELS[which][0], device='cuda',
                       dtype=F32, mma='f32', trainable=True, **modes, **MODELS[which][3])


def _runs(which):
    """forward_train / backward of a module built without the keyword, with fwd='f32' and with fwd='bf16', once."""
    if which in _RUNS:
        return _RUNS[which]
    from iterative_inference_segm_amd import ops
    params, hs, y, T = _model_case(which)
    hd, yd, Td = [_dev(h) for h in hs], _dev(y), _dev(T)
    out = {}
    for key, modes in (('none', {}), ('f32', {'fwd': 'f32'}), ('bf16', {'fwd': 'bf16'})):
        dae = _std_dae(which, **modes)
        assert dae.fwd == ('bf16' if key == 'bf16' else 'f32') and dae.wgrad == dae.dgrad == 'f32'
        score = dae.forward_train(hd, yd)
        _, g, _ = ops.ctx_loss(score, Td, ('crossentropy',), 1.0)
        grads = dae.backward(g)
        torch.cuda.synchronize()
        out[key] = dict(dae=dae, score=score.clone(), saved={k: v.clone() for k, v in dae.saved_maps().items()},
                        grads={n: (a.clone(), b.clone()) for n, (a, b) in grads.items()})
    _RUNS[which] = out
    return out


@pytest.mark.parametrize('which', list(MODELS))
def test_fwd_f32_is_the_module_without_the_keyword(built_lib, which):
    runs = _runs(which)
    a, b = runs['none'], runs['f32']
    assert sorted(a['saved']) == sorted(b['saved'])
    for k, v in a['saved'].items():
        assert torch.equal(v, b['saved'][k]), k
    assert torch.equal(a['score'], b['score'])
    for n in a['grads']:
        assert torch.equal(a['grads'][n][0], b['grads'][n][0]) and torch.equal(a['grads'][n][1], b['grads'][n][1]), n
    for key in ('none', 'f32'):
        convs = runs[key]['dae'].conv_layers()
        assert all(not c.fwd16 and c._W16 is None and c._packs for c in convs.values())
    convs = runs['bf16']['dae'].conv_layers()
    assert sorted(convs) == sorted(R.order_of(MODELS[which][3]))
    # every layer of the mode ran the bf16 kernel and built no fp32 pack
    assert all(c.fwd16 and c._W16 is not None and c._packs == {} for c in convs.values())


@pytest.mark.parametrize('which', list(MODELS))
def test_fwd_bf16_every_layer_meets_its_bound_on_its_own_saved_input(built_lib, which):
    from iterative_inference_segm_amd import ops
    params, hs = _model_case(which)[:2]
    cfg = MODELS[which][3]
    runs = _runs(which)
    s = runs['bf16']['saved']
    s64 = {k: v.cpu().double().numpy() for k, v in s.items()}
    worst = {}
    for name, (x, pad, relu, other, out) in FR.layer_calls(s64, hs, cfg).items():
        W, b = params[name]
        assert W.shape[1] == x.shape[1]                          # n = 9 (C1 + C2)
        ref, bnd = FR.layer(W, b, x, pad, relu, other), FR.bound(W, b, x, pad, other)
        err = np.abs(s64[out] - ref)
        worst[name] = float((err / np.maximum(bnd, 1e-300)).max())
        print('%s %s: worst error / bound %.3g' % (which, name, worst[name]))
        assert (err <= bnd).all(), (which, name, worst[name])
        assert not torch.equal(s[out], runs['f32']['saved'][out]), name          # the mode did run
    print('standard DAE fwd bf16 (%s), teacher-forced: worst error / bound per layer %s'
          % (which, {n: '%.3g' % v for n, v in worst.items()}))
    # every pooled map -- fused into the conv's epilogue or not -- is the pool kernel's on the stored pre-pool map
    total = len(worst) // 2
    for p in range(1, total + 1):
        assert torch.equal(s['pool%d' % p], ops.maxpool2x2(s['pre%d' % p])), p
    assert torch.equal(runs['bf16']['score'], s['fused_up1'])


def _np(grads):
    return {n: tuple(a.detach().cpu().double().numpy() for a in v) for n, v in grads.items()}


@pytest.mark.parametrize('which', list(MODELS))
def test_chain_error_is_the_restatements(built_lib, which):
    """1 - cosine per gradient array between fwd='bf16' and fwd='f32', on the GPU and in the float64 restatement
    with the same rounding points; the figures of both models are in DESIGN.md section 20."""
    params, hs, y, T = _model_case(which)
    cfg = MODELS[which][3]
    runs = _runs(which)
    ref = {key: FR.loss_and_param_grads(params, hs, y, T, cfg, rounded=rounded)[1]
           for key, rounded in (('f32', False), ('bf16', True))}
    cg = FR.cosines(_np(runs['bf16']['grads']), _np(runs['f32']['grads']))
    cr = FR.cosines(ref['bf16'], ref['f32'])
    fmt = lambda cos: {n: '%.3g' % (1 - c) for n, c in cos.items()}
    print('standard DAE (%s) fwd bf16 against f32, 1 - cosine per array: on the GPU %s; float64 restatement with the '
          'rounding points %s' % (which, fmt(cg), fmt(cr)))
    for n in cg:
        # (the factor 2: near-tie decisions that fall differently under fp32 and float64 accumulation)
        assert 1 - cg[n] <= 2 * (1 - cr[n]) + 1e-6, (which, n, 1 - cg[n], 1 - cr[n])


@pytest.mark.parametrize('which', list(MODELS))
def test_scores_without_a_session_equals_a_primed_sessions_second_call(built_lib, which):
    hs, y = _model_case(which)[1:3]
    hd, yd = [_dev(h) for h in hs], _dev(y)
    dae = _std_dae(which, fwd='bf16')
    eager = dae.scores(hd, yd).clone()
    session = dae.new_session(hd, yd)
    first = dae.scores(hd, yd, session=session).clone()
    assert session['primed']
    second = dae.scores(hd, yd, session=session)
    assert torch.equal(eager, first) and torch.equal(eager, second)
    assert all(c._packs == {} for c in dae.conv_layers().values())
    # and it is the mode's forward: the training forward (full maps, pre-pool maps kept) gives the same scores
    assert torch.equal(eager, dae.forward_train(hd, yd))
    r = dae(*hd, yd)
    assert tuple(r.shape) == tuple(yd.shape) and bool(torch.isfinite(r).all())


# ---- 4. a step, then refresh() ----
ALL16 = dict(fwd='bf16', wgrad='bf16', dgrad='bf16')


def _trainer(modes, params=None, noise=0.1, seed=1, **kw):
    from iterative_inference_segm_amd.train import DAETrainer
    return DAETrainer(None, _std_dae('second', params, **modes), 11, [11], noise=noise, seed=seed, **kw)


@pytest.mark.parametrize('modes', [dict(fwd='bf16'), ALL16], ids=['fwd', 'all'])
def test_a_step_then_refresh_leaves_a_module_equal_to_a_fresh_one(built_lib, modes):
    _, hs, y, T = _model_case('second')
    hd, yd, Td = [_dev(h) for h in hs], _dev(y), _dev(T)
    tr = _trainer(modes, learning_rate=1e-2)
    before = tr.dae.flat.clone()
    tr.train_step(hd, yd, Td)                                    # packs the images, steps, refresh()
    assert not torch.equal(before, tr.dae.flat)
    ptrs = {n: c._W16.data_ptr() for n, c in tr.dae.conv_layers().items()}
    fresh = _trainer(modes, params=tr.dae.state_arrays(), learning_rate=1e-2)
    assert torch.equal(fresh.dae.flat, tr.dae.flat)
    saved = []
    for t in (tr, fresh):
        t.dae.forward_train(hd, yd)
        torch.cuda.synchronize()
        saved.append({k: v.clone() for k, v in t.dae.saved_maps().items()})
    assert sorted(saved[0]) == sorted(saved[1])
    for k in saved[0]:
        assert torch.equal(saved[0][k], saved[1][k]), k
    assert {n: c._W16.data_ptr() for n, c in tr.dae.conv_layers().items()} == ptrs       # the buffers they had
    assert all(c._packs == {} for c in tr.dae.conv_layers().values())


# ---- 5. training ----
def test_loss_goes_down_over_40_steps_with_all_three_bf16_modes(built_lib):
    """The loop of tests/test_gpu_std_train.py::test_loss_goes_down_over_40_steps_f32: the same case, seed and
    learning rate."""
    params, hs, _, T = R.make_case(R.SECOND)
    tr = _trainer(ALL16, params=params, seed=2, learning_rate=1e-4)
    hd, Td = [_dev(h) for h in hs], _dev(T)
    yd = Td[:, :11].contiguous()                                 # from_gt
    losses = [tr.train_step(hd, yd, Td) for _ in range(40)]
    losses = [float(v) for v in torch.stack(losses).cpu()]
    print('standard DAE loss, fwd, wgrad and dgrad bf16, steps 0-9: %.5f, steps 30-39: %.5f'
          % (np.mean(losses[:10]), np.mean(losses[-10:])))
    assert np.all(np.isfinite(losses))
    assert np.mean(losses[-10:]) < np.mean(losses[:10])


def test_train_dae_end_to_end_with_fwd_bf16(built_lib, tmp_path):
    import sys
    from iterative_inference_segm_amd.dae import buildDAE
    sys.path.insert(0, ROOT)
    try:
        import train_dae
    finally:
        sys.path.remove(ROOT)
    save, load = str(tmp_path / 'save'), str(tmp_path / 'load')
    dd = {'kind': 'standard', 'dropout': 0, 'skip': True, 'unpool_type': 'trackind', 'noise': 0.1,
          'concat_h': ['pool2'], 'from_gt': True, 'n_filters': 8, 'conv_before_pool': 1, 'additional_pool': 2,
          'temperature': 1.0, 'path_weights': '', 'layer': 'probs_dimshuffle', 'exp_name': 't_', 'bn': 0}
    # 26 x 26: the smallest image whose pad-100 map (224 x 224) leaves fc6 of the frozen FCN-8 its 7 x 7 input
    res = train_dae.train('camvid', 'fcn8', learning_rate=1e-4, num_epochs=2, batch_size=[2, 2, 2],
                          dae_dict_updates=dd, training_loss=['crossentropy'], savepath=save, loadpath=load,
                          synthetic=True, n_images=2, image_size=(26, 26), fwd='bf16', verbose=False)
    assert len(res['err_train']) == 2 and np.all(np.isfinite(res['err_train'] + res['err_valid']))
    exp, = os.listdir(os.path.join(save, 'camvid'))
    assert 'bf16' not in exp                                     # the fp32 run's folder
    folder = os.path.join(load, 'camvid', exp)
    lines = open(os.path.join(folder, 'config.txt')).read().splitlines()
    assert 'fwd = bf16' in lines and 'wgrad = f32' in lines and 'dgrad = f32' in lines
    assert os.path.exists(os.path.join(folder, 'dae_model_best.npz'))
    dae = buildDAE(n_classes=11, concat_h=dd['concat_h'], n_filters=8, additional_pool=2, skip=True,
                   unpool_type='trackind', path_weights=folder, model_name='dae_model_best.npz', load_weights=True)
    assert dae.enc['conv3_1'].Cin == 16 + 128                    # h: pool2 of the FCN-8
    assert all(bool(torch.isfinite(c.W).all()) for c in dae.conv_layers().values())
