"""GPU: the 16-bit weight-gradient mode (wgrad='bf16'; csrc/conv_wgrad_bf16.hip).  The kernel:
exact on data bf16 holds exactly; on real data within the any-order fp32 accumulation bound of the float64 sum over
operands rounded on the CPU with .to(torch.bfloat16), ties and direction included, db from the unrounded g_z, the
same bits twice.  The modules: nothing but the 3x3 weight gradients changes between wgrad='f32' and 'bf16', every
ops.conv_wgrad call of `backward` carries the mode and meets the bound on its own operands.  Training and the two
drivers run in the mode.

Measured on an MI355X (for the record; the assertions are the derived bounds): see DESIGN.md section 15."""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import fcn8_train_ref as RF
import std_train_ref as R
import wgrad_bf16_ref as WR
from wgrad_bf16_ref import F32, U, bound_check as _bound_check, dev as _dev, pad as _pad, taps as _taps

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. exact on small integers ----
CHANNELS = [(11, 64), (24, 16), (64, 130), (130, 33)]            # none a multiple of the 64-channel block
GEOMETRY = [(7, 7, 1), (14, 13, 1), (37, 150, 1), (3, 4, 5), (14, 13, 5), (1, 1, 1), (2, 9, 1)]
# the edges of `wave_on`: a wave multiplies a 32 x 32 sub-block of the 64 x 64 block only if it holds a real channel;
# on three small maps
EDGES = [(32, 32), (33, 33), (65, 65)]
INT_CASES = [(ci, co, b, h, w, p) for h, w, p in GEOMETRY for b in (1, 3) for ci, co in CHANNELS] + \
            [(ci, co, b, h, w, p) for h, w, p in (GEOMETRY[0], GEOMETRY[1], GEOMETRY[3]) for b in (1, 3)
             for ci, co in EDGES]


def _int_case(Cin, Cout, B, H, W, pad):
    return WR.int_case(Cin, Cout, B, H, W, pad, np.int64)


@pytest.mark.parametrize('Cin,Cout,B,H,W,pad', INT_CASES)
def test_bf16_weight_gradient_is_exact_on_integers(built_lib, Cin, Cout, B, H, W, pad):
    from iterative_inference_segm_amd import _lib, ops
    x, gz, dW_ref, db_ref = _int_case(Cin, Cout, B, H, W, pad)
    xd, gzd = _dev(x), _dev(gz)
    nslab = _lib.load().iiseg_conv_wgrad_bf16_slabs(C.byref(ops.conv_wgrad_desc(x.shape, Cout, pad)))
    if (H, W) == (37, 150):
        assert nslab >= 2                                        # slabs + the finalize launch
    if (H, W) == (7, 7) and B == 1:
        assert nslab == 1                                        # straight into dW
    # the layer's own array, W[out, in, 3, 3]
    dW = torch.full(dW_ref.shape, 7.0, dtype=F32, device='cuda')
    db = torch.full((Cout,), 7.0, dtype=F32, device='cuda')
    ops.conv_wgrad(xd, gzd, dW, db, pad=pad, mma='bf16')
    # the middle of a wider parameter, in both layouts: the other input channels keep the sentinel; no db
    lo, hi = 3, 5
    big = torch.full((Cout, lo + Cin + hi, 3, 3), -9.0, dtype=F32, device='cuda')
    ops.conv_wgrad(xd, gzd, big, None, pad=pad, ci0=lo, mma='bf16')
    bigT = torch.full((lo + Cin + hi, Cout, 3, 3), -9.0, dtype=F32, device='cuda')
    ops.conv_wgrad(xd, gzd, bigT, None, pad=pad, ci0=lo, layout='iohw', mma='bf16')
    torch.cuda.synchronize()
    assert np.array_equal(dW.cpu().numpy(), dW_ref.astype(np.float64))
    assert np.array_equal(db.cpu().numpy(), db_ref.astype(np.float64))
    want = np.full(tuple(big.shape), -9.0)
    want[:, lo:lo + Cin] = dW_ref
    assert np.array_equal(big.cpu().numpy(), want)
    assert np.array_equal(bigT.cpu().numpy(), want.transpose(1, 0, 2, 3))


# ---- 2. the rounding point ----
def test_operands_are_rounded_to_nearest_once_and_db_is_not(built_lib):
    from iterative_inference_segm_amd import ops
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.standard_normal((1, 24, 7, 7)).astype(np.float32))
    gz = torch.from_numpy(rng.standard_normal((1, 16, 7, 7)).astype(np.float32))
    dW = torch.zeros((16, 24, 3, 3), dtype=F32, device='cuda')
    db = torch.zeros(16, dtype=F32, device='cuda')
    ops.conv_wgrad(x.cuda(), gz.cuda(), dW, db, pad=1, mma='bf16')
    torch.cuda.synchronize()
    frac, ref, mag = _bound_check(dW, x, gz, 1, 'rounding point')
    # (the statement discriminates: against the sum of the UNROUNDED operands the same bound fails)
    exact = _taps(gz.double().numpy(), _pad(x.double().numpy(), 1), 7, 7)
    n = 49
    assert (np.abs(dW.cpu().double().numpy() - exact) > (n + 1) * U * mag).mean() > 0.9
    g64 = gz.double().numpy()
    db_err = np.abs(db.cpu().double().numpy() - g64.sum(axis=(0, 2, 3)))
    db_bound = (n + 1) * U * np.abs(g64).sum(axis=(0, 2, 3))
    print('bf16 wgrad 24 -> 16 at 7x7: worst error / bound %.3g (dW), %.3g (db)' % (frac, (db_err / db_bound).max()))
    assert (db_err <= db_bound).all()


# ---- 3. ties and direction ----
def test_ties_go_to_even_and_negative_values_round_symmetrically(built_lib):
    from iterative_inference_segm_amd import ops
    vals = [1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -10, -(1 + 2.0 ** -8 + 2.0 ** -10),
            1 + 2.0 ** -7 - 2.0 ** -10]
    want = [1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, -(1 + 2.0 ** -7), 1 + 2.0 ** -7]
    v32 = torch.tensor(vals, dtype=F32)
    assert v32.double().tolist() == vals                         # float32 holds them
    assert v32.to(torch.bfloat16).double().tolist() == want      # torch's rounding on the CPU
    # channel c of x holds value c at every pixel; g_z is a single 1.0 at the centre: dW[0, c, ky, kx] = bf16(value c)
    x = v32.view(1, 5, 1, 1).expand(1, 5, 3, 3).contiguous().cuda()
    gz = torch.zeros((1, 1, 3, 3), dtype=F32, device='cuda')
    gz[0, 0, 1, 1] = 1.0
    dW = torch.full((1, 5, 3, 3), 7.0, dtype=F32, device='cuda')
    ops.conv_wgrad(x, gz, dW, None, pad=1, mma='bf16')
    got = dW.cpu().double().numpy()
    for c in range(5):
        assert (got[0, c] == want[c]).all(), (c, got[0, c], want[c])
    # and as the A operand: g_z holds value c in channel c, x is a single 1.0
    gz = v32.view(1, 5, 1, 1).expand(1, 5, 3, 3).contiguous().cuda()
    x = torch.zeros((1, 1, 3, 3), dtype=F32, device='cuda')
    x[0, 0, 1, 1] = 1.0
    dW = torch.full((5, 1, 3, 3), 7.0, dtype=F32, device='cuda')
    ops.conv_wgrad(x, gz, dW, None, pad=1, mma='bf16')
    got = dW.cpu().double().numpy()
    for c in range(5):
        assert (got[c, 0] == want[c]).all(), (c, got[c, 0], want[c])


# ---- 4. several slabs, twice ----
def test_several_slabs_give_the_same_bits_twice_within_both_bounds(built_lib):
    from iterative_inference_segm_amd import ops
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.standard_normal((3, 24, 37, 150)).astype(np.float32))
    gz = torch.from_numpy(rng.standard_normal((3, 16, 37, 150)).astype(np.float32))
    xd, gzd = x.cuda(), gz.cuda()
    runs = []
    for _ in range(2):
        dW = torch.zeros((16, 24, 3, 3), dtype=F32, device='cuda')
        db = torch.zeros(16, dtype=F32, device='cuda')
        ops.conv_wgrad(xd, gzd, dW, db, pad=1, mma='bf16')
        runs.append((dW.cpu(), db.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    n = 3 * 37 * 150
    frac, ref, mag = _bound_check(runs[0][0], x, gz, 1, 'several slabs')
    # against the UNROUNDED operands: each carries a relative 2^-9, so a product (1 + 2^-9)^2 - 1 = 2^-8 + 2^-18 at
    # most, below the 2^-8 + 2^-16 asserted; |a| |b| from the unrounded data
    g64, xp64 = gz.double().numpy(), _pad(x.double().numpy(), 1)
    exact, mag_exact = _taps(g64, xp64, 37, 150), _taps(np.abs(g64), np.abs(xp64), 37, 150)
    err = np.abs(runs[0][0].double().numpy() - exact)
    bound = (2.0 ** -8 + 2.0 ** -16) * mag_exact + (n + 1) * U * mag
    print('bf16 wgrad 3x24x37x150 -> 16: worst error / bound %.3g (rounded operands), %.3g (unrounded operands)'
          % (frac, (err / bound).max()))
    assert (err <= bound).all()
    db_err = np.abs(runs[0][1].double().numpy() - g64.sum(axis=(0, 2, 3)))
    assert (db_err <= (n + 1) * U * np.abs(g64).sum(axis=(0, 2, 3))).all()


# ---- 5. the modules ----
class _Recorder:
    """ops.conv_wgrad, recording every call's operands (copied: the walks reuse their buffers) and target."""

    def __init__(self, ops):
        self.ops, self.inner, self.calls = ops, ops.conv_wgrad, []

    def __call__(self, x, gz, dW, db=None, pad=1, ci0=0, layout='oihw', mma='f32'):
        self.calls.append(dict(x=x.detach().cpu().clone(), gz=gz.detach().cpu().clone(), dW=dW, pad=pad, ci0=ci0,
                               layout=layout, mma=mma))
        return self.inner(x, gz, dW, db, pad=pad, ci0=ci0, layout=layout, mma=mma)

    def __enter__(self):
        self.ops.conv_wgrad = self
        return self

    def __exit__(self, *exc):
        self.ops.conv_wgrad = self.inner


def _check_calls(calls, n_expected, what):
    assert len(calls) == n_expected, (what, len(calls), n_expected)
    worst = 0.0
    for k, c in enumerate(calls):
        assert c['mma'] == 'bf16' and c['layout'] == 'oihw', (what, k, c['mma'], c['layout'])
        Cin = c['x'].shape[1]
        wrote = c['dW'][:, c['ci0']:c['ci0'] + Cin]
        worst = max(worst, _bound_check(wrote, c['x'], c['gz'], c['pad'], '%s call %d' % (what, k))[0])
    return worst


def _cosines(a, b):
    cat = lambda v: torch.cat([t.reshape(-1).double() for t in v])
    return {n: float(cat(a[n]) @ cat(b[n]) / (cat(a[n]).norm() * cat(b[n]).norm())) for n in a}


def _max_rel(a, b, names):
    return max(float((x.double() - y.double()).abs().max() / y.double().abs().max())
               for n in names for x, y in zip(a[n], b[n]))


MODELS = {'small': R.SMALL, 'second': R.SECOND}
_STD = {}


def _std_case(which):
    if which not in _STD:
        _STD[which] = R.make_case(MODELS[which])
    return _STD[which]


def _std_dae(which, wgrad):
    from iterative_inference_segm_amd.dae import StandardDAE
    return StandardDAE(_std_case(which)[0], MODELS[which][0], device='cuda', dtype=F32, mma='f32', trainable=True,
                       wgrad=wgrad, **MODELS[which][3])


@pytest.mark.parametrize('which', ['small', 'second'])
def test_standard_dae_changes_nothing_but_the_weight_gradients(built_lib, which):
    from iterative_inference_segm_amd import ops
    params, hs, y, T = _std_case(which)
    cfg = MODELS[which][3]
    hd, yd, Td = [_dev(h) for h in hs], _dev(y), _dev(T)
    out = {}
    for mode in ('f32', 'bf16'):
        dae = _std_dae(which, mode)
        assert dae.wgrad == mode and dae.mma == 'f32'
        score = dae.forward_train(hd, yd)
        _, g, _ = ops.ctx_loss(score, Td, ('crossentropy',), 1.0)
        with _Recorder(ops) as rec:
            grads = dae.backward(g)
        torch.cuda.synchronize()
        if mode == 'bf16':
            # the 3x3 layers, plus one more call per concat point
            worst = _check_calls(rec.calls, len(R.order_of(cfg)) + len(cfg['concat_h']), 'standard DAE ' + which)
        else:
            assert all(c['mma'] == 'f32' for c in rec.calls)
        out[mode] = dict(score=score.clone(), saved={k: v.clone() for k, v in dae.saved_maps().items()},
                         grads={n: (a.clone(), b.clone()) for n, (a, b) in grads.items()},
                         gy=dae.backward_y(g, yd.shape).clone())
    a, b = out['f32'], out['bf16']
    assert torch.equal(a['score'], b['score']) and torch.equal(a['gy'], b['gy'])
    assert sorted(a['saved']) == sorted(b['saved'])
    for k in a['saved']:
        assert torch.equal(a['saved'][k], b['saved'][k]), k
    assert any(not torch.equal(a['grads'][n][0], b['grads'][n][0]) for n in a['grads'])
    cos = _cosines(b['grads'], a['grads'])
    print('standard DAE (%s) wgrad bf16 against f32: worst error / bound %.3g, max relative difference %.3g, cosine '
          'per layer %s' % (which, worst, _max_rel(b['grads'], a['grads'], list(a['grads'])),
                            {n: '%.6f' % c for n, c in cos.items()}))
    assert all(np.isfinite(c) for c in cos.values())


FCN8_3X3 = [n for names in RF.BLOCKS for n in names]
_FCN = {}


def _fcn_case():
    if not _FCN:
        _FCN['case'] = RF.make_case(3, 26, 30, seed=5)
    return _FCN['case']


def _fcn8(wgrad, params=None, **kw):
    from iterative_inference_segm_amd.fcn8 import FCN8
    return FCN8(params if params is not None else _fcn_case()[0], RF.SMALL['n_classes'], layer=['score'], dtype=F32,
                mma='f32', trainable=True, wgrad=wgrad, **kw)


def test_fcn8_changes_nothing_but_the_thirteen_3x3_weight_gradients(built_lib):
    from iterative_inference_segm_amd import ops
    params, x, T, k6, k7 = _fcn_case()
    xd, Td, k6d, k7d = _dev(x), _dev(T), _dev(k6), _dev(k7)
    out = {}
    assert len(FCN8_3X3) == 13
    for mode in ('f32', 'bf16'):
        net = _fcn8(mode)
        assert net.wgrad == mode
        score = net.forward_train(xd, k6d, k7d)
        _, g, _ = ops.ctx_loss(score, Td, ('crossentropy',), 1.0)
        with _Recorder(ops) as rec:
            grads = net.backward(g)
        torch.cuda.synchronize()
        if mode == 'bf16':
            worst = _check_calls(rec.calls, 13, 'FCN-8')
        else:
            assert all(c['mma'] == 'f32' for c in rec.calls)
        out[mode] = dict(score=score.clone(),
                         saved={k: v.clone() for k, v in net.saved_maps().items() if torch.is_tensor(v)},
                         grads={n: (a.clone(), b.clone()) for n, (a, b) in grads.items()})
    a, b = out['f32'], out['bf16']
    assert torch.equal(a['score'], b['score'])
    assert sorted(a['saved']) == sorted(b['saved'])
    for k in a['saved']:
        assert torch.equal(a['saved'][k], b['saved'][k]), k
    stay = [n for n in a['grads'] if n not in FCN8_3X3]
    assert sorted(stay) == sorted(['fc6', 'fc7', 'score_fr', 'score_pool3', 'score_pool4', 'score2', 'score4',
                                   'upsample'])
    for n in stay:                                               # K x K, 1 x 1 and transposed layers: float32 as before
        assert torch.equal(a['grads'][n][0], b['grads'][n][0]) and torch.equal(a['grads'][n][1], b['grads'][n][1]), n
    assert any(not torch.equal(a['grads'][n][0], b['grads'][n][0]) for n in FCN8_3X3)
    cos = _cosines({n: b['grads'][n] for n in FCN8_3X3}, {n: a['grads'][n] for n in FCN8_3X3})
    print('FCN-8 wgrad bf16 against f32: worst error / bound %.3g, max relative difference %.3g, cosine per layer %s'
          % (worst, _max_rel(b['grads'], a['grads'], FCN8_3X3), {n: '%.6f' % c for n, c in cos.items()}))
    assert all(np.isfinite(c) for c in cos.values())


# ---- 6. training ----
def _trainer(wgrad, **kw):
    from iterative_inference_segm_amd.train import DAETrainer
    return DAETrainer(None, _std_dae('second', wgrad), 11, [11], noise=0.1, **kw)


def test_loss_goes_down_over_40_steps_with_bf16_weight_gradients(built_lib):
    hs, T = _std_case('second')[1], _std_case('second')[3]
    tr = _trainer('bf16', seed=2, learning_rate=1e-4)
    hd, Td = [_dev(h) for h in hs], _dev(T)
    yd = Td[:, :11].contiguous()                                 # from_gt
    losses = [tr.train_step(hd, yd, Td) for _ in range(40)]
    losses = [float(v) for v in torch.stack(losses).cpu()]
    print('standard DAE loss, wgrad bf16, steps 0-9: %.5f, steps 30-39: %.5f'
          % (np.mean(losses[:10]), np.mean(losses[-10:])))
    assert np.all(np.isfinite(losses))
    assert np.mean(losses[-10:]) < np.mean(losses[:10])


def test_one_step_is_deterministic_and_differs_from_the_f32_mode(built_lib):
    hs, T = _std_case('second')[1], _std_case('second')[3]
    hd, Td = [_dev(h) for h in hs], _dev(T)
    yd = Td[:, :11].contiguous()
    flats = {}
    for key, mode in (('a', 'bf16'), ('b', 'bf16'), ('f32', 'f32')):
        tr = _trainer(mode, seed=3, learning_rate=1e-2)
        tr.train_step(hd, yd, Td)
        torch.cuda.synchronize()
        flats[key] = tr.dae.flat.clone()
    assert torch.equal(flats['a'], flats['b'])
    assert bool(torch.isfinite(flats['a']).all())
    assert not torch.equal(flats['a'], flats['f32'])             # the mode took effect


# ---- 7. the drivers ----
def test_train_dae_driver_end_to_end_with_bf16_weight_gradients(built_lib, tmp_path):
    from iterative_inference_segm_amd.dae import buildDAE
    from iterative_inference_segm_amd.helpers import build_experiment_name
    save, load, out = str(tmp_path / 'save'), str(tmp_path / 'load'), str(tmp_path / 'out')
    dd = {'kind': 'standard', 'dropout': 0, 'skip': True, 'unpool_type': 'trackind', 'noise': 0.1,
          'concat_h': ['pool2'], 'from_gt': True, 'n_filters': 8, 'conv_before_pool': 1, 'additional_pool': 2,
          'temperature': 1.0, 'path_weights': '', 'layer': 'probs_dimshuffle', 'exp_name': 't_', 'bn': 0}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_dae.py'), '--synthetic', '--num_epochs', '1',
                        '--n_images', '4', '--image_size', '40', '36', '--savepath', save, '--loadpath', load,
                        '-segmentation_net', 'fcn8', '-train_dict', '{"batch_size": [2, 2, 2]}',
                        '-dae_dict', json.dumps(dd), '--wgrad', 'bf16'],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    exp, = os.listdir(os.path.join(save, 'camvid'))
    # the folder of the fp32 run: the mode stays out of the name
    assert exp == build_experiment_name('fcn8', data_aug=True, ae_h=False, training_loss=['crossentropy'],
                                        learning_rate=0.0001, lr_anneal=0.99, weight_decay=0.0001,
                                        optimizer='rmsprop', **dd)
    assert 'wgrad = bf16' in open(os.path.join(save, 'camvid', exp, 'config.txt')).read().splitlines()
    folder = os.path.join(load, 'camvid', exp)
    dae = buildDAE(n_classes=11, concat_h=dd['concat_h'], n_filters=8, additional_pool=2, skip=True,
                   unpool_type='trackind', path_weights=folder, model_name='dae_model_best.npz', load_weights=True)
    assert dae.enc['conv3_1'].Cin == 16 + 128                    # h: pool2 of the FCN-8
    assert dae.enc['conv1_1'].W.dtype == torch.float32 and bool(torch.isfinite(dae.enc['conv1_1'].W).all())
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'iterative_inference.py'), '--synthetic', '--n_images', '2',
                        '--image_size', '40', '36', '--batch_size', '2', '--num_iter', '2', '-segmentation_net',
                        'fcn8', '--savepath', out, '--loadpath', load, '-dae_dict', json.dumps(dd)],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_train_fcn8_driver_end_to_end_with_bf16_weight_gradients(built_lib, tmp_path):
    from iterative_inference_segm_amd.fcn8 import buildFCN8
    save, weights, out = str(tmp_path / 'save'), str(tmp_path / 'weights'), str(tmp_path / 'out')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_fcn8.py'), '--synthetic', '--num_epochs', '2',
                        '--n_images', '2', '--image_size', '26', '30', '-batch_size', '[2, 2, 2]', '--savepath', save,
                        '--width_div', '16', '--fc_channels', '32', '--max_batches', '1', '-penal_cst', '1e-4',
                        '--wgrad', 'bf16'], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert os.listdir(os.path.join(save, 'camvid')) == ['fcn8_data_aug']     # the fp32 run's folder
    folder = os.path.join(save, 'camvid', 'fcn8_data_aug')
    assert 'wgrad = bf16' in open(os.path.join(folder, 'config.txt')).read().splitlines()
    models = [f for f in os.listdir(folder) if f in ('new_fcn8_model_best.npz', 'new_fcn8_model_last.npz')]
    assert models
    path = os.path.join(folder, models[0])
    net = buildFCN8(3, path_weights=path, n_classes=11)
    x = _dev(np.random.default_rng(1).random((2, 3, 26, 30)))
    probs = net(x)[0]
    assert tuple(probs.shape) == (2, 11, 26, 30) and bool(torch.isfinite(probs).all())
    assert all(conv.W.dtype == torch.float32 for conv in net.convs.values())
    # iterative inference on the checkpoint as the segmentation net (the DAE: the seeded context module on the image)
    os.makedirs(os.path.join(weights, 'camvid'))
    shutil.copy(path, os.path.join(weights, 'camvid', 'fcn8_model.npz'))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'iterative_inference.py'), '--synthetic', '--n_images', '2',
                        '--image_size', '26', '30', '--batch_size', '2', '--num_iter', '2', '-segmentation_net',
                        'fcn8', '--savepath', out, '--weights_path', weights, '--loadpath', str(tmp_path / 'none'),
                        '-dae_dict', '{"kind": "contextmod", "concat_h": ["input"]}'],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
