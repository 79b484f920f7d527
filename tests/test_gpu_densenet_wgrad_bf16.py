"""GPU: wgrad='bf16' on FC-DenseNet -- the 16-output-channel form of the bf16 weight gradient
(csrc/conv_wgrad_bf16.hip's co16 form; ops.conv_wgrad(mma='bf16', co_block=16)) and the switch through the module, the
trainer and train_fcdensenet.py.  The kernel: exact on data bf16 holds exactly, over every descriptor feature; on
real data within the any-order fp32 accumulation bound of the float64 sum over operands rounded on the CPU with
.to(torch.bfloat16), ties and direction included, db from the unrounded g_z, the same bits twice.  The module: nothing
but the zero-padded 3x3 weight gradients changes between the modes, every ops.conv_wgrad call of `backward` carries
the mode and the form `densenet.wgrad_co_block` names, and meets the bound on its own operands.

Measured on an MI355X (for the record; the assertions are the derived bounds): see DESIGN.md section 22."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import densenet_train_ref as R
import wgrad_bf16_ref as WR
from wgrad_bf16_ref import F32, U, bound_check as _bound_check, dev as _dev, pad as _pad, taps as _taps

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(mma='bf16', co_block=16)


# ---- 1. exact on small integers ----
GEOMETRY = [(7, 7, 1), (14, 13, 1), (37, 150, 1), (3, 4, 5), (14, 13, 5), (1, 1, 1), (2, 9, 1)]
CHANNELS = [(1, 16), (5, 16), (48, 16), (67, 16), (24, 4), (24, 11), (20, 33)]
DEEP = [(130, 16), (300, 16), (1072, 16)]                        # several input-channel blocks; on the small maps only
# the edges of the blocks that the staging decides: at most 16 / 32 / 64 input channels and one more (the kernel
# stages 2, 4 or 8 x channels per wave), and a second block of output channels; on three small maps
EDGES = [(16, 16), (17, 16), (32, 16), (33, 16), (64, 16), (65, 16), (24, 17)]
INT_CASES = [(ci, co, h, w, p) for ci, co in CHANNELS for h, w, p in GEOMETRY] + \
            [(ci, co, h, w, p) for ci, co in DEEP for h, w, p in GEOMETRY[:2]] + \
            [(ci, co, h, w, p) for ci, co in EDGES for h, w, p in (GEOMETRY[0], GEOMETRY[1], GEOMETRY[3])]


def _int_case(Cin, Cout, B, H, W, pad):
    return WR.int_case(Cin, Cout, B, H, W, pad, np.float64)


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('Cin,Cout,H,W,pad', INT_CASES)
def test_co16_weight_gradient_is_exact_on_integers(built_lib, Cin, Cout, B, H, W, pad):
    from iterative_inference_segm_amd import _lib, ops
    x, gz, dW_ref, db_ref = _int_case(Cin, Cout, B, H, W, pad)
    xd, gzd = _dev(x), _dev(gz)
    nslab = _lib.load().iiseg_conv_wgrad_bf16_co16_slabs(C.byref(ops.conv_wgrad_desc(x.shape, Cout, pad)))
    if (H, W) == (37, 150):
        assert nslab >= 2                                        # slabs + the finalize launch
    if (H, W) == (7, 7) and B == 1:
        assert nslab == 1                                        # straight into dW
    # the layer's own array, W[out, in, 3, 3]
    dW = torch.full(dW_ref.shape, 7.0, dtype=F32, device='cuda')
    db = torch.full((Cout,), 7.0, dtype=F32, device='cuda')
    ops.conv_wgrad(xd, gzd, dW, db, pad=pad, **KW)
    # the middle of a wider parameter, in both layouts: the other input channels keep the sentinel; no db
    lo, hi = 3, 5
    big = torch.full((Cout, lo + Cin + hi, 3, 3), -9.0, dtype=F32, device='cuda')
    ops.conv_wgrad(xd, gzd, big, None, pad=pad, ci0=lo, **KW)
    bigT = torch.full((lo + Cin + hi, Cout, 3, 3), -9.0, dtype=F32, device='cuda')
    ops.conv_wgrad(xd, gzd, bigT, None, pad=pad, ci0=lo, layout='iohw', **KW)
    torch.cuda.synchronize()
    assert np.array_equal(dW.cpu().numpy(), dW_ref)
    assert np.array_equal(db.cpu().numpy(), db_ref)
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
    ops.conv_wgrad(x.cuda(), gz.cuda(), dW, db, pad=1, **KW)
    torch.cuda.synchronize()
    frac, ref, mag = _bound_check(dW, x, gz, 1, 'rounding point')
    # (the statement discriminates: against the sum of the UNROUNDED operands the same bound fails)
    exact = _taps(gz.double().numpy(), _pad(x.double().numpy(), 1), 7, 7)
    n = 49
    assert (np.abs(dW.cpu().double().numpy() - exact) > (n + 1) * U * mag).mean() > 0.9
    g64 = gz.double().numpy()
    db_err = np.abs(db.cpu().double().numpy() - g64.sum(axis=(0, 2, 3)))
    db_bound = (n + 1) * U * np.abs(g64).sum(axis=(0, 2, 3))
    print('bf16 co16 wgrad 24 -> 16 at 7x7: worst error / bound %.3g (dW), %.3g (db)'
          % (frac, (db_err / db_bound).max()))
    assert (db_err <= db_bound).all()


# ---- 3. ties and direction ----
VALS = [1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -10, -(1 + 2.0 ** -8 + 2.0 ** -10),
        1 + 2.0 ** -7 - 2.0 ** -10]
WANT = [1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, -(1 + 2.0 ** -7), 1 + 2.0 ** -7]


# the single non-zero pixel of the other operand, on an H x W map it is interior to: the centre of 3 x 3 as in the
# 64-block test; on 4 x 12 both rows of a pair of tile rows (the second rides in the odd k-groups of a 16x16x32 step)
# and both pixel halves (the upper k-groups); (5, 3) of 8 x 5 sits in the third pair
@pytest.mark.parametrize('H,W,y,x', [(3, 3, 1, 1), (4, 12, 1, 3), (4, 12, 2, 3), (4, 12, 1, 9), (4, 12, 2, 10),
                                     (8, 5, 5, 3)])
def test_ties_go_to_even_and_negative_values_round_symmetrically(built_lib, H, W, y, x):
    from iterative_inference_segm_amd import ops
    v32 = torch.tensor(VALS, dtype=F32)
    assert v32.double().tolist() == VALS                         # float32 holds them
    assert v32.to(torch.bfloat16).double().tolist() == WANT      # torch's rounding on the CPU
    # as the B operand: channel c of x holds value c at every pixel, g_z is a single 1.0: dW[0, c, ky, kx] = bf16(value c)
    xs = v32.view(1, 5, 1, 1).expand(1, 5, H, W).contiguous().cuda()
    gz = torch.zeros((1, 1, H, W), dtype=F32, device='cuda')
    gz[0, 0, y, x] = 1.0
    dW = torch.full((1, 5, 3, 3), 7.0, dtype=F32, device='cuda')
    ops.conv_wgrad(xs, gz, dW, None, pad=1, **KW)
    got = dW.cpu().double().numpy()
    for c in range(5):
        assert (got[0, c] == WANT[c]).all(), (c, got[0, c], WANT[c])
    # as the A operand: g_z holds value c at that pixel of channel c, x is 1.0 everywhere
    gz = torch.zeros((1, 5, H, W), dtype=F32, device='cuda')
    gz[0, :, y, x] = v32.cuda()
    xs = torch.ones((1, 1, H, W), dtype=F32, device='cuda')
    dW = torch.full((5, 1, 3, 3), 7.0, dtype=F32, device='cuda')
    ops.conv_wgrad(xs, gz, dW, None, pad=1, **KW)
    got = dW.cpu().double().numpy()
    for c in range(5):
        assert (got[c, 0] == WANT[c]).all(), (c, got[c, 0], WANT[c])


# ---- 4. several slabs, twice ----
def test_several_slabs_give_the_same_bits_twice_within_the_bound(built_lib):
    from iterative_inference_segm_amd import ops
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.standard_normal((3, 24, 37, 150)).astype(np.float32))
    gz = torch.from_numpy(rng.standard_normal((3, 16, 37, 150)).astype(np.float32))
    xd, gzd = x.cuda(), gz.cuda()
    runs = []
    for _ in range(2):
        dW = torch.zeros((16, 24, 3, 3), dtype=F32, device='cuda')
        db = torch.zeros(16, dtype=F32, device='cuda')
        ops.conv_wgrad(xd, gzd, dW, db, pad=1, **KW)
        runs.append((dW.cpu(), db.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    n = 3 * 37 * 150
    frac = _bound_check(runs[0][0], x, gz, 1, 'several slabs')[0]
    print('bf16 co16 wgrad 3x24x37x150 -> 16: worst error / bound %.3g' % frac)
    g64 = gz.double().numpy()
    db_err = np.abs(runs[0][1].double().numpy() - g64.sum(axis=(0, 2, 3)))
    assert (db_err <= (n + 1) * U * np.abs(g64).sum(axis=(0, 2, 3))).all()


# ---- 4b. db alone, as the fp32 kernel forms it ----
@pytest.mark.parametrize('H,W,pad', GEOMETRY + [(56, 56, 1)])
@pytest.mark.parametrize('Cin,Cout', [(5, 16), (48, 16), (300, 16), (24, 4), (20, 33), (70, 130)])
def test_db_alone_has_the_bits_of_the_fp32_weight_gradient(built_lib, Cin, Cout, H, W, pad):
    """The fp32 kernel's plan depends on Cin (its slabs), B, the map and the padding (a border share at pad 5): over
    all of them ops.conv_wgrad_db gives the bits ops.conv_wgrad(mma='f32') gives db, on normal data."""
    from iterative_inference_segm_amd import _lib, ops
    B = 3
    OH, OW = H + 2 * pad - 2, W + 2 * pad - 2
    rng = np.random.default_rng(Cin + 10 * Cout + H + pad)
    x = _dev(rng.standard_normal((B, Cin, H, W)))
    gz = rng.standard_normal((B, Cout, OH, OW))
    gz[rng.integers(0, 2, size=gz.shape) == 0] = 0
    gz = _dev(gz)
    if (H, W) in ((37, 150), (56, 56)):
        d = ops.conv_wgrad_desc(x.shape, Cout, pad)
        assert _lib.load().iiseg_conv_wgrad_slabs(C.byref(d), 4) >= 2        # slabs + the finalize launch
    dW = torch.empty((Cout, Cin, 3, 3), dtype=F32, device='cuda')
    want = torch.full((Cout,), 7.0, dtype=F32, device='cuda')
    ops.conv_wgrad(x, gz, dW, want, pad=pad, mma='f32')
    got = torch.full((Cout,), -7.0, dtype=F32, device='cuda')
    ops.conv_wgrad_db(gz, got, Cin, pad=pad)
    torch.cuda.synchronize()
    assert torch.equal(got, want), (got - want).abs().max()


# ---- 5. the module ----
class _Recorder:
    """ops.conv_wgrad, recording every call's operands (copied: the walk reuses its buffers), target and form."""

    def __init__(self, ops):
        self.ops, self.inner, self.calls = ops, ops.conv_wgrad, []

    def __call__(self, x, gz, dW, db=None, pad=1, ci0=0, layout='oihw', mma='f32', co_block=64):
        self.calls.append(dict(x=x.detach().cpu().clone(), gz=gz.detach().cpu().clone(), dW=dW, pad=pad, ci0=ci0,
                               layout=layout, mma=mma, co_block=co_block))
        return self.inner(x, gz, dW, db, pad=pad, ci0=ci0, layout=layout, mma=mma, co_block=co_block)

    def __enter__(self):
        self.ops.conv_wgrad = self
        return self

    def __exit__(self, *exc):
        self.ops.conv_wgrad = self.inner


CASES = {'thin': R.THIN, 'wide': R.WIDE}
_CASES = {}


def _model_case(name):
    if name not in _CASES:
        _CASES[name] = R.make_case(CASES[name], seed=3)
    return _CASES[name]


def _net(name, wgrad, **kw):
    from iterative_inference_segm_amd.densenet import FCDenseNet
    cfg = CASES[name]
    return FCDenseNet(_model_case(name)[0], cfg['n_classes'], layer=[], n_layers_per_block=cfg['nlpb'],
                      n_pool=cfg['n_pool'], growth=cfg['growth'], dtype=F32, mma='f32', trainable=True, wgrad=wgrad,
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
def test_module_changes_nothing_but_the_3x3_weight_gradients(built_lib, name):
    from iterative_inference_segm_amd import ops
    cfg = CASES[name]
    params, x, T, keeps = _model_case(name)
    xd, Td, kd = _dev(x), _dev(T), [_dev(k) for k in keeps]
    out = {}
    for mode in ('f32', 'bf16'):
        net = _net(name, mode)
        assert net.wgrad == mode
        score = net.forward_train(xd, kd)
        _, g, _ = ops.ctx_loss(score, Td, ('crossentropy',), 1.0)
        prof = []
        ops.CONV_PROFILE = prof
        try:
            with _Recorder(ops) as rec:
                grads = net.backward(g)
            torch.cuda.synchronize()
        finally:
            ops.CONV_PROFILE = None
        launched = [k for k, _, _, _ in prof if k.startswith('conv_wgrad') and 'kxk' not in k]
        # the zero-padded 3x3 layers in the order `backward` walks them
        layers3 = [e for e in reversed(net._steps) if e['kind'] in ('brc', 'first')]
        assert len(rec.calls) == len(layers3) == sum(cfg['nlpb']) + 1        # exactly one call per 3x3 layer
        worst = 0.0
        for k, (c, e) in enumerate(zip(rec.calls, layers3)):
            cout = cfg['growth'] if e['kind'] == 'brc' else cfg['n_first']
            assert tuple(c['gz'].shape[:2]) == (x.shape[0], cout), (k, e['kind'])
            assert c['x'].shape[1] == (e['n'] if e['kind'] == 'brc' else x.shape[1]), (k, e['kind'])
            assert c['dW'].data_ptr() == grads['conv%03d' % e['li']][0].data_ptr() and c['ci0'] == 0
            assert c['mma'] == mode and c['layout'] == 'oihw' and c['pad'] == 1, (k, c['mma'])
            if mode == 'bf16':
                assert launched[2 * k + 1] == 'conv_wgrad_db_kernel'           # db: the fp32 mode's sums
                assert launched[2 * k] == ('conv_wgrad_bf16_co16_kernel' if c['co_block'] == 16 else
                                           'conv_wgrad_bf16_kernel')
                if e['kind'] == 'brc' or name == 'thin':
                    assert c['co_block'] == 16, (k, e['kind'], c['co_block'])  # growth 4 / 16; 'thin': 8 first filters
                else:
                    assert cout == 48 and c['co_block'] == 64, (k, c['co_block'])
                worst = max(worst, _bound_check(c['dW'], c['x'], c['gz'], 1, '%s call %d' % (name, k))[0])
            else:
                assert c['co_block'] == 64 and launched[k] == 'conv_wgrad_kernel'
        assert len(launched) == len(layers3) * (2 if mode == 'bf16' else 1)    # and nothing else of the kind
        out[mode] = dict(score=score.clone(), saved=_clone(net.saved_maps()), worst=worst,
                         grads={n: (a.clone(), b.clone()) for n, (a, b) in grads.items()},
                         kinds={'conv%03d' % li: L['kind'] for li, L in enumerate(net.layers)})
    a, b = out['f32'], out['bf16']
    assert torch.equal(a['score'], b['score'])
    assert _same(a['saved'], b['saved'])
    kinds = a['kinds']
    three = [n for n, k in kinds.items() if k in ('brc', 'first')]
    assert sorted(set(kinds.values())) == ['brc', 'first', 'softmax', 'td', 'tu']
    for n in a['grads']:
        assert torch.equal(a['grads'][n][1], b['grads'][n][1]), n              # every db; every dbeta
        if n.startswith('bn') or kinds[n] in ('td', 'tu', 'softmax'):
            assert torch.equal(a['grads'][n][0], b['grads'][n][0]), n          # every dgamma; the other layers' dW
    assert any(not torch.equal(a['grads'][n][0], b['grads'][n][0]) for n in three)
    cos, rel = {}, {}
    for n in three:
        u, v = b['grads'][n][0].double().reshape(-1), a['grads'][n][0].double().reshape(-1)
        cos[n] = float(u @ v / (u.norm() * v.norm()))
        rel[n] = float((u - v).abs().max() / v.abs().max())
    print('FC-DenseNet (%s) wgrad bf16 against f32: worst error / bound %.3g, max relative difference %.3g, lowest '
          'cosine %.6f; cosine per layer %s' % (name, b['worst'], max(rel.values()), min(cos.values()),
                                                {n: '%.6f' % c for n, c in cos.items()}))
    assert all(np.isfinite(c) for c in cos.values()) and all(np.isfinite(r) for r in rel.values())


# ---- 6. training ----
def _trainer(wgrad, **kw):
    from iterative_inference_segm_amd.train import DenseNetTrainer
    C_ = R.THIN['n_classes']
    return DenseNetTrainer(_net('thin', wgrad), C_, [C_], **kw)


def test_loss_goes_down_over_40_steps_with_bf16_weight_gradients(built_lib):
    x, T = _model_case('thin')[1:3]
    tr = _trainer('bf16', learning_rate=1e-3, seed=2)
    xd, Td = _dev(x), _dev(T)
    losses = [tr.train_step(xd, Td) for _ in range(40)]
    losses = [float(v) for v in torch.stack(losses).cpu()]
    print('FC-DenseNet loss, wgrad bf16, steps 0-9: %.5f, steps 30-39: %.5f'
          % (np.mean(losses[:10]), np.mean(losses[-10:])))
    assert np.all(np.isfinite(losses))
    assert np.mean(losses[-10:]) < np.mean(losses[:10])


def test_two_steps_are_deterministic_and_one_differs_from_the_f32_mode(built_lib):
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
def test_driver_end_to_end_with_bf16_weight_gradients(built_lib, tmp_path):
    from iterative_inference_segm_amd.densenet import build_fcdensenet
    save = str(tmp_path / 'save')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train_fcdensenet.py'), '--synthetic', '--num_epochs', '2',
                        '--n_images', '2', '--image_size', '16', '16', '--batch_size', '[2, 2, 2]', '--savepath', save,
                        '--layers_per_block', '[2, 3, 2, 3, 2]', '--growth', '4', '--n_first', '8',
                        '--max_batches', '1', '--wgrad', 'bf16'], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert os.listdir(os.path.join(save, 'camvid')) == ['fc_densenet']       # the fp32 run's folder
    folder = os.path.join(save, 'camvid', 'fc_densenet')
    assert 'wgrad = bf16' in open(os.path.join(folder, 'config.txt')).read().splitlines()
    assert 'FC-DenseNet103_weights_best.npz' in os.listdir(folder)           # ... and its checkpoint name
    net = build_fcdensenet(layer=[], n_classes=11, weight_path=os.path.join(folder, 'FC-DenseNet103_weights_best.npz'))
    x = _dev(np.random.default_rng(1).random((2, 3, 16, 16)))
    probs = net(x)[-1]
    assert tuple(probs.shape) == (2, 11, 16, 16) and bool(torch.isfinite(probs).all())
