"""GPU: the trainable modules hand the library the calls they handed it before their data gradients, parameter
plumbing and trainers were gathered in one place each (datagrads.DataGrads, params.Trainable, train._Trainer).
tests/golden/train_launch_trace.json holds, per case below, every call into libiiseg_hip.so in order: the entry point
and each argument as the entry's declared argtypes (_lib.SIGNATURES) classify it -- a scalar by value, a pointer as
null ('0') or not ('p'), a descriptor struct as its fields.  Recorded on an MI355X with the modules as they were
before that change, through the public API only (`python tests/test_gpu_train_launch_trace.py --record [path]`
rewrites it from the tree: only for a change that is meant to add, drop, reorder or re-describe a launch).

The cases: the standard DAE (SMALL and SECOND of tests/std_train_ref.py) in four modes -- two train steps (the second
covers refresh(), stale filter images and buffer reuse), val_step, backward_y (with dgrad alone 'bf16': the forced
flipped-filter form) -- and its C8 adjoint (mma='bf16c8', keep_pre: scores, backward_y); FCN-8 (SMALL of
tests/fcn8_train_ref.py at 26x30, batch 3) in five modes -- two train steps under given dropout masks, val_step; the
context-module DAE (the case of tests/test_gpu_ctx_train.py) in both precisions -- two train steps, val_step,
backward_y, sqerr_backward; FC-DenseNet (THIN of tests/densenet_train_ref.py at 13x18, batch 2) in three modes -- two
train steps under given dropout masks, val_step."""
import contextlib
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == '__main__':
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import densenet_train_ref as RD
import fcn8_train_ref as RF
import std_train_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'train_launch_trace.json')
DT = {'f32': torch.float32, 'f64': torch.float64}


# ---- the recorder ----
def _arg(argtype, a):
    if isinstance(argtype, type) and issubclass(argtype, C._Pointer):
        if a is not None and issubclass(argtype._type_, C.Structure):
            d = a._obj if hasattr(a, '_obj') else a.contents
            vals = (getattr(d, n) for n, _ in d._fields_)
            return '{%s}' % ','.join(repr(list(v)) if isinstance(v, C.Array) else repr(v) for v in vals)
        return 'p' if a else '0'
    v = getattr(a, 'value', a)
    if argtype in (C.c_void_p, C.c_char_p):
        return 'p' if v else '0'
    return repr(float(v)) if isinstance(v, (float, np.floating)) else repr(int(v))


class _Traced:
    """The library object with every declared entry point recording its call before making it."""

    def __init__(self, lib, calls):
        from iterative_inference_segm_amd import _lib
        self._lib, self._calls, self._sigs = lib, calls, _lib.SIGNATURES

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in self._sigs:
            return fn
        argtypes = self._sigs[name][1]

        def call(*args):
            self._calls.append('%s(%s)' % (name, ' '.join(_arg(t, a) for t, a in zip(argtypes, args))))
            return fn(*args)
        return call


@contextlib.contextmanager
def _tracing():
    from iterative_inference_segm_amd import _lib
    load, calls = _lib.load, []
    traced = _Traced(_lib.load(), calls)
    _lib.load = lambda: traced
    try:
        yield calls
    finally:
        _lib.load = load


# ---- the cases ----
def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda().contiguous()


STD_MODELS = {'small': R.SMALL, 'second': R.SECOND}
STD_MODES = {'f32': ('f32', {}), 'bf16': ('f32', dict(wgrad='bf16', dgrad='bf16', fwd='bf16')),
             'dgrad16': ('f32', dict(dgrad='bf16')), 'f64': ('f64', {})}
FCN_MODES = {'f32': ('f32', {}), 'bf16': ('f32', dict(wgrad='bf16', dgrad='bf16', kxk='bf16', fwd='bf16')),
             'kxk16': ('f32', dict(kxk='bf16')), 'dgrad16': ('f32', dict(dgrad='bf16')), 'f64': ('f64', {})}
DENSE_MODES = {'f32': ('f32', {}), 'bf16': ('f32', dict(wgrad='bf16', deconv='bf16')), 'f64': ('f64', {})}
_DATA = {}


def _data(key, make):
    if key not in _DATA:
        _DATA[key] = make()
    return _DATA[key]


def _std(which, mode):
    from iterative_inference_segm_amd.dae import StandardDAE
    from iterative_inference_segm_amd.train import DAETrainer
    C_, _, _, cfg = STD_MODELS[which]
    params, hs, y, T = _data(('std', which), lambda: R.make_case(STD_MODELS[which]))
    dt = DT[STD_MODES[mode][0]]
    hd, yd, Td = [_dev(h, dt) for h in hs], _dev(y, dt), _dev(T, dt)
    dae = StandardDAE(params, C_, device='cuda', dtype=dt, mma='f32', trainable=True, **STD_MODES[mode][1], **cfg)
    tr = DAETrainer(None, dae, C_, [C_], noise=0.1, seed=3, learning_rate=1e-3)
    for _ in range(2):
        tr.train_step(hd, yd, Td)
    tr.val_step(hd, yd, Td)
    gy = dae.backward_y(torch.ones_like(yd), yd.shape)
    return dict(flat=dae.flat, gflat=dae.gflat, gy=gy)


def _std_c8():
    from iterative_inference_segm_amd.dae import StandardDAE
    C_, _, _, cfg = R.SECOND
    params, hs, y, _ = _data(('std', 'second'), lambda: R.make_case(R.SECOND))
    dae = StandardDAE(params, C_, device='cuda', dtype=torch.float32, mma='bf16c8', **cfg)
    dae.keep_pre = True
    hd, yd = [_dev(h, torch.float32) for h in hs], _dev(y, torch.float32)
    score = dae.scores(hd, yd)
    return dict(score=score, gy=dae.backward_y(torch.ones_like(score), yd.shape))


def _fcn(mode):
    from iterative_inference_segm_amd.fcn8 import FCN8
    from iterative_inference_segm_amd.train import FCN8Trainer
    params, x, T, k6, k7 = _data('fcn', lambda: RF.make_case(3, 26, 30, seed=5))
    dt = DT[FCN_MODES[mode][0]]
    C_ = RF.SMALL['n_classes']
    net = FCN8(params, C_, layer=['score'], dtype=dt, mma='f32', trainable=True, **FCN_MODES[mode][1])
    tr = FCN8Trainer(net, C_, [C_], learning_rate=1e-3, weight_decay=1e-4)
    xd, Td, k6d, k7d = _dev(x, dt), _dev(T, dt), _dev(k6, dt), _dev(k7, dt)
    for _ in range(2):
        tr.train_step(xd, Td, k6d, k7d)
    tr.val_step(xd, Td)
    return dict(flat=net.flat, gflat=net.gflat)


def _densenet(mode):
    from iterative_inference_segm_amd.densenet import FCDenseNet
    from iterative_inference_segm_amd.train import DenseNetTrainer
    cfg = RD.THIN
    params, x, T, keeps = _data('densenet', lambda: RD.make_case(cfg, seed=3))
    dt = DT[DENSE_MODES[mode][0]]
    C_ = cfg['n_classes']
    net = FCDenseNet(params, C_, layer=[], n_layers_per_block=cfg['nlpb'], n_pool=cfg['n_pool'], growth=cfg['growth'],
                     dtype=dt, mma='f32', trainable=True, **DENSE_MODES[mode][1])
    tr = DenseNetTrainer(net, C_, [C_], learning_rate=1e-3, weight_decay=1e-4)
    xd, Td, kd = _dev(x, dt), _dev(T, dt), [_dev(k, dt) for k in keeps]
    for _ in range(2):
        tr.train_step(xd, Td, kd)
    tr.val_step(xd, Td)
    return dict(flat=net.flat, gflat=net.gflat)


def _ctx_case(B=2, H=40, W=36, seed=11):
    from iterative_inference_segm_amd import synthetic as S
    rng = np.random.default_rng(seed)
    params = S.make_contextmod_params(11, 3, seed=31)
    h = S.make_images(B, H, W, seed=seed)
    T = S.make_labels(B, H, W, n_classes=11, void_frac=0.1, seed=seed + 1)
    y = np.clip(T[:, :11] + 0.1 * rng.standard_normal((B, 11, H, W)), 0, 1)
    return params, h.astype(np.float64), y.astype(np.float64), T.astype(np.float64)


def _ctx(mode):
    from iterative_inference_segm_amd.contextmod import ContextModDAE
    from iterative_inference_segm_amd.train import DAETrainer
    params, h, y, T = _data('ctx', _ctx_case)
    dt = DT[mode]
    hd, yd, Td = _dev(h, dt), _dev(y, dt), _dev(T, dt)
    dae = ContextModDAE(params, 11, dtype=dt)
    tr = DAETrainer(None, dae, 11, [11], noise=0.1, seed=3, learning_rate=1e-3)
    for _ in range(2):
        tr.train_step(hd, yd, Td)
    tr.val_step(hd, yd, Td)
    dae.keep_pre = True
    score = dae.scores([hd], yd)
    gy = dae.backward_y(torch.ones_like(score), yd.shape)
    gs = dae.sqerr_backward(score, yd)
    return dict(flat=dae.flat, gflat=dae.gflat, gy=gy, gs=gs)


CASES = {'std/%s/%s' % (w, m): (lambda w=w, m=m: _std(w, m)) for w in STD_MODELS for m in STD_MODES}
CASES['std/second/c8_adjoint'] = _std_c8
CASES.update({'fcn8/%s' % m: (lambda m=m: _fcn(m)) for m in FCN_MODES})
CASES.update({'ctx/%s' % m: (lambda m=m: _ctx(m)) for m in ('f32', 'f64')})
CASES.update({'densenet/%s' % m: (lambda m=m: _densenet(m)) for m in DENSE_MODES})


def run_case(name):
    """(the calls of case `name`, its result tensors by name)."""
    with _tracing() as calls:
        out = CASES[name]()
        torch.cuda.synchronize()
    return calls, out


# ---- the test ----
@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    return {name: [g['calls'][i] for i in idx] for name, idx in g['cases'].items()}


def test_the_fixture_names_the_cases(golden):
    assert sorted(golden) == sorted(CASES)
    assert all(len(v) > 20 for v in golden.values())


@pytest.mark.parametrize('name', sorted(CASES))
def test_the_library_sees_the_calls_it_saw_before(built_lib, golden, name):
    got, want = run_case(name)[0], golden[name]
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            print('%s: call %d of %d differs\n  recorded: %s\n  now:      %s' % (name, i, len(want), w, g))
            pytest.fail('%s: call %d differs (printed in full above)' % (name, i))
    if len(got) != len(want):
        longer, what = (got, 'more') if len(got) > len(want) else (want, 'fewer')
        print('%s: %d calls recorded, %d now; the first of the rest: %s' % (name, len(want), len(got),
                                                                           longer[min(len(got), len(want))]))
        pytest.fail('%s: %d calls %s than recorded' % (name, abs(len(got) - len(want)), what))


def _record(path):
    table, cases = {}, {}
    for name in sorted(CASES):
        cases[name] = [table.setdefault(line, len(table)) for line in run_case(name)[0]]
        print('%s: %d calls' % (name, len(cases[name])), flush=True)
    with open(path, 'w') as f:                              # one call per line, one case per line
        f.write('{"calls": [\n%s\n],\n"cases": {\n%s\n}}\n' % (
            ',\n'.join(json.dumps(line) for line in table),
            ',\n'.join('%s: %s' % (json.dumps(n), json.dumps(idx, separators=(',', ':'))) for n, idx in cases.items())))
    print('recorded %d cases, %d distinct calls, %d bytes' % (len(cases), len(table), os.path.getsize(path)))


if __name__ == '__main__' and '--record' in sys.argv:
    rest = sys.argv[sys.argv.index('--record') + 1:]
    _record(rest[0] if rest else GOLDEN)
