"""GPU: the dense-CRF mean-field kernels (csrc/crf.hip) through iterative_inference_segm_amd.crf and the
raw C ABI, against the float64 restatement tests/crf_ref.py; and the crf_inference.py drop-in end to end."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import crf_ref as R
from iterative_inference_segm_amd import synthetic as S

pytestmark = pytest.mark.gpu


def scene(B, H, W, Cn=11, seed=0, conc=None):
    """Blob label maps (make_labels) painted one colour per class with +-4 levels of noise; probabilities
    from softened noisy one-hots (or Dirichlet(conc) when `conc` is given).  float32 values."""
    rng = np.random.default_rng(seed)
    L = S.make_labels(B, H, W, n_classes=Cn, seed=seed + 1, block=8)
    cls = L.argmax(1)
    palette = rng.integers(16, 240, size=(Cn + 1, 3))
    v = palette[cls] + rng.integers(-4, 5, size=(B, H, W, 3))
    X = ((v + 0.5) / 255.0).astype(np.float32).transpose(0, 3, 1, 2).copy()
    if conc is not None:
        P = rng.dirichlet(np.full(Cn, conc), size=(B, H, W)).transpose(0, 3, 1, 2)
    else:
        oh = np.eye(Cn)[np.minimum(cls, Cn - 1)].transpose(0, 3, 1, 2)
        logit = 2.0 * oh + rng.normal(0.0, 1.0, size=oh.shape)
        P = np.exp(logit) / np.exp(logit).sum(1, keepdims=True)
    return np.ascontiguousarray(P.astype(np.float32)), X


def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()


def run(P, X, n, dt, bilateral=True, radius=None):
    from iterative_inference_segm_amd.crf import DenseCRF
    Q = DenseCRF(radius=radius).inference(dev(P, dt), dev(X, dt), n, bilateral=bilateral)
    torch.cuda.synchronize()
    return Q.cpu().double().numpy()


@pytest.mark.parametrize('B,H,W,Cn,Rr,n,bil', [
    (2, 64, 48, 11, None, 80, True),
    (2, 64, 48, 11, None, 80, False),
    (1, 37, 150, 11, None, 80, True),       # ragged in both tile directions
    (1, 40, 33, 5, 1, 80, True),
    (1, 40, 33, 5, 16, 80, True),
    (1, 30, 70, 2, None, 80, True),
    (1, 30, 70, 16, None, 80, True),
    (2, 7, 90, 11, None, 80, True),         # H < R
    (1, 224, 224, 11, None, 5, True),
])
def test_f64_kernels_match_restatement(built_lib, B, H, W, Cn, Rr, n, bil):
    P, X = scene(B, H, W, Cn, seed=H * W + Cn)
    got = run(P, X, n, torch.float64, bilateral=bil, radius=Rr)
    ref = R.crf_inference(P.astype(np.float64), X, n, bilateral=bil, R=Rr)
    assert np.isfinite(got).all()
    err = np.abs(got - ref).max()
    assert err <= 1e-10, err


def _raw(dt, d, P, X):
    """crf_prepare through the raw ABI -> dict of device outputs."""
    from iterative_inference_segm_amd import _lib
    from iterative_inference_segm_amd.ops import _ptr, _stream
    lib = _lib.load()
    B, Cn, H, W = P.shape
    o = {k: torch.empty(s, dtype=dt, device='cuda') for k, s in
         (('U', (B, Cn, H, W)), ('Q0', (B, Cn, H, W)), ('I', (B, 3, H, W)), ('ng', (B, H, W)), ('nb', (B, H, W)))}
    sfx = 'f32' if dt == torch.float32 else 'f64'
    st = getattr(lib, 'iiseg_crf_prepare_' + sfx)(_stream(), C.byref(d), _ptr(P, dt), _ptr(X, dt),
                                                 *[_ptr(o[k], dt) for k in ('U', 'Q0', 'I', 'ng', 'nb')])
    assert st == 0
    return o


@pytest.mark.parametrize('H,W', [(224, 224), (37, 150)])
def test_f32_teacher_forced(built_lib, H, W):
    from iterative_inference_segm_amd import _lib
    from iterative_inference_segm_amd.crf import DenseCRF
    from iterative_inference_segm_amd.ops import _ptr, _stream
    P, X = scene(1, H, W, 11, seed=5, conc=0.8)
    crf = DenseCRF()
    d = crf.desc(1, 11, H, W)
    o32 = _raw(torch.float32, d, dev(P, torch.float32), dev(X, torch.float32))
    o64 = _raw(torch.float64, d, dev(P, torch.float64), dev(X, torch.float64))
    for k in o32:
        a, b = o32[k].double().cpu().numpy(), o64[k].cpu().numpy()
        assert (np.abs(a - b) <= 1e-6 * np.abs(b) + 1e-30).all(), k
    ref = R.ImageCRF(P[0].astype(np.float64), X[0])
    assert np.abs(o64['nb'].cpu().numpy()[0] - ref.nb).max() <= 1e-13
    assert np.array_equal(o64['I'].cpu().numpy()[0], ref.I)
    # one step fed the float64 Q of iteration 3
    Q3 = ref.run(3)
    want = ref.step(Q3)
    lib = _lib.load()
    qin = dev(Q3[None], torch.float32)
    qout = torch.empty_like(qin)
    st = lib.iiseg_crf_step_f32(_stream(), C.byref(d), _ptr(o32['U']), _ptr(qin), _ptr(o32['I']),
                                _ptr(o32['ng']), _ptr(o32['nb']), _ptr(qout))
    assert st == 0
    err = np.abs(qout.cpu().double().numpy()[0] - want).max()
    assert err <= 1e-5, err


@pytest.mark.parametrize('H,W', [(64, 48), (37, 150)])
def test_f32_free_running(built_lib, H, W):
    P, X = scene(2, H, W, 11, seed=11)
    P64 = P.astype(np.float64)
    err10 = np.abs(run(P, X, 10, torch.float32) - R.crf_inference(P64, X, 10)).max()
    assert err10 <= 1e-4, err10
    q32 = run(P, X, 80, torch.float32)
    q64 = R.crf_inference(P64, X, 80)
    agree = (q32.argmax(1) == q64.argmax(1)).mean()
    assert agree >= 0.999, agree


def test_batch_images_are_independent(built_lib):
    P, X = scene(10, 50, 70, 11, seed=21)
    allq = run(P, X, 6, torch.float32)
    for b in (0, 3, 9):
        one = run(P[b:b + 1], X[b:b + 1], 6, torch.float32)
        assert np.array_equal(one[0], allq[b]), b


@pytest.mark.parametrize('dt', [torch.float32, torch.float64])
def test_guard_bands_and_simplex(built_lib, dt):
    from iterative_inference_segm_amd import _lib
    from iterative_inference_segm_amd.crf import DenseCRF
    from iterative_inference_segm_amd.ops import _ptr, _stream
    B, Cn, H, W, G = 2, 11, 45, 77, 4096
    P, X = scene(B, H, W, Cn, seed=31)
    d = DenseCRF().desc(B, Cn, H, W)
    canary = -12345.0
    shapes = {'U': (B, Cn, H, W), 'I': (B, 3, H, W), 'ng': (B, H, W), 'nb': (B, H, W),
              'Qa': (B, Cn, H, W), 'Qb': (B, Cn, H, W)}
    bufs, views = {}, {}
    for k, s in shapes.items():
        n = int(np.prod(s))
        bufs[k] = torch.full((n + 2 * G,), canary, dtype=dt, device='cuda')
        views[k] = bufs[k][G:G + n].view(s)
    sfx = 'f32' if dt == torch.float32 else 'f64'
    lib = _lib.load()
    p = lambda t: _ptr(t, dt)
    assert getattr(lib, 'iiseg_crf_prepare_' + sfx)(_stream(), C.byref(d), p(dev(P, dt)), p(dev(X, dt)),
                                                   p(views['U']), p(views['Qa']), p(views['I']),
                                                   p(views['ng']), p(views['nb'])) == 0
    a, b = views['Qa'], views['Qb']
    for _ in range(5):
        assert getattr(lib, 'iiseg_crf_step_' + sfx)(_stream(), C.byref(d), p(views['U']), p(a), p(views['I']),
                                                    p(views['ng']), p(views['nb']), p(b)) == 0
        a, b = b, a
    torch.cuda.synchronize()
    for k, buf in bufs.items():
        h = buf.cpu().numpy()
        assert (h[:G] == canary).all() and (h[-G:] == canary).all(), k
    q = a.cpu().double().numpy()
    assert np.isfinite(q).all()
    assert np.abs(q.sum(1) - 1).max() <= 1e-6


def _numbers(line):
    return [float(v) for v in re.findall(r'[-+]?\d+\.\d+|nan', line)]


def test_driver_end_to_end_fcn8(built_lib, tmp_path, capsys):
    import crf_inference as ci
    from iterative_inference_segm_amd.api import IterativeInference
    sp, lp = str(tmp_path / 's'), str(tmp_path / 'l')
    ci.main(['--synthetic', '--savepath', sp, '--loadpath', lp, '--n_images', '3', '--image_size', '48', '64',
             '--sweep', '4', '-which_set', 'val'])
    out = capsys.readouterr().out
    res = np.load(os.path.join(lp, 'camvid', 'fcn8', 'img_plots', 'crf', 'results_val.npz'))['arr_0']
    assert res.shape == (11, 1)
    d = os.path.join(lp, 'camvid', 'fcn8', 'img_plots', 'crf', '4', 'val')
    z = np.load(os.path.join(d, 'batch0.npz'))
    assert sorted(z.files) == ['L', 'X', 'Y_crf', 'Y_fcn']
    assert z['Y_fcn'].shape == (3, 12, 48, 64) and z['Y_crf'].shape == (3, 11, 48, 64)
    assert (z['Y_fcn'][:, 11] == 0).all()
    assert '>>>>> Per class jaccard:' in out
    lines = out.splitlines()
    test_line = [l for l in lines if l.startswith('TEST: acc crf ')][0]
    acc_crf, jacc_crf, acc_fcn, jacc_fcn = _numbers(test_line)
    cls = [l for l in lines if re.match(r'    \w+ : fcn ->  ', l)]
    assert len(cls) == 11 and cls[0].startswith('    sky : fcn ->  ')
    ii = IterativeInference(None, None, 11, [11])
    acc, jacc, _ = ii.val_fn(torch.from_numpy(z['Y_crf']).cuda(), torch.from_numpy(z['L']).cuda())
    assert abs(acc - acc_crf) <= 1e-6
    iou = jacc[0] / jacc[1]
    assert abs(np.nanmean(iou) - jacc_crf) <= 1e-6
    assert np.allclose(res[:, 0], iou, equal_nan=True)
    acc, jacc, _ = ii.val_fn(torch.from_numpy(np.ascontiguousarray(z['Y_fcn'][:, :11])).cuda(),
                             torch.from_numpy(z['L']).cuda())
    assert abs(acc - acc_fcn) <= 1e-6 and abs(np.nanmean(jacc[0] / jacc[1]) - jacc_fcn) <= 1e-6


def test_driver_end_to_end_densenet(built_lib, tmp_path, capsys):
    import crf_inference as ci
    sp = str(tmp_path / 's')
    res = ci.inference('camvid', 'densenet', which_set='test', num_iter=3, savepath=sp, loadpath=sp,
                       synthetic=True, n_images=3, image_size=(64, 64), batch_size=2)
    out = capsys.readouterr().out
    assert res.shape == (11,)
    d = os.path.join(sp, 'camvid', 'densenet', 'img_plots', 'crf', '3', 'test')
    for i, nb in ((0, 2), (1, 1)):
        z = np.load(os.path.join(d, 'batch%d.npz' % i))
        assert z['Y_fcn'].shape == (nb, 11, 64, 64) and z['Y_crf'].shape == (nb, 11, 64, 64)
        assert np.abs(z['Y_crf'].sum(1) - 1).max() <= 1e-5
    assert 'Batch 2 out of 2' in out and 'TEST: acc crf ' in out and 'Copying' not in out
