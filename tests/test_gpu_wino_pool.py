"""GPU: the 2x2 max-pool and the DePool2D mask bytes on the fp32 Winograd layers
(include/iiseg.h, iiseg_conv_wino_mask_f32 / iiseg_maxpool2x2_mask_window_f32): pooled maps and
mask bytes equal, bit for bit, the stored conv output -> maxpool2x2 -> equality mask; the decoder
conv from mask bytes equals the pre / pooled form; the bench workload gives the same bits with the
fusion on and off."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops(built_lib):
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from iterative_inference_segm_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def arr(t):
    return host(t) if isinstance(t, torch.Tensor) else np.asarray(t)


def rnd(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


def eq_bits(pre, pooled):
    B, Cc, H, W = pre.shape
    h2, w2 = H // 2, W // 2
    m = np.zeros((B, Cc, h2, w2), np.uint8)
    for dy in (0, 1):
        for dx in (0, 1):
            m |= ((pre[:, :, dy:2 * h2:2, dx:2 * w2:2] == pooled).astype(np.uint8) << (dy * 2 + dx))
    return m


# B, Cin, H, W, Cout, add: Cin 128 runs the fused GEMM + output kernel, Cin 320 (or a skip-add) the
# GEMM + separate output transform; odd map sizes leave the last row / column unpooled
POOL_CASES = [(2, 128, 13, 13, 128, False), (1, 128, 33, 35, 256, False), (1, 320, 58, 57, 128, False),
              (2, 128, 21, 18, 128, True)]


@pytest.mark.parametrize('case', POOL_CASES)
def test_wino_pool_and_mask_epilogue_is_bit_exact(ops, case):
    B, Cin, H, W, Cout, with_add = case
    rng = np.random.default_rng(hash(case) % 2**32)
    x, w, b = rnd(rng, B, Cin, H, W), rnd(rng, Cout, Cin, 3, 3) * 0.05, rnd(rng, Cout)
    conv = ops.Conv(w, b, pad=1, relu=True)
    assert conv.wino
    fh, fw = conv.out_hw(H, W)
    kw = {}
    if with_add:
        add = dev(rnd(rng, B, Cout, fh, fw))
        kw = dict(add=add, add_off=(0, 0))
    full = conv(dev(x), anchor=(0, 0), **kw)
    ref_pool = ops.maxpool2x2(full)
    hp = host(ref_pool)
    ref_mask = eq_bits(host(full), hp)
    assert int((ref_mask == 15).sum()) > 0                      # ReLU ties: several bits per byte
    win = conv.pool_window(H, W, None, c8=False, anchor=(0, 0))
    assert win == (0, 0, fh, fw)
    pooled = torch.full_like(ref_pool, -3.0)
    mask = torch.full(ref_pool.shape, 0xAA, dtype=torch.uint8, device='cuda')
    out = conv(dev(x), anchor=(0, 0), pool_out=pooled, mask_out=mask, **kw)
    assert np.array_equal(host(out), host(full))
    assert np.array_equal(host(pooled), hp) and np.array_equal(mask.cpu().numpy(), ref_mask)
    pooled.fill_(-3.0)
    mask.fill_(0x55)
    assert conv(dev(x), anchor=(0, 0), pool_out=pooled, mask_out=mask, store_out=False, **kw) is None
    assert np.array_equal(host(pooled), hp) and np.array_equal(mask.cpu().numpy(), ref_mask)
    # windows widened to whole pooling windows, written in place (refinement-loop windows)
    for region in [(3, 5, 4, 6), (0, 1, fh, 3), (fh - 3, fw - 4, 3, 4), (2, 2, 1, 1)]:
        y0, x0, h, ww = win = conv.pool_window(H, W, region, c8=False, anchor=(0, 0))
        pool2 = torch.full_like(ref_pool, -3.0)
        mask = torch.full(ref_pool.shape, 0xAA, dtype=torch.uint8, device='cuda')
        buf = torch.full_like(full, -5.0)
        wkw = dict(kw, add_off=(y0, x0)) if with_add else {}
        conv(dev(x), window=win, out=buf, place=(y0, x0), anchor=(0, 0), pool_out=pool2,
             mask_out=mask, **wkw)
        exp_p = np.full(hp.shape, -3.0, np.float32)
        exp_m = np.full(hp.shape, 0xAA, np.uint8)
        q = (slice(None), slice(None), slice(y0 // 2, (y0 + h) // 2), slice(x0 // 2, (x0 + ww) // 2))
        exp_p[q], exp_m[q] = hp[q], ref_mask[q]
        assert np.array_equal(host(pool2), exp_p), region
        assert np.array_equal(mask.cpu().numpy(), exp_m), region
        assert np.array_equal(host(buf)[:, :, y0:y0 + h, x0:x0 + ww], host(full)[:, :, y0:y0 + h, x0:x0 + ww])


def test_odd_anchor_pools_with_the_mask_pool_kernel(ops):
    """At an odd tile anchor the layer refuses the fused pool (no anchor parity is changed); the
    pool kernel's byte form gives the same pooled map as maxpool2x2 and the bytes of pre == pooled,
    for the full map and a window."""
    rng = np.random.default_rng(7)
    B, Cin, H, W, Cout = 2, 128, 23, 24, 128
    conv = ops.Conv(rnd(rng, Cout, Cin, 3, 3) * 0.05, rnd(rng, Cout), pad=1, relu=True)
    assert conv.pool_window(H, W, None, c8=False, anchor=(1, 1)) is None
    full = conv(dev(rnd(rng, B, Cin, H, W)), anchor=(1, 1))
    fh, fw = full.shape[2:]
    pooled = torch.empty((B, Cout, fh // 2, fw // 2), device='cuda')
    pooled.fill_(-3.0)
    with pytest.raises(RuntimeError):
        conv(dev(rnd(rng, B, Cin, H, W)), anchor=(1, 1), pool_out=pooled)
    ref = host(ops.maxpool2x2(full))
    mask = torch.full(pooled.shape, 0xAA, dtype=torch.uint8, device='cuda')
    got = ops.maxpool2x2(full, mask=mask)
    assert np.array_equal(host(got), ref) and np.array_equal(mask.cpu().numpy(), eq_bits(host(full), ref))
    pool2 = torch.full_like(pooled, -3.0)
    mask.fill_(0xAA)
    ops.maxpool2x2(full, out=pool2, window=(2, 3, 4, 5), mask=mask)
    exp_p = np.full(ref.shape, -3.0, np.float32)
    exp_m = np.full(ref.shape, 0xAA, np.uint8)
    exp_p[:, :, 2:6, 3:8] = ref[:, :, 2:6, 3:8]
    exp_m[:, :, 2:6, 3:8] = eq_bits(host(full), ref)[:, :, 2:6, 3:8]
    assert np.array_equal(host(pool2), exp_p) and np.array_equal(mask.cpu().numpy(), exp_m)


# B, C, H, W (unpooled size), Cout: small maps run the per-tile input transform, >= 128 tiles per
# image with a good fill the LDS-staged one; both tile-anchor parities (patch-origin parity)
UNPOOL_CASES = [(2, 128, 26, 26, 128), (1, 128, 13, 15, 256), (2, 128, 58, 58, 128), (1, 256, 60, 61, 128)]


@pytest.mark.parametrize('anchor', [(0, 0), (1, 1), (0, 1)])
@pytest.mark.parametrize('case', UNPOOL_CASES)
def test_wino_unpool_from_mask_bytes_is_bit_identical(ops, case, anchor):
    B, Cc, H, W, Cout = case
    rng = np.random.default_rng(hash(case) % 2**32)
    pre = np.maximum(rnd(rng, B, Cc, H, W), 0)                  # post-ReLU map: ties at 0
    h2, w2 = H // 2, W // 2
    pooled = pre[:, :, :2 * h2, :2 * w2].reshape(B, Cc, h2, 2, w2, 2).max(axis=(3, 5))
    up = rnd(rng, B, Cc, h2, w2)
    conv = ops.Conv(rnd(rng, Cout, Cc, 3, 3) * 0.05, rnd(rng, Cout), pad=1, relu=False)
    assert conv.wino and conv.mask_ok()
    mask = torch.from_numpy(eq_bits(pre, pooled)).cuda()
    ref = conv(dev(up), pre=dev(pre), pooled=dev(pooled), anchor=anchor)
    got = conv(dev(up), mask_in=mask, unpool_hw=(H, W), anchor=anchor)
    assert np.array_equal(host(got), host(ref))
    add = rnd(rng, B, Cout, H + 3, W + 2)
    for (y0, x0, h, ww) in [(1, 2, 9, 11), (0, 0, H, 5), (H - 4, W - 7, 4, 7)]:
        kw = dict(window=(y0, x0, h, ww), add=dev(add), add_off=(y0 + 1, x0), anchor=anchor)
        ref = conv(dev(up), pre=dev(pre), pooled=dev(pooled), **kw)
        got = conv(dev(up), mask_in=mask, unpool_hw=(H, W), **kw)
        assert np.array_equal(host(got), host(ref)), (y0, x0, h, ww)


@pytest.mark.parametrize('knobs', [{}, {'dce': False}, {'licm': False}, {'fold_border': False}])
def test_configs1_refinement_is_bit_identical_with_the_winograd_pool_on_and_off(built_lib, knobs,
                                                                                 monkeypatch):
    """BASELINE configs[1] (FCN-8 + 64-filter DAE, 224 x 224) at batch 2: refined map, iteration
    counts, norms and the first reconstruction, plus a one-shot DAE call, with the Winograd pool /
    mask bytes on against IISEG_DEPOOL_MASKS=0 + IISEG_WINO_POOL_FUSE=0 (pre / pooled maps, the pool
    kernel) -- over two batches (the second on the reused border-folded session)."""
    from iterative_inference_segm_amd import ops as _ops
    from iterative_inference_segm_amd import synthetic as S
    from iterative_inference_segm_amd.api import IterativeInference
    from iterative_inference_segm_amd.dae import StandardDAE
    from iterative_inference_segm_amd.fcn8 import FCN8
    fp = S.make_fcn8_params(seed=1234)
    dp = S.make_dae_params(seed=4321)
    B = 2

    def make(on):
        monkeypatch.setattr(_ops, 'WINO_POOL_FUSE', on)
        ii = IterativeInference(FCN8(fp, 11, layer=['pool4', 'probs_dimshuffle']),
                                StandardDAE(dp, 11, concat_h=['pool4'], n_filters=64), 11, [11])
        ii.dae.use_masks = on
        for k, v in knobs.items():
            setattr(ii.dae, k, v)
        ii.prepare(B, 224, 224)
        return ii
    ii_on, ii_off = make(True), make(False)
    monkeypatch.setattr(_ops, 'WINO_POOL_FUSE', True)
    assert ii_on.dae._mask_levels(False) >= frozenset((3, 4, 5, 6))
    for i in range(2):
        X = S.make_images(B, 224, 224, seed=510 + i)
        monkeypatch.setattr(_ops, 'WINO_POOL_FUSE', True)
        o1 = ii_on.pred_fcn_fn(X)
        r1 = ii_on.refine(o1[:-1], o1[-1], 0.1, 4, first_reconstruction=True)
        monkeypatch.setattr(_ops, 'WINO_POOL_FUSE', False)
        o0 = ii_off.pred_fcn_fn(X)
        r0 = ii_off.refine(o0[:-1], o0[-1], 0.1, 4, first_reconstruction=True)
        for a, b in zip(o1, o0):
            assert np.array_equal(arr(a), arr(b)), 'fcn batch %d' % i
        for a, b in zip(r1, r0):
            assert np.array_equal(arr(a), arr(b)), 'refine batch %d' % i
    monkeypatch.setattr(_ops, 'WINO_POOL_FUSE', True)
    s1 = ii_on.dae.scores(list(o1[:-1]), o1[-1])
    monkeypatch.setattr(_ops, 'WINO_POOL_FUSE', False)
    s0 = ii_off.dae.scores(list(o0[:-1]), o0[-1])
    assert np.array_equal(host(s1), host(s0))
