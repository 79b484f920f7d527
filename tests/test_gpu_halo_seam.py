"""GPU: the fp32 halo-tile kernel's column tiles across the image seam (csrc/conv_halo.hip, SEAM;
include/iiseg.h iiseg_conv_halo_seam).  The tiling changes WHICH workgroup computes a pixel, never what
is summed into it or in what order: every launch here runs twice through ops.Conv, seam tiling on and
off (one tile grid per image), and every output -- the map, the pooled map, the mask bytes -- must be
equal bit for bit.  Inputs are random fp32 (integers would hide a change of summation order); outputs
are pre-filled, so a pixel that is not written, or one written outside the window, shows as well."""
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


def rnd(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


def both_tilings(ops, run, expect_seam):
    """run() -> tuple of output tensors, under the per-image tiling and under the seam tiling; asserts
    that the seam tiling really ran (or, for the fall-back cases, that it did not) and that all outputs
    are equal bit for bit."""
    before = ops.halo_seam()
    try:
        assert ops.halo_seam(False) is False
        n0 = ops.halo_seam_launches()
        ref = run()
        assert ops.halo_seam_launches() == n0
        assert ops.halo_seam(True) is True
        got = run()
        torch.cuda.synchronize()
        assert (ops.halo_seam_launches() > n0) == expect_seam
    finally:
        ops.halo_seam(before)
    assert len(ref) == len(got)
    for r, g in zip(ref, got):
        assert r.shape == g.shape and r.dtype == g.dtype
        assert torch.equal(r, g), 'seam tiling differs from the per-image tiling in %d elements' % int((r != g).sum())
    return got


# (Cin, Cout): BM = 64, TH = 8 with a padded k-tile (11 = 2 * 4 + 3 channels); BM = 128, TH = 4
CHANNELS = [(11, 64), (64, 128)]
# (B, OH, OW): a seam in nearly every tile, at both parities, last tile partial (99 columns);
# even width, five tiles instead of eight
SHAPES = [(3, 9, 33), (4, 10, 40)]


@pytest.mark.parametrize('channels', CHANNELS)
@pytest.mark.parametrize('shape', SHAPES)
def test_plain_layer(ops, channels, shape):
    (Cin, Cout), (B, H, W) = channels, shape
    rng = np.random.default_rng(1000 * Cin + W)
    x, w, b = dev(rnd(rng, B, Cin, H, W)), rnd(rng, Cout, Cin, 3, 3) * 0.1, rnd(rng, Cout)
    conv = ops.Conv(w, b, pad=1, relu=False)
    assert conv.kernel == 'conv_halo_f32_kernel' and not conv.wino

    def run():
        out = torch.full((B, Cout, H, W), -7.0, device='cuda')
        conv(x, out=out)
        return (out,)
    out, = both_tilings(ops, run, True)
    assert not bool((out == -7.0).any())


@pytest.mark.parametrize('channels', CHANNELS)
@pytest.mark.parametrize('shape', SHAPES)
def test_pool_and_mask_bytes(ops, channels, shape):
    """The fused 2x2 max-pool and the mask bytes.  Even OW: the seam falls on an even tile column and no
    pair straddles it.  Odd OW (33: the last column has no pooling window): the per-image tiling runs,
    whatever the switch says."""
    (Cin, Cout), (B, H, W) = channels, shape
    rng = np.random.default_rng(2000 * Cin + W)
    x, w, b = dev(rnd(rng, B, Cin, H, W)), rnd(rng, Cout, Cin, 3, 3) * 0.1, rnd(rng, Cout)
    conv = ops.Conv(w, b, pad=1, relu=True)
    assert conv.pool_window(H, W, None) == (0, 0, H, W)

    def run():
        out = torch.full((B, Cout, H, W), -7.0, device='cuda')
        pooled = torch.full((B, Cout, H // 2, W // 2), -3.0, device='cuda')
        mask = torch.full((B, Cout, H // 2, W // 2), 0xA0, dtype=torch.uint8, device='cuda')
        conv(x, out=out, pool_out=pooled, mask_out=mask)
        pooled2 = torch.full_like(pooled, -3.0)
        mask2 = torch.full_like(mask, 0x50)
        assert conv(x, pool_out=pooled2, mask_out=mask2, store_out=False) is None
        return out, pooled, mask, pooled2, mask2
    out, pooled, mask, pooled2, mask2 = both_tilings(ops, run, W % 2 == 0)
    assert torch.equal(pooled, torch.nn.functional.max_pool2d(out, 2)) and torch.equal(pooled, pooled2)
    assert torch.equal(mask, mask2) and int(mask.max()) <= 15 and int(mask.min()) >= 1


@pytest.mark.parametrize('mask_bytes', [True, False])
def test_decoder_layer(ops, mask_bytes):
    """up_conv2's form: 128 -> 64 over the DePool2D of `up` (mask bytes, or pre / pooled), a skip-add
    with crop, an odd window of 35 columns at an odd origin inside a larger map -- its halo reaches the
    last column, which has no pooling window -- placed inside a larger output, three images."""
    B, Cin, Cout, H, W = 3, 128, 64, 25, 47
    win = (3, 11, 11, 35)
    rng = np.random.default_rng(77)
    pre = rnd(rng, B, Cin, H, W)
    pre_t = dev(pre)
    pooled = torch.nn.functional.max_pool2d(pre_t, 2)
    up = dev(rnd(rng, B, Cin, H // 2, W // 2))
    mask = torch.zeros(pooled.shape, dtype=torch.uint8, device='cuda')
    for dy in (0, 1):
        for dx in (0, 1):
            eq = pre_t[:, :, dy:2 * (H // 2):2, dx:2 * (W // 2):2] == pooled
            mask |= eq.to(torch.uint8) << (dy * 2 + dx)
    add = dev(rnd(rng, B, Cout, 16, 41))
    conv = ops.Conv(rnd(rng, Cout, Cin, 3, 3) * 0.05, rnd(rng, Cout), pad=1, relu=True)
    assert conv.kernel == 'conv_halo_f32_kernel' and not conv.wino
    src = dict(mask_in=mask, unpool_hw=(H, W)) if mask_bytes else dict(pre=pre_t, pooled=pooled)

    def run():
        big = torch.full((B, Cout, 20, 44), -7.0, device='cuda')
        conv(up, add=add, add_off=(2, 3), window=win, out=big, place=(4, 6), **src)
        return (big,)
    big, = both_tilings(ops, run, True)
    inside = big[:, :, 4:4 + win[2], 6:6 + win[3]]
    assert not bool((inside == -7.0).any()) and int((big == -7.0).sum()) == B * Cout * (20 * 44 - win[2] * win[3])


@pytest.mark.parametrize('sources', [(8, 5), (4, 9)])
def test_two_source_concat(ops, sources):
    """Two sources with different channel counts: their images are C1 and C2 planes apart, the second
    source's closer together (C2 < C1) or further apart (C2 > C1) than the first's."""
    (C1, C2), B, Cout, H, W = sources, 2, 64, 7, 34
    rng = np.random.default_rng(5 + C1)
    x1, x2 = dev(rnd(rng, B, C1, H, W)), dev(rnd(rng, B, C2, H, W))
    conv = ops.Conv(rnd(rng, Cout, C1 + C2, 3, 3) * 0.1, rnd(rng, Cout), pad=1, relu=True)

    def run():
        out = torch.full((B, Cout, H, W), -7.0, device='cuda')
        conv(x1, x2, out=out)
        return (out,)
    both_tilings(ops, run, True)


@pytest.mark.parametrize('shape', [(1, 10, 40), (3, 9, 31), (2, 8, 64)])
def test_launches_without_a_seam_keep_the_per_image_tiling(ops, shape):
    """One image; windows narrower than a tile (two seams could fall into one); a width that wastes no
    column: the per-image tiling runs and the results are what they were."""
    B, H, W = shape
    rng = np.random.default_rng(W)
    x = dev(rnd(rng, B, 11, H, W))
    conv = ops.Conv(rnd(rng, 64, 11, 3, 3) * 0.1, rnd(rng, 64), pad=1, relu=True)

    def run():
        out = torch.full((B, 64, H, W), -7.0, device='cuda')
        pooled = torch.full((B, 64, H // 2, W // 2), -3.0, device='cuda')
        if W % 2 == 0:
            conv(x, out=out, pool_out=pooled)
        else:
            conv(x, out=out)
        return out, pooled
    both_tilings(ops, run, False)
