"""GPU: the streaming input transform of the fp32 Winograd layers (include/iiseg.h,
iiseg_conv_wino_input_wide; four tiles per thread, 16-byte stores) against the per-tile and LDS-staged
kernels it replaces: the whole workspace -- V with its padding, pre-filled with a sentinel, and the products
behind it -- and the conv output are the same, byte for byte, with the switch off and on."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -7777.25


@pytest.fixture(scope='module')
def ops(built_lib):
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from iterative_inference_segm_amd import ops as _ops
    return _ops


def rnd(rng, *shape):
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda()


def make_conv(ops, rng, cin, cout=32):
    conv = ops.Conv(rnd(rng, cout, cin, 3, 3) * 0.1, rnd(rng, cout), pad=1, relu=True)
    conv.wino = True            # (the width rule keeps such narrow layers off the form: forced here)
    return conv


def run_both(ops, monkeypatch, conv, *args, **kw):
    """conv(*args, **kw) with the old and the new input kernels; returns the kernel each one ran
    (iiseg_conv_wino_input_path) after asserting equal workspaces and outputs."""
    lib = conv.lib
    paths = []
    staged = ops._launch_staged

    def spy(fn, a, whole, stages):
        assert fn in (lib.iiseg_conv_wino_f32, lib.iiseg_conv_wino_mask_f32)
        mb = fn is lib.iiseg_conv_wino_mask_f32 and a[5] is not None
        paths.append(lib.iiseg_conv_wino_input_path(a[0], int(mb)))
        return staged(fn, a, whole, stages)
    monkeypatch.setattr(ops, '_launch_staged', spy)
    before = lib.iiseg_conv_wino_input_wide(-1)
    got = []
    try:
        conv(*args, **kw)                                   # sizes the workspace (and packs U)
        ws = ops.workspace_refs(args[0].device)[0]
        n = int(lib.iiseg_conv_wino_workspace_elems(C.byref(conv._describe_call(*args, **kw).d)))
        assert 0 < n <= ws.numel()
        for on in (False, True):
            assert ops.wino_input_wide(on, force=True) is on     # (forced: these launches have few tiles)
            ws.fill_(SENTINEL)
            out = conv(*args, **kw)
            torch.cuda.synchronize()
            got.append((ws[:n].clone().view(torch.int32), out.clone()))
    finally:
        lib.iiseg_conv_wino_input_wide(before)
        monkeypatch.setattr(ops, '_launch_staged', staged)
    assert len(paths) == 3 and paths[1] in (0, 1), paths
    assert torch.equal(got[0][0], got[1][0]), 'workspace (V, padding, products) differs'
    assert torch.equal(got[0][1].view(torch.int32), got[1][1].view(torch.int32))
    assert int((got[1][0] == got[1][0].new_tensor(np.float32(SENTINEL).view(np.int32))).sum()) > 0
    return paths[1], paths[2]


# map, window (y0, x0, h, w) or None, anchor: tile rows of 17 and 29 (odd; the second fills the LDS-staged
# kernel's chunks well enough to run it), 5 and 7 tiles (per-tile kernel, T no multiple of 256), 6 tiles;
# an odd window origin; a window ending at the last row and column of the map (pad taps)
PLAIN_CASES = [(34, None, (0, 0)), (58, None, (0, 0)), (10, None, (0, 0)), (13, None, (0, 0)), (13, None, (1, 1)),
               (34, (3, 5, 12, 12), (1, 1)), (34, (21, 19, 13, 15), (0, 0)), (13, (1, 1, 10, 10), (1, 1))]


@pytest.mark.parametrize('cin', [16, 32])
@pytest.mark.parametrize('idx', range(len(PLAIN_CASES)))
def test_plain_input_is_byte_identical(ops, monkeypatch, idx, cin):
    hw, window, anchor = PLAIN_CASES[idx]
    rng = np.random.default_rng(1000 * cin + idx)
    conv = make_conv(ops, rng, cin)
    x = rnd(rng, 2, cin, hw, hw)
    kw = dict(anchor=anchor)
    if window:
        kw['window'] = window
    old, new = run_both(ops, monkeypatch, conv, x, **kw)
    assert new == 2
    if hw == 58:
        assert old == 1


@pytest.mark.parametrize('hw', [34, 13])
def test_two_source_concat_is_byte_identical(ops, monkeypatch, hw):
    """C1 + C2 = 32 with neither a multiple of the channels a thread or a workgroup takes."""
    rng = np.random.default_rng(11 + hw)
    conv = make_conv(ops, rng, 32)
    x1, x2 = rnd(rng, 2, 13, hw, hw), rnd(rng, 2, 19, hw, hw)
    assert run_both(ops, monkeypatch, conv, x1, x2, anchor=(0, 0))[1] == 2
    assert run_both(ops, monkeypatch, conv, x1, x2, anchor=(1, 0), window=(2, 1, hw - 4, hw - 3))[1] == 2


def pooled_pair(rng, B, Cc, H, W):
    """A post-ReLU map, its 2x2 max-pool and the mask bytes (ties at 0: several bits per byte)."""
    pre = torch.clamp(rnd(rng, B, Cc, H, W), min=0)
    h2, w2 = H // 2, W // 2
    blocks = pre[:, :, :2 * h2, :2 * w2].reshape(B, Cc, h2, 2, w2, 2)
    pooled = blocks.amax(dim=(3, 5))
    eq = (blocks == pooled[:, :, :, None, :, None]).to(torch.uint8)
    mask = eq[:, :, :, 0, :, 0] | (eq[:, :, :, 0, :, 1] << 1) | (eq[:, :, :, 1, :, 0] << 2) | (eq[:, :, :, 1, :, 1] << 3)
    assert int((mask == 15).sum()) > 0
    return pre, pooled.contiguous(), mask.contiguous()


@pytest.mark.parametrize('anchor', [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize('hw', [(34, 35), (13, 10)])
def test_depool_input_is_byte_identical_for_every_patch_parity(ops, monkeypatch, hw, anchor):
    """DePool2D input from mask bytes (the streaming kernel) and from pre / pooled (which keeps the older
    kernels under both settings), all four patch-origin parities, odd unpooled sizes."""
    H, W = hw
    rng = np.random.default_rng(1000 * H + 10 * anchor[0] + anchor[1])
    conv = make_conv(ops, rng, 16)
    assert conv.mask_ok()
    pre, pooled, mask = pooled_pair(rng, 2, 16, H, W)
    up = rnd(rng, 2, 16, H // 2, W // 2)
    old, new = run_both(ops, monkeypatch, conv, up, mask_in=mask, unpool_hw=(H, W), anchor=anchor)
    assert new == 2
    win = (1, 2, H - 3, W - 2)
    assert run_both(ops, monkeypatch, conv, up, mask_in=mask, unpool_hw=(H, W), anchor=anchor, window=win)[1] == 2
    old, new = run_both(ops, monkeypatch, conv, up, pre=pre, pooled=pooled, anchor=anchor)
    assert new == old
    ref = conv(up, pre=pre, pooled=pooled, anchor=anchor)
    assert torch.equal(conv(up, mask_in=mask, unpool_hw=(H, W), anchor=anchor), ref)


# The streaming kernel's quads run over the tiles of ALL images laid end to end, so what its last quad
# holds depends on T = B * tiles per image modulo 4, and a workgroup of 1024 tiles covers many small images.
# B, map, anchor -> tiles per image, T mod 4: (3, 10) 25, 3; (5, 10) 25, 1; (3, 13) 49, 3; (5, 13) 49, 1;
# (7, 13, odd anchor) 49, 3.  T = 1125 (B = 45, 10 x 10) takes two workgroups, the first one spanning 41
# images and ending inside one, the second ending on a quad of one tile.
MANY_IMAGE_CASES = [(3, 10, (0, 0)), (5, 10, (0, 0)), (3, 13, (0, 0)), (5, 13, (0, 0)), (7, 13, (1, 1)),
                    (45, 10, (0, 0))]


@pytest.mark.parametrize('idx', range(len(MANY_IMAGE_CASES)))
def test_last_quad_of_1_and_3_tiles_and_many_images_per_workgroup(ops, monkeypatch, idx):
    B, hw, anchor = MANY_IMAGE_CASES[idx]
    rng = np.random.default_rng(7000 + idx)
    conv = make_conv(ops, rng, 16)
    x = rnd(rng, B, 16, hw, hw)
    nt = (hw + 1 + (anchor[0] & 1)) // 2
    assert (B * nt * nt) % 4 in (1, 3) and B >= 3
    assert run_both(ops, monkeypatch, conv, x, anchor=anchor)[1] == 2
    # the same from mask bytes (unpooled size hw x hw, odd sizes leave a last row / column without a byte)
    pre, pooled, mask = pooled_pair(rng, B, 16, hw, hw)
    up = rnd(rng, B, 16, hw // 2, hw // 2)
    assert run_both(ops, monkeypatch, conv, up, mask_in=mask, unpool_hw=(hw, hw), anchor=anchor)[1] == 2
    # concat: the image stride differs between the two sources
    x1, x2 = rnd(rng, B, 5, hw, hw), rnd(rng, B, 11, hw, hw)
    assert run_both(ops, monkeypatch, conv, x1, x2, anchor=anchor)[1] == 2
