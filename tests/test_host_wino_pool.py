"""CPU: the planner puts the max-pool and the DePool2D mask bytes on the fp32 Winograd layers of the
bench workload (BASELINE configs[1]: FCN-8 + the 64-filter DAE).  Layers are built on the host; no
GPU, no launches."""
import pytest
import torch


@pytest.fixture(scope='module')
def dae(built_lib):
    from iterative_inference_segm_amd import synthetic as S
    from iterative_inference_segm_amd.dae import StandardDAE
    dp = S.make_dae_params(seed=4321)
    return StandardDAE(dp, 11, concat_h=['pool4'], padding=100, n_filters=64, additional_pool=2,
                       skip=True, unpool_type='trackind', device='cpu', dtype=torch.float32)


def _enc(dae, L):
    name = 'conv%d_1' % L
    return dae.hsplit[name][1] if name in dae.hsplit else dae.enc[name]


def test_configs1_levels_3_to_6_carry_byte_masks(dae):
    """Levels 1-2 (halo kernels) and 3-6 (Winograd; level 5 is the split h-concat, pooled after the
    h-half is added) all travel as mask bytes."""
    assert dae.total == 6
    assert all(_enc(dae, L).wino for L in (3, 4, 5, 6))
    assert dae._mask_levels(False) == frozenset(range(1, 7))
    for L in (3, 4, 5, 6):
        assert _enc(dae, L).mask_ok(False) and dae.dec['up_conv%d' % L].mask_ok(False)


def test_winograd_pool_fuses_only_at_an_even_tile_anchor(dae):
    """A 2x2 Winograd tile is one pooling window only at an even anchor; at an odd one the layer
    keeps storing its map (the pool kernel writes pooled map + bytes), so no anchor parity changes."""
    for L in (3, 4, 5, 6):
        conv = _enc(dae, L)
        assert not conv.pool_fusable(False)                      # no anchor given: no promise
        assert conv.pool_fusable(False, (0, 0)) and conv.pool_fusable(False, (10, 4))
        assert not conv.pool_fusable(False, (23, 23)) and not conv.pool_fusable(False, (0, 1))
        assert conv.pool_window(33, 33, None, c8=False, anchor=(1, 1)) is None
        fh, fw = conv.out_hw(33, 33)
        assert conv.pool_window(33, 33, None, c8=False, anchor=(0, 0)) == (0, 0, fh, fw)
        assert conv.pool_window(33, 33, (3, 5, 4, 6), c8=False, anchor=(0, 0)) == (2, 4, 6, 8)


def test_switches_turn_the_winograd_forms_off(dae, monkeypatch):
    """IISEG_WINO_POOL_FUSE=0 / IISEG_DEPOOL_MASKS=0 / IISEG_FUSE_UNPOOL=0: the A/B controls."""
    from iterative_inference_segm_amd import ops
    monkeypatch.setattr(ops, 'WINO_POOL_FUSE', False)
    assert dae._mask_levels(False) == frozenset((1, 2))
    assert not _enc(dae, 4).pool_fusable(False, (0, 0))
    monkeypatch.setattr(ops, 'WINO_POOL_FUSE', True)
    monkeypatch.setattr(dae, 'use_masks', False)
    assert dae._mask_levels(False) == frozenset()
    monkeypatch.setattr(dae, 'use_masks', True)
    monkeypatch.setattr(dae, 'fuse_unpool', False)
    assert dae._mask_levels(False) == frozenset()


def test_wino_pool_query_needs_whole_windows_at_an_even_anchor(built_lib):
    """iiseg_conv_wino_pool_supported: even tile anchor, even window origin, even extent unless the
    window ends at the map's last row / column; calls without operands return statuses, no launch."""
    import ctypes as C
    from iterative_inference_segm_amd import _lib
    lib = _lib.load()
    d = _lib.ConvDesc()
    d.B, d.C1, d.C2, d.H, d.W, d.Cout, d.KH, d.KW, d.pad, d.dil = 1, 128, 0, 13, 13, 128, 3, 3, 1, 1
    d.OH, d.OW = 13, 13
    assert lib.iiseg_conv_wino_supported(C.byref(d)) == 1
    assert lib.iiseg_conv_wino_pool_supported(C.byref(d)) == 1       # odd extent ending at the edge
    d.tile_y0 = 1
    assert lib.iiseg_conv_wino_pool_supported(C.byref(d)) == 0       # odd anchor
    d.tile_y0 = 0
    d.oy0, d.OH = 1, 12
    assert lib.iiseg_conv_wino_pool_supported(C.byref(d)) == 0       # odd origin
    d.oy0, d.OH = 2, 5
    assert lib.iiseg_conv_wino_pool_supported(C.byref(d)) == 0       # cuts a pooling window
    d.oy0, d.OH = 2, 6
    assert lib.iiseg_conv_wino_pool_supported(C.byref(d)) == 1
    assert lib.iiseg_conv_wino_mask_f32(None, C.byref(d), *([None] * 12), 7) == -1   # IISEG_ERR_NULL
    d.C1 = 20
    assert lib.iiseg_conv_wino_pool_supported(C.byref(d)) == 0
    assert lib.iiseg_conv_wino_mask_f32(None, C.byref(d), *([None] * 12), 7) == -5
    assert lib.iiseg_maxpool2x2_mask_window_f32(None, None, None, None, 1, 4, 4, 0, 0, 2, 2) == -1
