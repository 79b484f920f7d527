"""CPU: which fp32 kernel runs each case of test_gpu_conv_fallbacks.py and of test_gpu_ops.py::CONV_CASES.

The expectations (tests/conv_fallback_cases.py) were worked out by hand from the tile shapes in
csrc/conv_igemm.hip, conv_taps.hip, conv_halo.hip, conv_small.hip and from the cost model of
`gemm_conv_geom` (csrc/conv_wino.hip); the library answers from the dispatch its launches go through
(iiseg_conv_direct_kernel) and from iiseg_conv_gemm_workspace_elems.  The day a case moves to another
kernel, this file's table has to change with it -- and the case that was meant to pin the old kernel needs
a new shape."""
import ctypes as C

import pytest
import torch

import conv_fallback_cases as K


def _conv(c):
    from iterative_inference_segm_amd import ops
    shape = (c.C1 + c.C2, c.Cout, c.k, c.k) if c.transposed else (c.Cout, c.C1 + c.C2, c.k, c.k)
    conv = ops.Conv(torch.zeros(shape), torch.zeros(c.Cout), pad=c.pad, relu=c.relu, dil=c.dil,
                    layout='iohw' if c.transposed else 'oihw', device='cpu', transposed=c.transposed, mma='f32')
    conv.wino = False
    return conv


def _launch(conv, c, placed):
    meta = lambda name, shape: torch.empty(shape, device='meta', dtype=torch.float32)
    g = K.geometry(c, placed)
    return conv._describe_call(meta('x1', g['x1']), **K.call_kwargs(g, meta))


def _route(conv, launch):
    tiles = (C.c_int32 * 4)()
    family = conv.lib.iiseg_conv_direct_kernel(C.byref(launch.d), int(launch.add is not None),
                                               int(conv.b is not None), tiles)
    return (family,) + tuple(tiles)


def _split_k(conv, d):
    """S from iiseg_conv_gemm_workspace_elems = Tpad * (Kpad + S * Mpad)."""
    T = d.B * d.OH * d.OW
    Tpad = (T + 127) // 128 * 128
    per_pixel, rem = divmod(conv.lib.iiseg_conv_gemm_workspace_elems(C.byref(d)), Tpad)
    S, rem2 = divmod(per_pixel - d.Kpad, d.Mpad)
    assert rem == 0 and rem2 == 0
    return S


ALL = K.FALLBACK_CASES + K.OPS_CONV_CASES


def test_case_names_are_unique():
    assert len({c.name for c in ALL}) == len(ALL)


def test_the_rows_of_conv_cases_are_the_cases_of_test_gpu_ops():
    from test_gpu_ops import CONV_CASES
    rows = [(c.B, c.C1, c.H, c.W, c.Cout, c.k, c.pad, c.dil, c.relu) for c in K.OPS_CONV_CASES]
    assert rows == CONV_CASES and not any(c.C2 or c.window or c.add or c.unpool for c in K.OPS_CONV_CASES)


@pytest.mark.parametrize('c', ALL, ids=lambda c: c.name)
def test_case_takes_the_kernel_it_is_meant_to_pin(built_lib, c):
    if K.switched_off(c):
        pytest.skip('%s is not at its default' % K.switched_off(c))
    conv = _conv(c)
    for placed in sorted({None, c.placed if c.placed != 'guard' else None}, key=str):
        launch = _launch(conv, c, placed)
        assert _route(conv, launch) == c.route, placed
        if c.S is None:
            assert conv._form(launch) == 'direct', placed
        else:
            assert conv._form(launch) == 'gemm_f32' and _split_k(conv, launch.d) == c.S


LABELS = {K.SMALL: 'conv_small_f32_kernel', K.HALO: 'conv_halo_f32_kernel', K.HALO16: 'conv_halo_f32_kernel',
          K.TAPS: 'conv_taps_f32_kernel', K.IGEMM: 'conv_igemm_f32_kernel'}


@pytest.mark.parametrize('c', [c for c in ALL if c.S is None], ids=lambda c: c.name)
def test_profile_label_names_the_kernel_that_runs(built_lib, c, monkeypatch):
    """`Conv._direct_kernel` (the 'direct' form's profile label, restated in Python) against the dispatch."""
    if K.switched_off(c):
        pytest.skip('%s is not at its default' % K.switched_off(c))
    from iterative_inference_segm_amd import ops
    monkeypatch.setattr(ops, 'KERNEL_BYTES', {})       # (the label of conv_small comes with its byte count)
    conv = _conv(c)
    launch = _launch(conv, c, c.placed)
    assert conv._direct_kernel(launch.d, launch.add) == LABELS[_route(conv, launch)[0]]


def test_split_k_does_not_depend_on_the_batch(built_lib):
    """`gemm_conv_geom` chooses S for a nominal pixel count: an image is summed in the same order alone and
    in any batch."""
    for c in K.GEMM_CASES:
        conv = _conv(c)
        for B in (1, 2, 64):
            launch = _launch(conv, c._replace(B=B), None)
            assert conv._form(launch) == 'gemm_f32' and _split_k(conv, launch.d) == c.S, (c.name, B)


def test_the_query_refuses_what_the_launch_refuses(built_lib):
    from iterative_inference_segm_amd import _lib
    conv = _conv(K.IGEMM_CASES[0])
    d = _launch(conv, K.IGEMM_CASES[0], None).d
    tiles = (C.c_int32 * 4)()
    q = conv.lib.iiseg_conv_direct_kernel
    assert q(None, 0, 1, tiles) == -1                               # IISEG_ERR_NULL
    assert q(C.byref(d), 0, 1, None) == -1
    bad = _lib.ConvDesc.from_buffer_copy(d)
    bad.OH += 1                                                     # window outside the output map
    assert q(C.byref(bad), 0, 1, tiles) == -2                       # IISEG_ERR_SHAPE
    bad = _lib.ConvDesc.from_buffer_copy(d)
    bad.Kpad += 16                                                  # not the planned packing
    assert q(C.byref(bad), 0, 1, tiles) == -2
    assert q(C.byref(d), 1, 1, tiles) == -2                         # a skip-add smaller than the window (AH = 0)
    assert q(C.byref(d), 0, 1, tiles) == K.IGEMM


def test_every_launched_instantiation_has_a_case():
    """Every (filter, BM, BN, UNPOOL) instantiation that launch_conv and iiseg_launch_conv_taps can launch
    with the default switches (a negative filter size: transposed), and both tiles of the GEMM form."""
    igemm = {(c.route[1], c.route[2], c.unpool) for c in K.IGEMM_CASES}
    assert igemm == {(bm, bn, u) for bm, bn in ((32, 256), (64, 256), (128, 128)) for u in (False, True)}
    tiles = {1: ((32, 256), (64, 256), (128, 128)), 3: ((32, 256), (64, 256), (128, 128)),
             4: ((32, 128), (64, 128), (128, 128))}
    taps = {(k, bm, bn, u) for k in tiles for bm, bn in tiles[k] for u in (False, True)} | {(3, 256, 128, False)}
    got = {(c.k, c.route[1], c.route[2], c.unpool) for c in K.TAPS_CASES}
    # (the plain 4x4 tile of 128 channels: test_gpu_e2e.py::test_unpool_type_standard_and_inverse)
    assert got == taps - {(4, 128, 128, False)}
    # the transposed variants of the 3x3 and 4x4 tiles (the same instantiations, another tap pattern)
    assert {(c.k, c.route[1]) for c in K.TAPS_CASES if c.transposed} == {(3, 32), (3, 64), (3, 128), (4, 32), (4, 64)}
    # the GEMM form: its 128- and 256-channel tile, with and without split-K
    assert {(c.S, c.route[4] % 2 == 0) for c in K.GEMM_CASES} == {(2, False), (7, True), (5, True), (1, False)}
