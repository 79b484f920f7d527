"""GPU: the register diet of the fp32 Winograd GEMM tiles (include/iiseg.h, iiseg_conv_wino_gemm_slim) against the
form it replaces, the two-tile form of the streaming input transform (iiseg_conv_wino_input_narrow) against the
four-tile one, and a GEMM and an output transform of two layers running on two streams at once.

Every case calls `iiseg_conv_wino_f32` with its stages given explicitly (1 input transform, 2 GEMM, 4 output
transform), so the separate GEMM runs whatever Cin is.  V is written once; the products M (the whole region with
its padding rows and columns, pre-filled with a sentinel before each GEMM launch) and the final map must be
`np.array_equal` between `ops.wino_gemm_slim(False)` and `(True)`, under both layouts of M (`ops.wino_m_quad`).

Shapes: B = 2 on a 27 x 27 map.  A 7 x 5 window at the odd origin (3, 5) with anchor (1, 1) has 4 x 3 x 2 = 24 tiles,
well under one 128-tile column block; a 23 x 23 window has 12 x 12 x 2 = 288, three blocks, the last one partly
padding.  Cin = 32 is two k-tiles, the shortest loop with a prefetch; Cin = 16 one k-tile, no prefetch.  Cout = 130
leaves rows beyond Cout in the last channel quad; Cout = 256 is one 256-row block.  The launcher's last-round rule
(`tile_rows` restates it) runs all of these on 128 x 128 tiles, the switch for 256 x 128 being read from the
environment once per process; Cout = 768 with 288 tiles and Cout = 2304 with 24 (144 workgroups each) are the
smallest layers the rule itself gives 256 x 128 tiles, and they are here for that kernel."""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest
import torch
import torch.nn.functional as F

SENTINEL = -7777.25
HW = 27
WINDOWS = {'t24': ((3, 5, 7, 5), (1, 1), 24), 't288': ((2, 2, 23, 23), (0, 0), 288)}

Layer = namedtuple('Layer', 'conv d args n_v n_ws ws out x w b window')


@pytest.fixture(scope='module')
def ops(built_lib):
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from iterative_inference_segm_amd import ops as _ops
    return _ops


def tile_rows(cout, T):
    """Rows of the GEMM tile the launcher picks (conv_wino.hip, wino_run): 256 for Cout > 128 unless 128 x 128
    tiles fill the last round of 256 compute units better."""
    if cout <= 128:
        return 128 if cout > 64 else 64
    grid = 16 * ((T + 127) // 128) * ((cout + 255) // 256)
    return 128 if 0.5 * 1.06 * ((2 * grid + 255) // 256) < (grid + 255) // 256 else 256


def make_layer(ops, seed, B, cin, cout, hw, window, anchor, relu=True):
    """A 3x3 layer with its own workspace and output, described for `iiseg_conv_wino_f32`; U packed."""
    rng = np.random.default_rng(seed)
    f32 = lambda a: a.astype(np.float32)
    w = f32(rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin))
    b = f32(rng.standard_normal(cout))
    x = f32(rng.standard_normal((B, cin, hw, hw)))
    conv = ops.Conv(w, b, pad=1, relu=relu)
    xd = torch.from_numpy(x).cuda()
    out = torch.full((B, cout, window[2], window[3]), SENTINEL, device='cuda')
    c = conv._describe_call(xd, window=window, anchor=anchor, out=out)
    d, lib = c.d, conv.lib
    assert lib.iiseg_conv_wino_supported(C.byref(d))
    U = torch.empty(lib.iiseg_conv_wino_weight_elems(C.byref(d)), dtype=torch.float32, device='cuda')
    ops.check(lib.iiseg_conv_wino_pack_f32(ops._stream(), C.byref(d), ops._ptr(conv.W), conv.so, conv.sc, ops._ptr(U)),
              'iiseg_conv_wino_pack_f32')
    n_ws = int(lib.iiseg_conv_wino_workspace_elems(C.byref(d)))
    T = B * ((window[2] + 1) // 2) * ((window[3] + 1) // 2)
    Tpad = (T + 127) // 128 * 128
    assert n_ws % (16 * Tpad) == 0 and n_ws // (16 * Tpad) - cin >= cout
    ws = torch.full((n_ws,), SENTINEL, device='cuda')
    args = (C.byref(d), ops._ptr(xd), None, None, None, ops._ptr(U), ops._ptr(conv.b), None, ops._ptr(ws),
            ops._ptr(out))
    keep = (xd, U)
    return Layer((conv, keep), d, args, 16 * cin * Tpad, n_ws, ws, out, x, w, b, window)


def stage(ops, L, bits, stream=None):
    lib = L.conv[0].lib
    s = ops._stream() if stream is None else C.c_void_p(stream.cuda_stream)
    ops.check(lib.iiseg_conv_wino_f32(s, *L.args, bits), 'iiseg_conv_wino_f32 stages %d' % bits)


def gemm_and_output(ops, L):
    """M (bits) and the final map of `L` from a fresh GEMM and output launch; V stays as the input stage left it."""
    L.ws[L.n_v:].fill_(SENTINEL)
    L.out.fill_(SENTINEL)
    stage(ops, L, 2)
    stage(ops, L, 4)
    torch.cuda.synchronize()
    return L.ws[L.n_v:].cpu().numpy().view(np.int32), L.out.cpu().numpy()


GEMM_CASES = [(win, cin, cout) for win in ('t24', 't288') for cin in (32, 16) for cout in (130, 256)] + \
    [('t288', cin, 768) for cin in (32, 16)] + [('t24', cin, 2304) for cin in (32, 16)]


def test_the_cases_reach_both_gemm_tiles():
    """No GPU needed: by the launcher's rule the 768- and 2304-channel cases are the 256 x 128 ones."""
    rows = {(win, cout): tile_rows(cout, WINDOWS[win][2]) for win, _, cout in GEMM_CASES}
    assert all(r == (256 if cout > 256 else 128) for (win, cout), r in rows.items()), rows


@pytest.mark.gpu
@pytest.mark.parametrize('win,cin,cout', GEMM_CASES, ids=['%s-cin%d-cout%d' % c for c in GEMM_CASES])
def test_slim_gemm_gives_the_same_products_and_map(ops, win, cin, cout):
    window, anchor, T = WINDOWS[win]
    L = make_layer(ops, 100 * cout + cin + T, 2, cin, cout, HW, window, anchor)
    before = ops.wino_gemm_slim(), ops.wino_m_quad()
    got = {}
    try:
        stage(ops, L, 1)
        for quad in (False, True):
            assert ops.wino_m_quad(quad) is quad
            for slim in (False, True):
                assert ops.wino_gemm_slim(slim) is slim
                got[quad, slim] = gemm_and_output(ops, L)
    finally:
        ops.wino_gemm_slim(before[0])
        ops.wino_m_quad(before[1])
    for quad in (False, True):
        (m_old, y_old), (m_new, y_new) = got[quad, False], got[quad, True]
        assert np.array_equal(m_old, m_new), 'M differs (quad layout %s)' % quad
        assert np.array_equal(y_old.view(np.int32), y_new.view(np.int32)), 'the map differs (quad layout %s)' % quad
        assert int((m_new == np.float32(SENTINEL).view(np.int32)).sum()) == 0      # the GEMM wrote all of it
    assert np.array_equal(got[False, True][1], got[True, True][1])
    assert not np.array_equal(got[False, True][0], got[True, True][0])       # the two layouts are two layouts
    # and the map is the layer's: float64 on the CPU, the bound of a K-term fp32 chain with Winograd's constant
    y0, x0, wh, ww = window
    tt = lambda a: torch.from_numpy(a.astype(np.float64))
    ref = torch.clamp(F.conv2d(tt(L.x), tt(L.w), tt(L.b), padding=1), min=0)[:, :, y0:y0 + wh, x0:x0 + ww].numpy()
    err = float(np.abs(got[True, True][1] - ref).max())
    tol = 4 * 2.0 ** -18 * np.sqrt(9 * cin)
    print('cout %d cin %d %s: max |err| vs float64 %.3e (bound %.3e)' % (cout, cin, win, err, tol))
    assert err <= tol


# The streaming input transform with two tiles per thread (iiseg_conv_wino_input_narrow) against the four-tile form:
# stage 1 alone, V -- the whole region, sentinel-filled, so that a store at t >= T shows -- equal bit for bit.
# (B, H, W, anchor, forced): 3 x 13 x 13 is 7 x 7 x 3 = 147 tiles, fewer than 4096 (the streaming kernel only when
# forced) and odd, so T cuts the last quad after three tiles and the last pair after one; 7 x 49 x 49 at an odd anchor
# is 25 x 25 x 7 = 4375, odd again, what the default rule streams, nine workgroups of 512 tiles.
INPUT_MAPS = {'t147': (3, 13, 13, (0, 0), True), 't4375': (7, 49, 49, (1, 1), False)}
SPLITS = {16: (5, 11), 48: (13, 35)}


def input_case(ops, kind, cin, B, H, W, anchor, seed):
    """(fn, args, V's elements, workspace) of a layer whose input is plain / a two-source concat / DePool2D from
    mask bytes, for stage 1 of iiseg_conv_wino_f32 / iiseg_conv_wino_mask_f32."""
    rng = np.random.default_rng(seed)
    rnd = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda()
    conv = ops.Conv(rnd(32, cin, 3, 3) * 0.1, rnd(32), pad=1, relu=True)
    lib = conv.lib
    x2 = mask = None
    if kind == 'plain':
        x1 = rnd(B, cin, H, W)
        c = conv._describe_call(x1, anchor=anchor)
    elif kind == 'concat':
        x1, x2 = rnd(B, SPLITS[cin][0], H, W), rnd(B, SPLITS[cin][1], H, W)
        c = conv._describe_call(x1, x2, anchor=anchor)
    else:
        x1 = rnd(B, cin, H // 2, W // 2)
        mask = torch.from_numpy(rng.integers(0, 16, size=(B, cin, H // 2, W // 2)).astype(np.uint8)).cuda()
        c = conv._describe_call(x1, mask_in=mask, unpool_hw=(H, W), anchor=anchor)
    d = c.d
    assert lib.iiseg_conv_wino_supported(C.byref(d))
    U = torch.empty(lib.iiseg_conv_wino_weight_elems(C.byref(d)), dtype=torch.float32, device='cuda')
    ops.check(lib.iiseg_conv_wino_pack_f32(ops._stream(), C.byref(d), ops._ptr(conv.W), conv.so, conv.sc, ops._ptr(U)),
              'iiseg_conv_wino_pack_f32')
    n_ws = int(lib.iiseg_conv_wino_workspace_elems(C.byref(d)))
    T = B * ((H + 1 + anchor[0]) // 2) * ((W + 1 + anchor[1]) // 2)
    Tpad = (T + 127) // 128 * 128
    assert n_ws % (16 * Tpad) == 0
    ws = torch.full((n_ws,), SENTINEL, device='cuda')
    if kind == 'depool':
        fn = lib.iiseg_conv_wino_mask_f32
        args = (C.byref(d), ops._ptr(x1), None, None, None, ops._ptr(mask, torch.uint8), ops._ptr(U), ops._ptr(conv.b),
                None, ops._ptr(ws), ops._ptr(c.out), None, None)
    else:
        fn = lib.iiseg_conv_wino_f32
        args = (C.byref(d), ops._ptr(x1), ops._ptr(x2), None, None, ops._ptr(U), ops._ptr(conv.b), None, ops._ptr(ws),
                ops._ptr(c.out))
    return fn, args, 16 * cin * Tpad, ws, T, (conv, x1, x2, mask, U, c)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['plain', 'concat', 'depool'])
@pytest.mark.parametrize('cin', [16, 48])
@pytest.mark.parametrize('shape', sorted(INPUT_MAPS))
def test_narrow_input_transform_writes_the_same_v(ops, shape, cin, kind):
    B, H, W, anchor, forced = INPUT_MAPS[shape]
    fn, args, n_v, ws, T, keep = input_case(ops, kind, cin, B, H, W, anchor, 31 * cin + len(kind) + H)
    assert T == int(shape[1:]) and T % 2 == 1 and (T < 4096) == forced
    lib = keep[0].lib
    before = ops.wino_input_narrow(), lib.iiseg_conv_wino_input_wide(-1)
    got = []
    try:
        assert ops.wino_input_wide(True, force=forced) is True
        for narrow in (False, True):
            assert ops.wino_input_narrow(narrow) is narrow
            assert lib.iiseg_conv_wino_input_path(args[0], int(kind == 'depool')) == 2
            assert lib.iiseg_conv_wino_input_tiles(args[0], int(kind == 'depool')) == (2 if narrow else 4)
            ws.fill_(SENTINEL)
            ops.check(fn(ops._stream(), *args, 1), 'input stage')
            torch.cuda.synchronize()
            got.append(ws[:n_v].cpu().numpy().view(np.int32))
    finally:
        ops.wino_input_narrow(before[0])
        lib.iiseg_conv_wino_input_wide(before[1])
    assert np.array_equal(got[0], got[1]), 'V differs'
    sent = got[1].reshape(16 * cin, -1) == np.float32(SENTINEL).view(np.int32)
    assert not sent[:, :T].any() and sent[:, T:].all()          # every tile below T written, nothing from T on


@pytest.mark.gpu
def test_gemm_and_output_transform_of_two_layers_on_two_streams(ops):
    """The slim GEMM of layer A on one stream while the output transform of layer B -- prepared beforehand, with
    its own workspace -- runs on a second: M of A and the map of B are what the same two launches give one after
    the other.  (800 GEMM workgroups and 105 MB of products, enough for the two launches to meet on the chip.)"""
    before = ops.wino_gemm_slim()
    try:
        assert ops.wino_gemm_slim(True) is True
        A = make_layer(ops, 1, 8, 256, 512, 40, (0, 0, 40, 40), (0, 0))
        Bl = make_layer(ops, 2, 8, 64, 512, 40, (0, 0, 40, 40), (0, 0))
        stage(ops, A, 1)
        stage(ops, Bl, 1)
        stage(ops, Bl, 2)
        torch.cuda.synchronize()

        def clear():
            A.ws[A.n_v:].fill_(SENTINEL)
            Bl.out.fill_(SENTINEL)
            torch.cuda.synchronize()

        clear()
        stage(ops, A, 2)
        torch.cuda.synchronize()
        stage(ops, Bl, 4)
        torch.cuda.synchronize()
        m_seq, y_seq = A.ws[A.n_v:].cpu().numpy().view(np.int32), Bl.out.cpu().numpy().view(np.int32)
        assert int((y_seq == np.float32(SENTINEL).view(np.int32)).sum()) == 0

        clear()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        stage(ops, A, 2, s1)
        stage(ops, Bl, 4, s2)
        s1.synchronize()
        s2.synchronize()
        m_par, y_par = A.ws[A.n_v:].cpu().numpy().view(np.int32), Bl.out.cpu().numpy().view(np.int32)
    finally:
        ops.wino_gemm_slim(before)
    assert np.array_equal(m_seq, m_par)
    assert np.array_equal(y_seq, y_par)
