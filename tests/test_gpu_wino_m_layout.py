"""GPU: the products M of the separate-GEMM layers in channel quads (include/iiseg.h, iiseg_conv_wino_m_quad:
M[slice][Mpad / 4][Tpad][4], 16-byte stores in the GEMM epilogues, 16-byte loads in the output kernels)
against the layout it replaces, M[slice][Mpad][Tpad].

Every case runs its layer under both settings of `ops.wino_m_quad` and requires
  * `torch.equal` of the whole output tensor -- larger planes pre-filled with a sentinel, the layer's window
    placed inside, so that a store outside the window shows -- and, where the pool is fused, of the pooled map
    and the mask bytes;
  * for the fp32 Winograd form, that the new workspace holds exactly the old products, permuted: every row up to
    Mpad and every column up to Tpad, so that the documented layout is what the producers write;
  * on integer data -- inputs in [-3, 3], weights multiples of 4 in [-8, 8], so that U = G g G^T is integral
    and every partial sum an exact fp32 integer -- equality with torch.nn.functional.conv2d in float64 on the
    CPU.  The float64 result is asserted to stay below 2^24 before anything is launched
    (`test_integer_references_fit_fp32` does so without a GPU).

Shapes (fp32, Cin = 272 > WINO_FUSED_MAX_CIN and no multiple of 32: the separate GEMM): T = 50 tiles (below one
128-tile block, no multiple of 4) with Cout = 130 (Mpad 256, the last quad half used) and 128; T = 300 (a
second pixel block; 128 x 128 tiles by the launcher's last-round rule); T = 600 with Cout = 512 (16 * 5 * 2 =
160 workgroups of 256 x 128 fill one round where 320 of 128 x 128 take two: the 256 x 128 tile)."""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest
import torch
import torch.nn.functional as F

SENTINEL = -7777.25
MASK_SENTINEL = 0xEE
CIN = 272

Case = namedtuple('Case', 'name B cin hw cout k pad mma relu bias anchor window add pool unpool form')


def case(name, B, hw, cout, cin=CIN, k=3, pad=1, mma='f32', relu=True, bias=True, anchor=(0, 0), window=None,
         add=False, pool=False, unpool=False, form='wino_f32'):
    return Case(name, B, cin, hw, cout, k, pad, mma, relu, bias, anchor, window, add, pool, unpool, form)


CASES = [
    case('t50-cout130', 2, 9, 130),
    case('t50-cout128-plain', 2, 9, 128, relu=False, bias=False),
    case('t300-two-blocks', 3, 20, 130),
    # tiles start at odd rows / columns: rows 1..14 and columns 3..18 for the window rows 2..13, columns 4..17
    case('t300-odd-anchor-cut-window', 3, 20, 130, anchor=(1, 1), window=(2, 4, 12, 14)),
    case('t300-skip-add', 3, 20, 130, add=True),
    case('t300-skip-add-odd-anchor-window', 3, 20, 130, anchor=(1, 1), window=(2, 4, 12, 14), add=True, relu=False),
    case('t600-cout512-256x128', 6, 20, 512),
    case('pool-mask-even-map', 3, 20, 130, pool=True),
    case('pool-mask-odd-map', 2, 9, 130, pool=True),             # the last row / column has no pooled value
    case('depool-from-mask-bytes', 3, 20, 130, unpool=True),
    case('depool-odd-map-odd-anchor', 2, 13, 128, unpool=True, anchor=(1, 1), window=(1, 2, 10, 11)),
    case('bf16-gemm-fp32-output', 1, 8, 256, cin=1024, mma='bf16', form='wino_bf16'),
    case('bf16-gemm-cut-window-add', 2, 9, 258, cin=1024, mma='bf16', form='wino_bf16', anchor=(1, 0),
         window=(2, 1, 6, 7), add=True),
    case('splitk-1x1-cout11', 2, 7, 11, cin=1024, k=1, pad=0, form='gemm_f32'),
    case('splitk-7x7-valid', 2, 9, 130, cin=48, k=7, pad=0, form='gemm_f32'),
    case('splitk-1x1-bf16', 2, 7, 11, cin=1024, k=1, pad=0, mma='bf16', form='gemm_bf16'),
]
IDS = [c.name for c in CASES]


def out_hw(c):
    return c.hw + 2 * c.pad - (c.k - 1)


def make_data(c, integer):
    """CPU float64 operands of a case: w, b, x (the logical input), and up / mask bytes / add where used."""
    rng = np.random.default_rng(sum((i + 1) * ord(ch) for i, ch in enumerate(c.name)) + (1 if integer else 0))
    K = c.cin * c.k * c.k
    if integer:
        w = 4.0 * rng.integers(-2, 3, size=(c.cout, c.cin, c.k, c.k))
        b = rng.integers(-4, 5, size=c.cout).astype(np.float64)
        draw = lambda shape: rng.integers(-3, 4, size=shape).astype(np.float64)
    else:
        f32 = lambda a: a.astype(np.float32).astype(np.float64)
        w = f32(rng.standard_normal((c.cout, c.cin, c.k, c.k)) / np.sqrt(K))
        b = f32(rng.standard_normal(c.cout))
        draw = lambda shape: f32(rng.standard_normal(shape))
    t = {'w': w, 'b': b if c.bias else None}
    if c.unpool:
        h2 = c.hw // 2
        up = draw((c.B, c.cin, h2, h2))
        mask = rng.integers(0, 16, size=(c.B, c.cin, h2, h2)).astype(np.uint8)
        x = np.zeros((c.B, c.cin, c.hw, c.hw))
        for a in range(2):
            for bb in range(2):
                bit = (mask >> (a * 2 + bb)) & 1
                x[:, :, a:2 * h2:2, bb:2 * h2:2] = up * bit
        t.update(up=up, mask=mask, x=x)
    else:
        t['x'] = draw((c.B, c.cin, c.hw, c.hw))
    if c.add:
        oh = out_hw(c)
        wh, ww = (c.window or (0, 0, oh, oh))[2:]
        t['add'] = draw((c.B, c.cout, wh + 3, ww + 4))
    return t


ADD_OFF = (2, 3)
PLACE = (2, 3)


def reference(c, t):
    """float64 on the CPU: (the window of the output, pooled map or None, mask bytes or None)."""
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    full = F.conv2d(tt(t['x']), tt(t['w']), None if t['b'] is None else tt(t['b']), padding=c.pad)
    oh = out_hw(c)
    y0, x0, wh, ww = c.window or (0, 0, oh, oh)
    ref = full[:, :, y0:y0 + wh, x0:x0 + ww]
    if c.add:
        ref = ref + tt(t['add'])[:, :, ADD_OFF[0]:ADD_OFF[0] + wh, ADD_OFF[1]:ADD_OFF[1] + ww]
    if c.relu:
        ref = torch.clamp(ref, min=0)
    pooled = mask = None
    if c.pool:
        assert c.window is None
        h2 = oh // 2
        blocks = ref[:, :, :2 * h2, :2 * h2].reshape(c.B, c.cout, h2, 2, h2, 2)
        pooled = blocks.amax(dim=(3, 5))
        eq = (blocks == pooled[:, :, :, None, :, None]).to(torch.uint8)
        mask = eq[:, :, :, 0, :, 0] | (eq[:, :, :, 0, :, 1] << 1) | (eq[:, :, :, 1, :, 0] << 2) | \
            (eq[:, :, :, 1, :, 1] << 3)
    return ref, pooled, mask


_REFS = {}


def integer_reference(c):
    """The integer operands of a case and their float64 result, computed once."""
    if c.name not in _REFS:
        t = make_data(c, integer=True)
        ref = reference(c, t)
        full = reference(c._replace(relu=False), t)[0]
        _REFS[c.name] = (t, ref, float(full.abs().max()))
    return _REFS[c.name]


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_integer_references_fit_fp32(c):
    """No GPU: the float64 result of every exactness case stays below 2^24, and so does the bound on any partial
    sum of the transformed operands (|V| <= 4 * 3, |U| <= 9 * 8 / 4, an output sums 9 products M)."""
    t, ref, peak = integer_reference(c)
    assert peak < 2 ** 24
    assert np.all(t['w'] % 4 == 0) and np.abs(t['w']).max() <= 8 and np.abs(t['x']).max() <= 3
    if c.k == 3:
        assert 9 * c.cin * 12 * 18 < 2 ** 24
    else:
        assert c.cin * c.k * c.k * 3 * 8 < 2 ** 24


@pytest.fixture(scope='module')
def ops(built_lib):
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from iterative_inference_segm_amd import ops as _ops
    return _ops


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def make_call(ops, c, t, monkeypatch):
    """The layer of a case and a function that launches it into fresh, sentinel-filled targets and returns
    (out -- the whole placed tensor --, pooled map or None, mask bytes or None)."""
    if c.mma == 'bf16':
        monkeypatch.setattr(ops, 'BF16_FORCE', 'wino')
    conv = ops.Conv(t['w'], t['b'], pad=c.pad, relu=c.relu, mma=c.mma)
    oh = out_hw(c)
    wh, ww = (c.window or (0, 0, oh, oh))[2:]
    kw = {}
    dense = c.form in ('gemm_f32', 'gemm_bf16')            # the split-K GEMM form takes dense outputs only
    if not dense:
        kw.update(anchor=c.anchor, place=PLACE)
    if c.window:
        kw['window'] = c.window
    if c.add:
        kw.update(add=dev(t['add']), add_off=ADD_OFF)
    if c.unpool:
        assert conv.mask_ok()
        x1 = dev(t['up'])
        kw.update(mask_in=dev(t['mask'], np.uint8), unpool_hw=(c.hw, c.hw))
    else:
        x1 = dev(t['x'])
    if c.pool:
        assert conv.pool_window(c.hw, c.hw, anchor=c.anchor) == (0, 0, oh, oh)
    oshape = (c.B, c.cout, wh, ww) if dense else (c.B, c.cout, wh + 5, ww + 6)

    def targets():
        k2 = dict(kw, out=torch.full(oshape, SENTINEL, device='cuda'))
        if c.pool:
            k2['pool_out'] = torch.full((c.B, c.cout, oh // 2, oh // 2), SENTINEL, device='cuda')
            k2['mask_out'] = torch.full((c.B, c.cout, oh // 2, oh // 2), MASK_SENTINEL, dtype=torch.uint8,
                                        device='cuda')
        return k2

    launch = conv._describe_call(x1, **targets())
    assert conv._form(launch) == c.form
    if c.form == 'wino_f32':
        assert c.cin > ops.WINO_FUSED_MAX_CIN or c.add                # the separate GEMM, not the fused kernel

    def call():
        k2 = targets()
        conv(x1, **k2)
        torch.cuda.synchronize()
        return k2['out'], k2.get('pool_out'), k2.get('mask_out')
    return conv, launch, call


def split_k(conv, d):
    """S of the fp32 split-K GEMM, from iiseg_conv_gemm_workspace_elems = Tpad * (Kpad + S * Mpad)."""
    T = d.B * d.OH * d.OW
    Tpad = (T + 127) // 128 * 128
    per_pixel, rem = divmod(conv.lib.iiseg_conv_gemm_workspace_elems(C.byref(d)), Tpad)
    S, rem2 = divmod(per_pixel - d.Kpad, d.Mpad)
    assert rem == 0 and rem2 == 0
    return S


def products(ops, conv, c, d, dev_of):
    """The products of the fp32 Winograd form as the last launch left them in the workspace: (16, Mpad * Tpad),
    with Mpad and Tpad."""
    r0, c0 = d.oy0 - ((d.oy0 - d.tile_y0) & 1), d.ox0 - ((d.ox0 - d.tile_x0) & 1)
    T = d.B * ((d.oy0 + d.OH - r0 + 1) // 2) * ((d.ox0 + d.OW - c0 + 1) // 2)
    Tpad = (T + 127) // 128 * 128
    n = int(conv.lib.iiseg_conv_wino_workspace_elems(C.byref(d)))
    per, rem = divmod(n, 16 * Tpad)
    Mpad = per - c.cin
    assert rem == 0 and Mpad >= c.cout and Mpad % 64 == 0
    ws = ops.workspace_refs(dev_of)[0]
    return ws[16 * c.cin * Tpad:n].clone().view(16, Mpad * Tpad), Mpad, Tpad


def run_both(ops, c, t, monkeypatch, check_products):
    conv, launch, call = make_call(ops, c, t, monkeypatch)
    before = ops.wino_m_quad()
    got, prods = [], []
    try:
        for on in (False, True):
            assert ops.wino_m_quad(on) is on
            got.append(call())
            if check_products:
                prods.append(products(ops, conv, c, launch.d, launch.x1.device))
    finally:
        ops.wino_m_quad(before)
    for old, new in zip(*got):
        assert (old is None) == (new is None)
        if old is not None:
            assert torch.equal(old, new)
    if check_products:
        (m_old, Mpad, Tpad), (m_new, _, _) = prods
        want = m_old.view(16, Mpad // 4, 4, Tpad).permute(0, 1, 3, 2).reshape(16, Mpad * Tpad)
        assert torch.equal(want.view(torch.int32), m_new.view(torch.int32)), 'M is not the old M in channel quads'
        assert not torch.equal(m_old, m_new)
    return conv, launch, got[1]


@pytest.mark.gpu
@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_quad_layout_gives_the_same_bits(ops, monkeypatch, c):
    t = make_data(c, integer=False)
    conv, launch, (out, pooled, mask) = run_both(ops, c, t, monkeypatch, c.form == 'wino_f32')
    if c.form == 'gemm_f32':
        S = split_k(conv, launch.d)
        print('%s: S = %d' % (c.name, S))
        if c.name == 'splitk-7x7-valid':
            assert S > 1                                   # the slice stride is exercised
    # Against the float64 result: the comparison above cannot tell two equally wrong layouts apart on a form
    # whose products are not inspected.  Outputs have unit variance (K terms x * w, w ~ 1 / sqrt(K)), so a
    # misplaced product is an error of order 1.  fp32: the bound of a K-term fp32 chain with Winograd's
    # constant, 4 * 2^-18 * sqrt(K).  bf16 operands: each rounded by at most 2^-9 of its size, a product by
    # 2^-8; the worst case over the sum of the products' sizes, K * E|x| * E|w| = 0.64 * sqrt(K), times 2.25
    # for the output transform's 9 / 4 terms of a 3x3 layer.
    ref = reference(c, t)[0]
    oh = out_hw(c)
    wh, ww = (c.window or (0, 0, oh, oh))[2:]
    win = out if c.form in ('gemm_f32', 'gemm_bf16') else out[:, :, PLACE[0]:PLACE[0] + wh, PLACE[1]:PLACE[1] + ww]
    err = float((win.double().cpu() - ref).abs().max())
    K = c.cin * c.k * c.k
    tol = 2.0 ** -8 * 0.64 * (2.25 if c.k == 3 else 1.0) * np.sqrt(K) if c.mma == 'bf16' else 4 * 2.0 ** -18 * np.sqrt(K)
    print('%s: max |err| vs float64 %.3e (bound %.3e)' % (c.name, err, tol))
    assert err <= tol


@pytest.mark.gpu
@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_quad_layout_is_exact_on_integer_data(ops, monkeypatch, c):
    t, (ref, ref_pooled, ref_mask), peak = integer_reference(c)
    assert peak < 2 ** 24                                  # before any launch
    conv, launch, (out, pooled, mask) = run_both(ops, c, t, monkeypatch, False)
    oh = out_hw(c)
    wh, ww = (c.window or (0, 0, oh, oh))[2:]
    whole = out.cpu()
    if c.form in ('gemm_f32', 'gemm_bf16'):
        win = whole
    else:
        sl = (slice(None), slice(None), slice(PLACE[0], PLACE[0] + wh), slice(PLACE[1], PLACE[1] + ww))
        win = whole[sl].clone()
        whole[sl] = SENTINEL
        assert bool((whole == SENTINEL).all()), 'wrote outside the window'
    assert torch.equal(win.double(), ref)
    if c.pool:
        assert torch.equal(pooled.cpu().double(), ref_pooled)
        assert torch.equal(mask.cpu(), ref_mask)
