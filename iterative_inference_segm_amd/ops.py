"""Operator layer: torch tensors in, HIP kernels of libiiseg_hip.so out.

torch is plumbing here (device memory + the current HIP stream); every arithmetic op is a
call through the C ABI (include/iiseg.h).  All ops enqueue on torch's current stream and
never synchronise.  Two arithmetic modes: float32 (throughput path) and float64 (strict-parity
path: the reference's CPU numerics), selected by the tensors' dtype.
"""
import collections
import ctypes as C
import os

import torch

from . import _lib
from ._lib import ConvDesc, DeconvDesc, CONV_RELU, CONV_UNPOOL, CONV_TRANSPOSED2, CONV_X3, CONV_ZINS, check
from .params import MODES_16BIT

# When set to a list, every conv launch appends (kernel, executed_flops, start_event, end_event):
# HIP events recorded on the launch stream right around the kernel (bench.py's roofline leg).
CONV_PROFILE = None
# With CONV_PROFILE: when set to a list, every C8 launch also appends its geometry (one dict per launch,
# same order as the 'conv_c8_kernel' entries of CONV_PROFILE) -- scripts/c8_step_profile.py
CONV_PROFILE_INFO = None
# ... and for kernels that are bound by HBM traffic rather than the matrix pipe: algorithmic bytes (input planes
# read once + output planes written once) summed per kernel name while CONV_PROFILE is on
KERNEL_BYTES = {}

_SUFFIX = {torch.float32: 'f32', torch.float64: 'f64'}

# float32 3x3 layers with at least this many input / output channels (and Cin % 16 == 0) run in
# Winograd F(2x2,3x3) form (conv_wino.hip); IISEG_WINO_MIN_CIN=0 switches the path off.  Below
# these widths the HBM-bound transforms cost more than the saved MFMAs (scripts/bench_wino.py).
WINO_MIN_CIN = int(os.environ.get('IISEG_WINO_MIN_CIN', '128'))
# float64 (strict-parity) path: Winograd F(2x2,3x3) on v_mfma_f64_16x16x4_f64 from this many input /
# output channels (conv_wino_f64.hip); IISEG_WINO_F64=0 keeps every layer on the direct kernel
WINO_F64 = os.environ.get('IISEG_WINO_F64', '1') != '0'
WINO_F64_MIN_CIN = int(os.environ.get('IISEG_WINO_F64_MIN_CIN', '128'))
# (a 128 -> 64 layer at 113^2 is HBM-bound on the V / M round trips: 1.35 ms against 1.1 ms on the halo kernel)
WINO_F64_MIN_COUT = int(os.environ.get('IISEG_WINO_F64_MIN_COUT', '128'))
WINO_MIN_COUT = int(os.environ.get('IISEG_WINO_MIN_COUT', '128'))
# Layers with at most this many input channels use the kernel that also applies the output
# transform (products stay in registers, no M round trip through HBM); deeper layers are
# MFMA-bound and run faster on the plain 256x128 GEMM + separate output transform.  0: never.
WINO_FUSED_MAX_CIN = int(os.environ.get('IISEG_WINO_FUSED_MAX_CIN', '256'))
# fuse the 2x2 max-pool behind a halo-kernel conv into that conv's epilogue
POOL_FUSE = os.environ.get('IISEG_POOL_FUSE', '1') != '0'
# ... and behind an fp32 Winograd layer (even tile anchor) into its output transform, with the DePool2D
# mask bytes on both sides of such layers (IISEG_WINO_POOL_FUSE=0: pre / pooled maps, the pool kernel)
WINO_POOL_FUSE = os.environ.get('IISEG_WINO_POOL_FUSE', '1') != '0'
# float64 path: the same in the halo-tile float64 kernel's epilogue (conv_halo_f64.hip)
F64_POOL_FUSE = os.environ.get('IISEG_F64_POOL_FUSE', '1') != '0'
# ... and DePool2D masks as bytes between its encoder / decoder layers (the float64 pre-pool map is never stored)
F64_MASKS = os.environ.get('IISEG_F64_MASKS', '1') != '0'
# BN_ReLU_Conv of FC-DenseNet's dense blocks as one kernel.  Off by default: measured 6 % SLOWER
# end to end on config 3 (361 vs 383 images/s) -- the per-element parameter loads in the conv's
# staging cost more than the separate HBM-bound normalisation pass saves.
BNRELU_FUSE = os.environ.get('IISEG_BNRELU_FUSE', '0') != '0'
# 'valid' KxK layers without a static-tap variant (7x7 fc6) as im2col + split-K GEMM
CONV_GEMM = os.environ.get('IISEG_CONV_GEMM', '1') != '0'
# Matrix-pipe operand precision of the float32 path's wide 3x3 layers: 'f32' (exact fp32 MFMA, the
# default: the path with tolerance claims) or 'bf16' (bf16 operands, fp32 accumulation -- statistical
# parity only; BASELINE north_star's 16-bit MFMA target).  Per-Conv `mma=` overrides the default.
DEFAULT_MMA = os.environ.get('IISEG_MMA', 'f32')
# bf16 mode: 3x3 layers at least this wide (input AND output channels) are candidates for the bf16
# Winograd kernels (conv_wino_bf16.hip); below, the direct bf16 kernel won every measured case
#  and also fuses the pool and the DePool2D byte masks
BF16_WINO_MIN_CIN = int(os.environ.get('IISEG_BF16_WINO_MIN_CIN', '256'))
# Both 16-bit forms possible for a layer (Winograd / direct): the choice is DETERMINISTIC -- an optional
# table of measured winners per launch geometry (bf16_picks.json beside this file, keys without the
# batch size; NONE is shipped: the static rule decides everywhere) and, for a geometry the table does
# not hold, a static rule on the geometry alone (`_bf16_static_pick`).  Two processes, two ranks, two runs make the same choices,
# so bf16 outputs are reproducible and identical across the ranks of a data-parallel evaluation, and a
# loop-invariant border and its recomputed window come from the same form.  IISEG_BF16_TUNE=1 (the
# generating script only) times both forms for keys the table lacks and records them in BF16_PICKS.
BF16_TUNE = os.environ.get('IISEG_BF16_TUNE', '0') == '1'
# 'wino' / 'halo': force one form wherever both apply (tests, A/B timing); '' = table, then rule
BF16_FORCE = os.environ.get('IISEG_BF16_FORM', '')
BF16_PICKS_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'bf16_picks.json')


def _bf16_key(Cin, Cout, C1, C2, unpool, OH, OW):
    return '%d,%d,%d,%d,%d,%d,%d' % (Cin, Cout, C1, C2, 1 if unpool else 0, OH, OW)


def _load_bf16_picks():
    import json
    try:
        with open(BF16_PICKS_FILE) as f:
            return {k: v for k, v in json.load(f).get('picks', {}).items() if v in ('wino', 'halo')}
    except OSError:
        return {}


BF16_PICKS = _load_bf16_picks()
BF16_TIMES = {}      # key -> [ms Winograd, ms direct] of the keys timed in this process (tuning runs)


def _bf16_static_pick(Cin, OW):
    """Rule for geometries outside the table, from the round-2 measurements: the
    direct kernel's 32-pixel column tiles waste (1 - OW / (32 ceil(OW / 32))) of its MFMAs, and from
    1024 input channels the long-K Winograd GEMM wins on any window."""
    fill = OW / (32.0 * ((OW + 31) // 32))
    return 'wino' if (Cin >= 1024 or fill < 0.7) else 'halo'


# C8 layers with at most 16 output channels on the 16-row MFMA kernel (conv_c8_m16.hip); 0: the
# 32-row form of conv_c8_bf16.hip (timing experiments)
C8_M16 = os.environ.get('IISEG_C8_M16', '1') != '0'
BF16_UPCONV1 = os.environ.get('IISEG_BF16_UPCONV1', '0') != '0'
BF16_WINO_MIN_COUT = int(os.environ.get('IISEG_BF16_WINO_MIN_COUT', '256'))
# Scratch is reused by consecutive launches of ONE stream (stream-ordered).  Engines that run
# concurrently on different streams (bench.py --streams 2) must not share it: every
# IterativeInference tags its launches (`workspace_tag`), and the cache is keyed (kind, device, tag).
# Kinds, in `workspace_refs` order: fp32 / float64 Winograd + GEMM scratch, BN partial sums, split-K slabs (C8 m16)
_SCRATCH_KINDS = {'f32': torch.float32, 'f64': torch.float64, 'bn': torch.float64, 'm16': torch.uint8}
_scratch = {}
_ws_tag = [0]


# The fp32 halo kernel's column tiles across the image seam are switched in the library, not here:
# IISEG_HALO_SEAM=0 in the environment, or `halo_seam(False)`, selects one tile grid per image.
def halo_seam(on=None):
    """The fp32 halo kernel's tiling for the launches that follow: True = 32-column tiles across the seam
    between consecutive images (the default, IISEG_HALO_SEAM), False = one tile grid per image; None only
    asks.  Returns the setting in force.  Both tilings give the same bits (A/B timing, tests)."""
    return bool(_lib.load().iiseg_conv_halo_seam(-1 if on is None else int(bool(on))))


def halo_seam_launches():
    """Launches of the fp32 halo kernel so far that ran the seam tiling."""
    return int(_lib.load().iiseg_conv_halo_seam_launches())


# The fp32 Winograd input transform's streaming kernel is switched in the library too:
# IISEG_WINO_INPUT_WIDE=0 in the environment, or `wino_input_wide(False)`, keeps the one-dword-store kernels.
def wino_input_wide(on=None, force=False):
    """The fp32 Winograd input transform for the launches that follow: True = the streaming kernel with
    16-byte stores wherever it applies (the default, IISEG_WINO_INPUT_WIDE), False = the per-tile and
    LDS-staged kernels; None only asks.  `force` (with True): also for the two classes that measured no gain
    and keep the older kernels otherwise (include/iiseg.h: under 4096 tiles; plain maps that fill the
    LDS-staged kernel's workgroups).  Returns the setting in force.  Same bits (A/B timing, tests)."""
    return bool(_lib.load().iiseg_conv_wino_input_wide(-1 if on is None else (2 if on and force else int(bool(on)))))


# And its form with two tiles per thread: IISEG_WINO_INPUT_NARROW=0, or `wino_input_narrow(False)`, keeps four.
def wino_input_narrow(on=None):
    """The streaming input transform for the launches that follow: True = two tiles per thread (24 KB of LDS,
    8-byte stores) where its staging fits (the default, IISEG_WINO_INPUT_NARROW), False = four; None only asks.
    Returns the setting in force.  Same bits (A/B timing, tests)."""
    return bool(_lib.load().iiseg_conv_wino_input_narrow(-1 if on is None else int(bool(on))))


# So is the layout of the GEMM products M in the workspace: IISEG_WINO_M_QUAD=0, or `wino_m_quad(False)`.
def wino_m_quad(on=None):
    """The products M of the separate-GEMM layers (fp32 / bf16 Winograd GEMM, split-K GEMM) for the launches
    that follow: True = channel quads, 16-byte stores and loads (the default, IISEG_WINO_M_QUAD), False =
    M[slice][Mpad][Tpad] in 4-byte pieces; None only asks.  Returns the setting in force.  Same bits (A/B
    timing, tests).  Process-wide: not to be changed between the separately launched stages of one layer."""
    return bool(_lib.load().iiseg_conv_wino_m_quad(-1 if on is None else int(bool(on))))


# And the register diet of the fp32 GEMM tiles: IISEG_WINO_GEMM_SLIM=0, or `wino_gemm_slim(False)`.
def wino_gemm_slim(on=None):
    """The 256x128 / 128x128 fp32 GEMM tiles (Winograd GEMM stage, split-K GEMM) for the launches that follow:
    True = addressing in scalar registers, 88 vector registers allocated (the default, IISEG_WINO_GEMM_SLIM),
    False = 120; None only asks.  Returns the setting in force.  Same bits (A/B timing, tests)."""
    return bool(_lib.load().iiseg_conv_wino_gemm_slim(-1 if on is None else int(bool(on))))


class workspace_tag:
    """Context manager: launches inside use the scratch buffers of `tag` (an engine's id)."""

    def __init__(self, tag):
        self.tag, self.prev = tag, None

    def __enter__(self):
        self.prev, _ws_tag[0] = _ws_tag[0], self.tag
        return self

    def __exit__(self, *exc):
        _ws_tag[0] = self.prev
        return False


def current_workspace_tag():
    return _ws_tag[0]


def _workspace(kind, n, device):
    """At least `n` elements of scratch of `kind` under the current workspace tag.  One grow rule: the
    old tensor is dropped before the larger one is allocated."""
    key = (kind, device, _ws_tag[0])
    ws = _scratch.get(key)
    if ws is None or ws.numel() < n:
        _scratch[key] = None
        ws = _scratch[key] = torch.empty(int(n), dtype=_SCRATCH_KINDS[kind], device=device)
    return ws


def drop_workspaces(tag):
    """Forget the scratch buffers of `tag` (an engine that goes away)."""
    for key in [k for k in _scratch if k[2] == tag]:
        _scratch.pop(key, None)


def workspace_refs(device):
    """The scratch tensors launches under the current workspace tag point into (fp32 / float64
    Winograd workspaces, BN partial sums, split-K slabs): a captured HIP graph keeps them alive."""
    return tuple(_scratch.get((kind, device, _ws_tag[0])) for kind in _SCRATCH_KINDS)


def workspace_ptrs(device):
    """Their device addresses (None where not allocated): part of what a captured graph is valid for."""
    return tuple(None if t is None else t.data_ptr() for t in workspace_refs(device))


# Dispatch timing (bench.py's roofline pass, `profile_begin` / `profile_end`): the two "events" around a
# conv call are positions in the library's launch sequence, and the time between them is the sum of the
# execution times of the kernels launched in between -- each measured by the start / stop HIP events its
# own dispatch carries (include/iiseg.h iiseg_profile_begin).  Off: torch events recorded on the stream.
_DISPATCH_TIMING = [False]
PROFILE_MS = []


class _LaunchMark:
    def __init__(self, n):
        self.n = n

    def elapsed_time(self, other):
        return float(sum(PROFILE_MS[self.n:other.n]))


_PROFILE_CAP = [16384]


def profile_begin(capacity=16384):
    check(_lib.load().iiseg_profile_begin(int(capacity)), 'iiseg_profile_begin')
    _DISPATCH_TIMING[0] = True
    _PROFILE_CAP[0] = int(capacity)
    del PROFILE_MS[:]


def profile_end():
    """Ends the pass and fills PROFILE_MS (one entry per launch of the library, in launch order).  A pass
    that filled the event table raises: launches past the capacity carry no events, and a roofline built
    on such a pass would silently under-report kernel time."""
    _DISPATCH_TIMING[0] = False
    cap = _PROFILE_CAP[0]
    buf = (C.c_float * cap)()
    n = _lib.load().iiseg_profile_end(buf, cap)
    if n < 0:
        raise RuntimeError('iiseg_profile_end: %d' % n)
    if n >= cap:
        raise RuntimeError('profiling pass reached its capacity of %d launches: later launches were not '
                           'timed (raise profile_begin(capacity))' % cap)
    PROFILE_MS[:] = list(buf[:n])
    return n


def _ev():
    """A mark on the launch stream right now (bench.py's roofline leg): a HIP event recorded on it, or,
    under dispatch timing, the position in the library's launch sequence."""
    if _DISPATCH_TIMING[0]:
        return _LaunchMark(_lib.load().iiseg_profile_count())
    ev = torch.cuda.Event(enable_timing=True)
    ev.record()
    return ev


def _stream():
    if not torch.cuda.is_available():
        raise RuntimeError('iiseg ops need device tensors on a HIP GPU; none is available and '
                           'there is no CPU fallback')
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t, dtype=torch.float32):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError('iiseg ops need device tensors (got %s)' % t.device)
    if t.dtype != dtype:
        raise RuntimeError('expected %s, got %s' % (dtype, t.dtype))
    if not t.is_contiguous():
        raise RuntimeError('iiseg ops need C-contiguous NCHW tensors')
    return C.c_void_p(t.data_ptr())


def _fn(name, dtype):
    """C entry point `iiseg_<name>_<f32|f64>` for a tensor dtype."""
    if dtype not in _SUFFIX:
        raise RuntimeError('iiseg ops support float32 and float64, not %s' % dtype)
    return getattr(_lib.load(), 'iiseg_%s_%s' % (name, _SUFFIX[dtype]))


def _launch(kernel, flops, fn, *args):
    """One call `fn(stream, *args)` of the library.  With CONV_PROFILE (read here, at call time) the call --
    and nothing else: operands, packing and scratch are the caller's business before it -- sits between two
    marks on the launch stream and is recorded as (kernel, flops, start, end).  `kernel` may be a function
    that names the kernel: it is evaluated only when profiling."""
    prof = CONV_PROFILE
    if prof is None:
        check(fn(_stream(), *args), fn.__name__)
        return
    ev0 = _ev()
    check(fn(_stream(), *args), fn.__name__)
    ev1 = _ev()
    prof.append((kernel() if callable(kernel) else kernel, flops, ev0, ev1))


def _launch_staged(fn, args, whole, stages):
    """The entry points whose last argument is a bit set of the kernels to run: one call with `whole`, or,
    under CONV_PROFILE, one call per (kernel, bits, flops) of `stages`, each recorded between its own marks."""
    prof = CONV_PROFILE
    if prof is None:
        check(fn(_stream(), *args, whole), fn.__name__)
        return
    ev0 = _ev()
    for kernel, bits, flops in stages:
        check(fn(_stream(), *args, bits), fn.__name__)
        ev1 = _ev()
        prof.append((kernel, flops, ev0, ev1))
        ev0 = ev1


def _count(n, what):
    """The result of a query of the library that returns a count, or a negative status (raised here)."""
    if n < 0:
        check(int(n), what)
    return int(n)


def _add_bytes(kernel, nbytes):
    """Algorithmic bytes of one launch, summed per kernel name (KERNEL_BYTES; callers do it under CONV_PROFILE)."""
    KERNEL_BYTES[kernel] = KERNEL_BYTES.get(kernel, 0.0) + nbytes


# the descriptor and operands of one launch of a Conv, as its `_run_<form>` methods take them; a bf16 C8 launch
# (`_describe_c8`) also has the scalars its kernels take and the 16-channel kernel's bn / stats / fold vectors
_Launch = collections.namedtuple(
    '_Launch', 'd x1 x2 pre pooled add out pool_out mask_in mask_out x1_ctot add_kind kind bn stats fold',
    defaults=(0, 0, 0, None, None, None))


class Conv:
    """One convolution layer bound to its weights: packed-weight (+ gather-table) cache per
    input geometry.  Weight layouts: 'oihw' (Lasagne Conv2DLayer W[out,in,kh,kw], P1) or
    'iohw' (DilatedConv2DLayer W[in,out,kh,kw], P11).  A call on NCHW tensors is three steps:
    `_describe_call` (host only), `_choose` (the kernel FORM, by name; host only), `_run_<form>`.  On bf16 C8
    tensors: `_choose_c8` (first: each of the two kernels has checks of its own), `_describe_c8`, `_run_<form>`."""

    # every form `_choose` can name; each has a `_run_<form>`
    FORMS = ('wino_bf16', 'halo_bf16', 'wino_f32', 'mask_f64', 'mask_f32', 'pool_f64', 'pool_f32',
             'gemm_bf16', 'gemm_f32', 'gemm_f64', 'wino_f64', 'direct', 'kxk_bf16')
    # ... and the two `_choose_c8` can name
    C8_FORMS = ('c8', 'c8_m16')
    # ... those with the 2x2 max-pool in their epilogue, and those that read / write DePool2D mask bytes
    POOL_FORMS = ('halo_bf16', 'wino_f32', 'mask_f64', 'mask_f32', 'pool_f64', 'pool_f32')
    MASK_FORMS = ('halo_bf16', 'wino_f32', 'mask_f64', 'mask_f32')

    def __init__(self, W, b, pad, relu, dil=1, layout='oihw', device='cuda', dtype=torch.float32,
                 transposed=False, mma=None, fwd16=False):
        """transposed=True: 3x3 stride-2 transposed convolution, crop='valid' (Deconv2DLayer
        W[in,out,3,3] -> layout 'iohw'); output (2H+1, 2W+1).  mma: 'f32' | 'bf16' operand
        precision on the matrix pipe (float32 tensors only; None: ops.DEFAULT_MMA).
        fwd16=True (a trainable module's fwd='bf16'; float32 with mma='f32' only): every
        launch of a plain 3x3 layer takes the 'halo_bf16' form and every launch of an undilated 'valid' K x K
        'oihw' layer (1 <= K <= 7, not 3) 'kxk_bf16' (conv_fwd_kxk on the parameter itself), whatever
        BF16_PICKS or the environment say -- a launch neither kernel takes is an error, never another form -- and
        `refresh()` packs the 3x3 layer's bf16 image again into the buffer it has.  A two-source launch of such a
        layer may have any C1 (iiseg_conv_halo_bf16_fwd: the k-tile that straddles x1 and x2)."""
        self.lib = _lib.load()
        self.mma = (mma or DEFAULT_MMA) if dtype == torch.float32 else 'f32'
        if self.mma not in ('f32', 'bf16', 'bf16c8', 'bf16x3'):
            raise ValueError("mma must be 'f32', 'bf16', 'bf16c8' or 'bf16x3'")
        # 'bf16c8': bf16 MFMA operands AND bf16 C8 activations between the 3x3 layers (conv_c8_bf16.hip);
        # a layer takes that form when it is handed a C8 tensor, any other call is the 'bf16' mode.
        # 'bf16x3': the fp32-class mode of the same kernel -- activations and weights as bf16 hi / lo
        # pairs, three products per term (IISEG_CONV_X3); any other call is the 'f32' mode
        self.x3 = self.mma == 'bf16x3'
        self.c8 = self.mma in ('bf16c8', 'bf16x3')
        if self.c8:
            self.mma = 'f32' if self.x3 else 'bf16'
        self.transposed = bool(transposed)
        self.dtype = dtype
        # (the conv kernels do not promise to propagate a NaN -- build.py EXTRA_FLAGS -- so non-finite
        # parameters are refused where they enter, once, when the layer is built)
        if not bool(torch.isfinite(torch.as_tensor(W)).all()) or \
                (b is not None and not bool(torch.isfinite(torch.as_tensor(b)).all())):
            raise ValueError('non-finite convolution parameters (NaN / Inf in W or b)')
        self.W = torch.as_tensor(W).to(dtype).contiguous().to(device)
        self.b = None if b is None else torch.as_tensor(b).to(dtype).contiguous().to(device)
        self.layout = layout
        if layout == 'oihw':
            self.Cout, self.Cin, self.KH, self.KW = self.W.shape
            self.so, self.sc = self.Cin * self.KH * self.KW, self.KH * self.KW
        elif layout == 'iohw':
            self.Cin, self.Cout, self.KH, self.KW = self.W.shape
            self.so, self.sc = self.KH * self.KW, self.Cout * self.KH * self.KW
        else:
            raise ValueError(layout)
        self.pad, self.dil, self.relu = int(pad), int(dil), bool(relu)
        # a plain 3x3 layer: what every Winograd / halo / C8 form requires
        self.plain3x3 = (self.KH, self.KW) == (3, 3) and self.dil == 1 and not self.transposed
        taps = (self.KH, self.KW) in ((1, 1), (3, 3)) or \
            ((self.KH, self.KW) == (4, 4) and dtype == torch.float32)
        # which kernel family the C ABI dispatches this filter shape to
        if dtype == torch.float64:
            self.kernel = 'conv_taps_f64_kernel'
            # other filter shapes (7x7 fc6): im2col + the same weights as a 1x1 convolution
            self.via_im2col = not taps
            if self.via_im2col and (layout != 'oihw' or self.pad != 0 or self.dil != 1):
                raise NotImplementedError('float64 path: only valid, undilated oihw KxK filters '
                                          'go through im2col')
        else:
            self.kernel = 'conv_taps_f32_kernel' if taps else 'conv_igemm_f32_kernel'
            # direct 3x3 layers below 256 output channels run on the halo-tile kernel (the C side
            # dispatches: conv_igemm.hip, IISEG_CONV_HALO)
            # (dilated 3x3 layers with at most 16 output channels -- the context module -- too)
            if (self.KH, self.KW) == (3, 3) and not self.transposed and \
                    os.environ.get('IISEG_CONV_HALO', '1') != '0' and \
                    ((self.dil == 1 and self.Cout < 256) or
                     (self.dil in (2, 4, 8, 16) and self.Cout <= 16)):
                self.kernel = 'conv_halo_f32_kernel'
            self.via_im2col = False
        self.wino = (dtype == torch.float32 and self.plain3x3 and self.Cin % 16 == 0 and
                     0 < WINO_MIN_CIN <= self.Cin and self.Cout >= WINO_MIN_COUT)
        self.wino_f64 = (dtype == torch.float64 and WINO_F64 and self.plain3x3 and self.Cin % 16 == 0 and
                         self.Cin >= WINO_F64_MIN_CIN and self.Cout >= WINO_F64_MIN_COUT)
        self.wino_bf16 = (self.mma == 'bf16' and self.plain3x3 and self.Cin >= BF16_WINO_MIN_CIN and
                          self.Cout >= BF16_WINO_MIN_COUT)
        # bf16 mode: every other plain 3x3 layer on the bf16 halo kernel (conv_halo_bf16.hip)
        self.halo_bf16 = self.mma == 'bf16' and self.plain3x3 and not self.wino_bf16
        self.c8 = self.c8 and self.plain3x3
        self.fwd16 = bool(fwd16)
        if self.fwd16:
            kxk = (self.KH == self.KW and 1 <= self.KH <= 7 and self.dil == 1 and self.pad == 0 and
                   not self.transposed and layout == 'oihw')
            if dtype != torch.float32 or self.mma != 'f32' or self.c8 or not (self.plain3x3 or kxk):
                raise NotImplementedError("Conv(fwd16=True): a float32 mma='f32' layer, plain 3x3 or 'valid' K x K "
                                          "'oihw' with 1 <= K <= 7 (dtype %s, mma %r, filter %dx%d, pad %d, dil %d)"
                                          % (dtype, self.mma, self.KH, self.KW, self.pad, self.dil))
        self._W16_desc = None       # fwd16: the descriptor `_W16` was packed for (`refresh`)
        self._U = None
        self._U16 = None
        self._W16 = None
        self._W16c8 = None
        self._form_cache = {}
        self._descs = {}
        self._packs = {}
        self._pack_descs = {}       # the descriptor each entry of `_packs` was packed for (`refresh`)

    def out_hw(self, H, W):
        if self.transposed:
            return (H - 1) * 2 + self.KH, (W - 1) * 2 + self.KW
        return (H + 2 * self.pad - self.dil * (self.KH - 1),
                W + 2 * self.pad - self.dil * (self.KW - 1))

    def flops(self, B, OH, OW):
        """Nominal 2*Cin*Cout*k*k*OH*OW*B (SURVEY 6.2 convention)."""
        return 2.0 * self.Cin * self.Cout * self.KH * self.KW * OH * OW * B

    def _fill(self, B, C1, C2, H, W, window, add_geom, flags, out_slice=None, place=None, pad=None):
        """A ConvDesc of this layer filled in, no library call: an NCHW launch's before `_describe` plans it, a
        bf16 C8 launch's as it stands (never planned).  window = (oy0, ox0, OH, OW); or None: add_geom = (AH,
        AW, ay0, ax0), out_slice = (out_ctot, out_c0), place = (out_H, out_W, out_y0, out_x0)."""
        d = ConvDesc()
        d.B, d.C1, d.C2, d.H, d.W = B, C1, C2, H, W
        d.Cout, d.KH, d.KW, d.dil, d.pad = self.Cout, self.KH, self.KW, self.dil, self.pad if pad is None else pad
        d.oy0, d.ox0, d.OH, d.OW = window
        if add_geom is not None:
            d.AH, d.AW, d.ay0, d.ax0 = add_geom
        d.flags = flags
        if out_slice is not None:
            d.out_ctot, d.out_c0 = out_slice
        if place is not None:
            d.out_H, d.out_W, d.out_y0, d.out_x0 = place
        return d

    def _describe(self, B, C1, C2, H, W, window, add_geom, unpool, out_slice=None, place=None,
                  anchor=(0, 0)):
        """The planned ConvDesc of a launch (iiseg_conv_plan / _f64 fill Kpad, Mpad and refuse bad
        geometry): no device, no stream.  Cached per argument tuple."""
        key = (B, C1, C2, H, W, window, add_geom, unpool, out_slice, place, anchor)
        d = self._descs.get(key)
        if d is not None:
            return d
        if C1 + C2 != self.Cin:
            raise RuntimeError('conv expects %d input channels, got %d+%d' % (self.Cin, C1, C2))
        fullH, fullW = self.out_hw(H, W)
        d = self._fill(B, C1, C2, H, W, window if window is not None else (0, 0, fullH, fullW), add_geom,
                       (CONV_RELU if self.relu else 0) | (CONV_UNPOOL if unpool else 0) |
                       (CONV_TRANSPOSED2 if self.transposed else 0), out_slice, place)
        d.tile_y0, d.tile_x0 = int(anchor[0]) & 1, int(anchor[1]) & 1
        if self.via_im2col:
            # logical layer: 1x1 over C*KH*KW channels of the im2col'd tensor (OH x OW)
            d.C1, d.C2, d.H, d.W = C1 * self.KH * self.KW, 0, fullH, fullW
            d.KH = d.KW = 1
        if self.dtype == torch.float64:
            check(self.lib.iiseg_conv_plan_f64(C.byref(d)), 'iiseg_conv_plan_f64')
        else:
            check(self.lib.iiseg_conv_plan(C.byref(d)), 'iiseg_conv_plan')
        self._descs[key] = d
        return d

    def _packed(self, d):
        """(wp, ktab): the direct kernels' packed weights (+ gather table), made on first use.  They depend
        on the input geometry only: one copy per (C1, C2, H, W), shared by every window / placement."""
        pkey = (d.C1, d.C2, d.H, d.W)
        packed = self._packs.get(pkey)
        if packed is None:
            so, sc = (self.Cin * self.KH * self.KW, 1) if self.via_im2col else (self.so, self.sc)
            wp = torch.empty(d.Kpad * d.Mpad, dtype=self.dtype, device=self.W.device)
            if self.dtype == torch.float64:
                check(self.lib.iiseg_conv_pack_f64(_stream(), C.byref(d), _ptr(self.W, self.dtype),
                                                   so, sc, _ptr(wp, self.dtype)), 'iiseg_conv_pack_f64')
                packed = (wp, None)
            else:
                ktab = torch.empty(d.Kpad * 4, dtype=torch.int32, device=self.W.device)
                check(self.lib.iiseg_conv_pack_f32(_stream(), C.byref(d), _ptr(self.W), so, sc,
                                                   _ptr(wp), _ptr(ktab, torch.int32)), 'iiseg_conv_pack_f32')
                packed = (wp, ktab)
            self._packs[pkey] = packed
            self._pack_descs[pkey] = d
        return packed

    def refresh(self):
        """After `self.W` / `self.b` have been changed IN PLACE (an optimizer step): packs every entry of
        `_packs` again into the buffers it already has -- launches that hold their addresses (a captured graph)
        see the new weights.  Layers that already hold a Winograd / 16-bit transform of their weights are
        refused: those live in tensors a captured graph would keep pointing at -- except a fwd16 layer's bf16
        halo image, which is packed again in place here.  No host wait."""
        if any(t is not None for t in (self._U, self._U16, None if self.fwd16 else self._W16, self._W16c8)):
            raise NotImplementedError('Conv.refresh: this layer holds transformed weights (Winograd / bf16 forms); '
                                      'only the direct kernels\' packs are refreshed in place')
        so, sc = (self.Cin * self.KH * self.KW, 1) if self.via_im2col else (self.so, self.sc)
        for pkey, (wp, ktab) in self._packs.items():
            d = self._pack_descs[pkey]
            if self.dtype == torch.float64:
                check(self.lib.iiseg_conv_pack_f64(_stream(), C.byref(d), _ptr(self.W, self.dtype),
                                                   so, sc, _ptr(wp, self.dtype)), 'iiseg_conv_pack_f64')
            else:
                check(self.lib.iiseg_conv_pack_f32(_stream(), C.byref(d), _ptr(self.W), so, sc,
                                                   _ptr(wp), _ptr(ktab, torch.int32)), 'iiseg_conv_pack_f32')
        if self.fwd16 and self._W16 is not None:
            self._pack_halo_bf16(self._W16_desc, profiled=True)

    def _plan(self, B, C1, C2, H, W, window, add_geom, unpool, out_slice=None, place=None,
              anchor=(0, 0)):
        """(d, wp, ktab): descriptor + the direct kernels' packed weights (`_describe`, `_packed`)."""
        d = self._describe(B, C1, C2, H, W, window, add_geom, unpool, out_slice, place, anchor)
        return (d,) + self._packed(d)


    def _choose(self, d, unpool=False, masked=False, pool=False, add=False, x2=False, mask_in=False,
                tune=None):
        """The FORM (one of Conv.FORMS) that runs the launch `d` describes, given the few facts of the call
        that matter: DePool2D input, mask bytes on either side (`masked`), a fused pool, a skip-add, a second
        source, mask bytes as input.  The order below IS the precedence.  Only the library's host-side
        `*_supported` queries are asked: no stream, no allocation, no launch.  `tune(key)`: BF16_TUNE's
        timing of both 16-bit forms, handed in by the caller."""
        lib, dp, f64 = self.lib, C.byref(d), self.dtype == torch.float64
        if masked and not self.mask_ok(False):
            raise RuntimeError('DePool2D byte masks need a halo-kernel or fp32 Winograd layer '
                               '(Conv.mask_ok)')
        if self.fwd16:
            # one kernel and one rounding statement per layer class; nothing else may run the launch
            # (its own check: a two-source launch may have any C1 -- the straddling k-tile)
            if self.plain3x3 and lib.iiseg_conv_halo_bf16_fwd_check(dp) == 0:
                return 'halo_bf16'
            if not self.plain3x3 and not (masked or pool or add or x2 or unpool) and \
                    (d.oy0, d.ox0, d.OH, d.OW) == (0, 0) + self.out_hw(d.H, d.W) and not d.out_ctot and not d.out_H:
                return 'kxk_bf16'
            raise RuntimeError('Conv(fwd16=True): neither conv_halo_bf16_kernel nor conv_fwd_kxk_bf16_kernel takes '
                               'this launch (%dx%d filter, window / placement / extras)' % (self.KH, self.KW))
        plain = not masked and not pool
        if plain and self.wino_bf16 and lib.iiseg_conv_wino_bf16_supported(dp):
            if lib.iiseg_conv_halo_bf16_supported(dp):
                # both 16-bit forms can run this layer: table of measured winners, else the static rule
                # (see BF16_PICKS above).  The key carries no batch size: an image gets the same form
                # alone and in a batch.
                key = _bf16_key(self.Cin, self.Cout, d.C1, d.C2, unpool, d.OH, d.OW)
                pick = BF16_FORCE or BF16_PICKS.get(key)
                if not pick and tune is not None:
                    pick = tune(key)
                if (pick or _bf16_static_pick(self.Cin, d.OW)) == 'halo':
                    return 'halo_bf16'
            return 'wino_bf16'
        # (the DAE's last layer -- DePool2D input, <= 16 output channels: reading pre / pooled it is
        # read-bound and faster on the 16-row fp32 kernel, 0.60 vs 0.74 ms at configs[1]; from mask
        # bytes the bf16 kernel wins, 0.45 vs 0.58 ms)
        if self.halo_bf16 and not (unpool and self.Cout <= 16 and not mask_in and not BF16_UPCONV1) and \
                lib.iiseg_conv_halo_bf16_supported(dp):
            return 'halo_bf16'
        # (fp32 operands: the pool and the mask bytes ride in the Winograd kernels too, iiseg_conv_wino_mask_f32)
        if self.wino and (self.mma == 'f32' or plain) and lib.iiseg_conv_wino_supported(dp) and \
                self._form_by_full_map(lib.iiseg_conv_wino_supported, d):
            return 'wino_f32'
        if masked:
            return 'mask_f64' if f64 else 'mask_f32'
        if pool:
            return 'pool_f64' if f64 else 'pool_f32'
        if CONV_GEMM and not x2 and not unpool and not add:
            # 'valid' KxK layers without a static-tap variant (7x7 fc6), and deep 1x1 layers on few pixels
            # (fc7, score_fr), where the same split-K GEMM beats the 1x1 tap kernel
            if not f64 and (self.kernel == 'conv_igemm_f32_kernel' or
                            ((self.KH, self.KW) == (1, 1) and self.Cin >= 1024)):
                if self.mma == 'bf16' and lib.iiseg_conv_gemm_bf16_supported(dp):
                    return 'gemm_bf16'
                if lib.iiseg_conv_gemm_supported(dp):
                    return 'gemm_f32'
            # float64 (fc6 after im2col, fc7, score_fr): split-K GEMM on the Winograd path's kernel
            if f64 and (d.KH, d.KW) == (1, 1) and d.C1 >= 1024 and lib.iiseg_conv_gemm_f64_supported(dp):
                return 'gemm_f64'
        if self.wino_f64 and not self.via_im2col and lib.iiseg_conv_wino_f64_supported(dp) and \
                self._form_by_full_map(lib.iiseg_conv_wino_f64_supported, d):
            return 'wino_f64'
        return 'direct'

    def _form_by_full_map(self, supported, d):
        """A layer's kernel FORM (Winograd or direct) is decided on its FULL-MAP geometry, not on the
        window a launch covers: a form with a size limit (workspace within 32-bit offsets) that takes a
        small window but not the full map would otherwise compute the loop-invariant border with one
        kernel and the recomputed window with another -- and the two differ in their last bits, which the
        exact work eliminations rule out.  Cached per input geometry."""
        key = (id(supported), d.B, d.C1, d.C2, d.H, d.W, d.flags)
        ok = self._form_cache.get(key)
        if ok is None:
            full = ConvDesc()
            C.memmove(C.byref(full), C.byref(d), C.sizeof(ConvDesc))
            fh, fw = self.out_hw(d.H, d.W)
            full.oy0, full.ox0, full.OH, full.OW = 0, 0, fh, fw
            full.out_H = full.out_W = full.out_y0 = full.out_x0 = 0
            if full.AH:
                full.AH, full.AW, full.ay0, full.ax0 = max(full.AH, fh), max(full.AW, fw), 0, 0
            ok = self._form_cache[key] = bool(supported(C.byref(full)))
        return ok

    def _direct_kernel(self, d, add):
        """The 'direct' form's profile label: which kernel the C side's own dispatch (iiseg_conv_f32 /
        _f64) takes for `d`.  Evaluated only under profiling."""
        kern = self.kernel
        if self.dtype == torch.float64:
            if self.lib.iiseg_conv_halo_f64_supported(C.byref(d)):
                kern = 'conv_halo_f64_kernel'
        elif (add is None or self.b is None) and self.lib.iiseg_conv_small_supported(C.byref(d)):
            kern = 'conv_small_f32_kernel'         # vector ALU, HBM-bound: algorithmic bytes for the roofline
            _add_bytes(kern, 4.0 * d.B * (self.Cin * d.H * d.W +
                                          (2 if add is not None else 1) * self.Cout * d.OH * d.OW))
        if kern == 'conv_halo_f32_kernel' and d.C2 > 0 and d.C1 % 4:
            kern = 'conv_taps_f32_kernel'      # a k-tile would straddle the two sources
        return kern

    def _check_pool(self, form, d, add=False):
        """The form-specific refusals of a fused pool (host only)."""
        lib, dp = self.lib, C.byref(d)
        if form == 'wino_f32' and not lib.iiseg_conv_wino_pool_supported(dp):
            raise RuntimeError('conv + pool fusion is not available for this launch '
                               '(Winograd: even tile anchor and whole pooling windows)')
        if (form == 'pool_f64' and (add or not lib.iiseg_conv_pool_f64_supported(dp))) or \
                (form == 'pool_f32' and not lib.iiseg_conv_pool_supported(dp)):
            raise RuntimeError('conv + pool fusion is not available for this launch')


    def _extras_form(self):
        """Where `_choose` sends a pooled / masked launch of this layer as far as the layer's own flags
        decide it (its order of precedence without the per-launch queries): 'halo_bf16', 'wino_f32', or the
        direct kernels' pool / mask entry points ('f64' / 'f32')."""
        if self.halo_bf16:
            return 'halo_bf16'
        if self.wino and self.mma == 'f32':
            return 'wino_f32'
        return 'f64' if self.dtype == torch.float64 else 'f32'

    def _f64_halo_runs(self):
        """float64: does the LIBRARY run this layer on the halo-tile kernel (the only float64 kernel with the
        fused pool and the mask bytes)?  Asked once per layer on a representative request -- the switch
        IISEG_F64_HALO, the packed-weight shape (Kpad % 36, Mpad % 64) -- so that `pool_fusable` / `mask_ok`
        never promise what iiseg_conv_pool_f64 / iiseg_conv_mask_f64 would refuse."""
        ok = self._form_cache.get('f64_halo')
        if ok is None:
            d = ConvDesc()
            d.B, d.C1, d.C2, d.H, d.W = 1, self.Cin, 0, 16, 16
            d.Cout, d.KH, d.KW, d.pad, d.dil = self.Cout, self.KH, self.KW, self.pad, self.dil
            d.OH, d.OW = self.out_hw(16, 16)
            d.flags = CONV_RELU if self.relu else 0
            ok = self.lib.iiseg_conv_plan_f64(C.byref(d)) == 0 and \
                bool(self.lib.iiseg_conv_halo_f64_supported(C.byref(d)))
            self._form_cache['f64_halo'] = ok
        return ok

    def pool_fusable(self, c8=None, anchor=None):
        """True if this layer runs on a kernel whose epilogue can do the 2x2 max-pool.  `c8`:
        whether the call will hand it a C8 tensor (None: the form the layer was built for) -- a
        layer built with mma='bf16c8' and called on fp32 NCHW input runs the 'bf16' forms, and
        those decide.  `anchor`: the Winograd tile anchor of the call -- an fp32 Winograd layer
        pools in its output transform only at an even anchor (a 2x2 tile is then one pooling
        window); without an anchor such a layer answers False."""
        if not POOL_FUSE or self.dtype not in _SUFFIX:
            return False
        if self.c8 and c8 is not False:
            return True
        form = self._extras_form()
        if form == 'halo_bf16':
            return True
        if form == 'wino_f32':
            return anchor is not None and WINO_POOL_FUSE and not (int(anchor[0]) & 1 or int(anchor[1]) & 1)
        if form == 'f64':
            # float64: the halo-tile kernel's epilogue (conv_halo_f64.hip), layers it runs with > 16 output channels
            return F64_POOL_FUSE and self.plain3x3 and not self.wino_f64 and self.Cout > 16 and \
                self._f64_halo_runs()
        # iiseg_conv_pool_f32: the fp32 halo kernel's epilogue (a bf16 layer that gets here is a Winograd one)
        return self.mma == 'f32' and self.kernel == 'conv_halo_f32_kernel' and 16 < self.Cout < 256

    def mask_ok(self, c8=None):
        """True if this layer can take / produce DePool2D masks as bytes (halo kernels and the fp32
        Winograd form, only where the byte form runs the very kernel the pre / pooled form runs).
        `c8` as in `pool_fusable`.  (A Winograd layer produces them with its fused pool at an even
        tile anchor; at an odd one its caller pools with `maxpool2x2(..., mask=)`.)"""
        if self.c8 and c8 is not False:
            return True
        if not self.plain3x3 or self.dtype not in _SUFFIX:
            return False
        form = self._extras_form()
        if form == 'wino_f32':
            return WINO_POOL_FUSE
        if form == 'f64':
            # float64: layers of the halo-tile kernel (the mask bytes hold float64 comparisons)
            return F64_MASKS and not self.wino_f64 and self._f64_halo_runs()
        # iiseg_conv_halo_bf16 / iiseg_conv_mask_f32 (a bf16 layer on the latter is a Winograd one: no bytes)
        return self.kernel == 'conv_halo_f32_kernel' and (form == 'halo_bf16' or self.mma == 'f32')

    def pool_window(self, H, W, region=None, c8=None, anchor=None):
        """If the 2x2 max-pool that follows this layer can be fused into its epilogue: the conv
        window (y0, x0, h, w) to launch so that every pooling window touching `region` (of the
        conv output; None = the whole map) is whole -- even origin, even extent unless it ends at
        the map's last row / column.  None if the layer has no such epilogue (`pool_fusable`,
        `anchor` as there)."""
        if not self.pool_fusable(c8, anchor):
            return None
        fh, fw = self.out_hw(H, W)
        if region is None:
            return (0, 0, fh, fw)
        y0, x0 = region[0] & ~1, region[1] & ~1
        y1, x1 = min((region[0] + region[2] + 1) & ~1, fh), min((region[1] + region[3] + 1) & ~1, fw)
        if region[0] + region[2] == fh:
            y1 = fh
        if region[1] + region[3] == fw:
            x1 = fw
        return (y0, x0, y1 - y0, x1 - x0)


    def __call__(self, x1, x2=None, pre=None, pooled=None, add=None, add_off=(0, 0),
                 window=None, out=None, out_c0=None, place=None, anchor=(0, 0), pool_out=None,
                 mask_in=None, unpool_hw=None, mask_out=None, store_out=True, out_format=None,
                 in_c=None, bn=None, stats=None, fold=None, zins=False):
        """x1 (B,C1,H,W) [+ x2 (B,C2,H,W): channel concat, x1 first].  With `pre`/`pooled`
        the logical input is the equality-mask unpool of x1 (DePool2D) at pre's size.
        `add` (B,Cout,AH,AW) is summed into the result starting at `add_off`;
        `window` = (oy0, ox0, OH, OW) restricts the computed output region.  With `out_c0`
        the result is written into channels [out_c0, out_c0+Cout) of the wider tensor `out`; with
        `place` = (y0, x0) the (OH, OW) result is written at that offset of the larger planes of
        `out` (everything else in `out` is left untouched).  `anchor` = parity of the output
        row / column where the Winograd 2x2 tiles start (a per-layer constant for the caller:
        launches of one layer agree bit for bit only under the same anchor).  `pool_out`: the FULL
        pooled tensor (B, Cout, fullH//2, fullW//2) of this layer; the 2x2 max-pool of the computed
        window is written into it by the conv's epilogue (see `pool_window`).

        DePool2D masks as bytes (`mask_ok()` layers, include/iiseg.h iiseg_conv_mask_f32):
        `mask_out` (uint8, pool_out's shape) receives, with the pool, one byte per pooled element
        whose bit (y&1)*2+(x&1) says pre == pooled; `store_out=False` then skips the pre-pool map
        itself (returns None; `out`, if given, only carries the placement geometry).  `mask_in`
        (uint8, x1's shape) + `unpool_hw` = (H, W) replace `pre` / `pooled` for the unpooled
        input."""
        if is_c8(x1):
            form = self._choose_c8(x2, add, pool_out, store_out, out_format, zins, in_c, bn, stats, fold)
            launch = self._describe_c8(form, x1, x2, add, add_off, window, out, out_c0, place, pool_out, mask_in,
                                       unpool_hw, mask_out, store_out, out_format, in_c, bn, stats, fold, zins)
            getattr(self, '_run_' + form)(launch)
            return launch.out
        if zins or in_c is not None or bn is not None or stats is not None or fold is not None:
            raise RuntimeError('in_c / bn / stats: C8 input only (layers with at most 16 output channels)')
        launch = self._describe_call(x1, x2, pre, pooled, add, add_off, window, out, out_c0, place, anchor,
                                     pool_out, mask_in, unpool_hw, mask_out, store_out)
        tune = None
        if BF16_TUNE and self.wino_bf16 and not torch.cuda.is_current_stream_capturing():
            tune = lambda key: self._tune_bf16(key, launch)
        getattr(self, '_run_' + self._form(launch, tune))(launch)
        return launch.out

    def _describe_call(self, x1, x2=None, pre=None, pooled=None, add=None, add_off=(0, 0), window=None,
                       out=None, out_c0=None, place=None, anchor=(0, 0), pool_out=None, mask_in=None,
                       unpool_hw=None, mask_out=None, store_out=True):
        """Step 1: `__call__`'s arguments checked, the launch described, `out` settled (shapes / dtypes only)."""
        dt = self.dtype
        unpool = pre is not None or mask_in is not None
        masked = mask_in is not None or mask_out is not None
        B, C1 = x1.shape[0], x1.shape[1]
        if masked:
            if mask_in is not None and (pre is not None or mask_in.dtype != torch.uint8 or
                                        mask_in.shape != x1.shape or unpool_hw is None or
                                        (unpool_hw[0] // 2, unpool_hw[1] // 2) != tuple(x1.shape[2:])):
                raise RuntimeError('mask_in: uint8 of x1\'s shape %s with unpool_hw, without pre'
                                   % (tuple(x1.shape),))
            if mask_out is not None and (pool_out is None or mask_out.dtype != torch.uint8 or
                                         mask_out.shape != pool_out.shape):
                raise RuntimeError('mask_out: uint8 of pool_out\'s shape')
        if not store_out and (mask_out is None or out_c0 is not None):
            raise RuntimeError('store_out=False needs pool_out and mask_out')
        if mask_in is not None:
            H, W = int(unpool_hw[0]), int(unpool_hw[1])
        elif unpool:
            H, W = pre.shape[2], pre.shape[3]
            if pooled.shape != x1.shape or pre.shape[:2] != x1.shape[:2] or \
                    (H // 2, W // 2) != tuple(x1.shape[2:]):
                raise RuntimeError('unpool shapes: up %s pre %s pooled %s'
                                   % (tuple(x1.shape), tuple(pre.shape), tuple(pooled.shape)))
        else:
            H, W = x1.shape[2], x1.shape[3]
        C2 = 0
        if x2 is not None:
            if x2.shape[0] != B or tuple(x2.shape[2:]) != (H, W):
                raise RuntimeError('concat shapes %s vs %s' % (tuple(x1.shape), tuple(x2.shape)))
            C2 = x2.shape[1]
        add_geom = None
        if add is not None:
            add_geom = (add.shape[2], add.shape[3], add_off[0], add_off[1])
            if add.shape[0] != B or add.shape[1] != self.Cout:
                raise RuntimeError('add tensor shape %s' % (tuple(add.shape),))
        if self.via_im2col:
            if x2 is not None or unpool or window is not None:
                raise NotImplementedError('float64 im2col path: plain single-source conv only')
            d = self._describe(B, C1, 0, H, W, None, add_geom, False)
        else:
            out_slice = None if out_c0 is None else (out.shape[1], int(out_c0))
            pl = None if place is None else (out.shape[2], out.shape[3], int(place[0]), int(place[1]))
            d = self._describe(B, C1, C2, H, W, window, add_geom, unpool, out_slice, pl,
                               (int(anchor[0]) & 1, int(anchor[1]) & 1))
        if not store_out:
            out = None                     # geometry taken above; nothing is written
        elif place is not None:
            if self.via_im2col or out is None or out.shape[0] != B or out.dtype != dt or \
                    (out_c0 is None and out.shape[1] != self.Cout):
                raise RuntimeError('bad placement target %s' % (None if out is None else tuple(out.shape),))
        elif out_c0 is not None:
            if self.via_im2col or tuple(out.shape[2:]) != (d.OH, d.OW) or out.shape[0] != B or \
                    out.dtype != dt or out_c0 + self.Cout > out.shape[1]:
                raise RuntimeError('bad output slice %s @%d' % (tuple(out.shape), out_c0))
        elif out is None:
            out = torch.empty((B, self.Cout, d.OH, d.OW), dtype=dt, device=x1.device)
        elif tuple(out.shape) != (B, self.Cout, d.OH, d.OW) or out.dtype != dt:
            raise RuntimeError('out shape %s != %s' % (tuple(out.shape), (B, self.Cout, d.OH, d.OW)))
        if pool_out is not None:
            fh, fw = self.out_hw(H, W)
            if tuple(pool_out.shape) != (B, self.Cout, fh // 2, fw // 2) or pool_out.dtype != dt:
                raise RuntimeError('pool_out shape %s %s' % (tuple(pool_out.shape), pool_out.dtype))
        return _Launch(d, x1, x2, pre, pooled, add, out, pool_out, mask_in, mask_out)

    def _form(self, c, tune=None):
        """Step 2: the form of the described launch `c`; refuses a fused pool that form cannot do."""
        form = self._choose(c.d, unpool=c.pre is not None or c.mask_in is not None,
                            masked=c.mask_in is not None or c.mask_out is not None,
                            pool=c.pool_out is not None, add=c.add is not None, x2=c.x2 is not None,
                            mask_in=c.mask_in is not None, tune=tune)
        if c.pool_out is not None:
            self._check_pool(form, c.d, c.add is not None)
        return form

    def _tune_bf16(self, key, c):
        """BF16_TUNE: times both 16-bit forms of a launch (unprofiled), fills BF16_TIMES / BF16_PICKS."""
        global CONV_PROFILE
        prof, CONV_PROFILE = CONV_PROFILE, None
        try:
            ms = []
            for f in (self._run_wino_bf16, self._run_halo_bf16):
                f(c)                                          # packs the weights, warms up
                e0 = _ev(); f(c); f(c); f(c); e1 = _ev()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
        finally:
            CONV_PROFILE = prof
        BF16_TIMES[key] = ms
        pick = BF16_PICKS[key] = 'wino' if ms[0] <= ms[1] else 'halo'
        return pick


    def _source(self, c):
        """x1 as the kernels read it: float64 layers without a static-tap variant run on its im2col."""
        if not self.via_im2col:
            return c.x1
        B, C1, H, W = c.x1.shape
        cols = torch.empty((B, c.d.C1, c.d.H, c.d.W), dtype=self.dtype, device=c.x1.device)
        check(self.lib.iiseg_im2col_f64(_stream(), _ptr(c.x1, self.dtype), _ptr(cols, self.dtype), B, C1, H, W,
                                        self.KH, self.KW), 'iiseg_im2col_f64')
        return cols

    def _direct_args(self, c, x1, *between):
        """Operands the direct kernels' entry points share: sources, [`between`,] packed weights (+ the fp32
        gather table), bias, skip-add, output."""
        d, dt = c.d, self.dtype
        wp, ktab = self._packed(d)
        tab = () if ktab is None else (_ptr(ktab, torch.int32),)
        return (C.byref(d), _ptr(x1, dt), _ptr(c.x2, dt), _ptr(c.pre, dt), _ptr(c.pooled, dt), *between,
                _ptr(wp, dt), *tab, _ptr(self.b, dt), _ptr(c.add, dt), _ptr(c.out, dt))

    def _run_direct(self, c):
        """The C side's own dispatch among the direct kernels (iiseg_conv_f32 / iiseg_conv_f64)."""
        d = c.d
        _launch(lambda: self._direct_kernel(d, c.add), self.flops(d.B, d.OH, d.OW), _fn('conv', self.dtype),
                *self._direct_args(c, self._source(c)))

    def _halo_kernel(self):
        return 'conv_halo_f64_kernel' if self.dtype == torch.float64 else self.kernel

    def _run_mask_f32(self, c):
        """The direct kernel with DePool2D mask bytes in and / or pool + bytes out (iiseg_conv_mask_f32 / _f64)."""
        _launch(self._halo_kernel(), self.flops(c.d.B, c.d.OH, c.d.OW), _fn('conv_mask', self.dtype),
                *self._direct_args(c, c.x1, _ptr(c.mask_in, torch.uint8)), _ptr(c.pool_out, self.dtype),
                _ptr(c.mask_out, torch.uint8))

    def _run_pool_f32(self, c):
        """The direct kernel with the 2x2 max-pool in its epilogue (iiseg_conv_pool_f32 / _f64)."""
        _launch(self._halo_kernel(), self.flops(c.d.B, c.d.OH, c.d.OW), _fn('conv_pool', self.dtype),
                *self._direct_args(c, c.x1), _ptr(c.pool_out, self.dtype))

    _run_mask_f64, _run_pool_f64 = _run_mask_f32, _run_pool_f32

    def _run_gemm_bf16(self, c):
        """im2col + split-K GEMM on bf16 operands (iiseg_conv_gemm_bf16)."""
        lib, d = self.lib, c.d
        if self._W16 is None:
            self._W16 = torch.empty(lib.iiseg_conv_gemm_bf16_weight_bytes(C.byref(d)) // 2,
                                    dtype=torch.bfloat16, device=self.W.device)
            check(lib.iiseg_conv_gemm_bf16_pack(_stream(), C.byref(d), _ptr(self.W), self.so,
                                                self.sc, _ptr(self._W16, torch.bfloat16)),
                  'iiseg_conv_gemm_bf16_pack')
        ws = _workspace('f32', (lib.iiseg_conv_gemm_bf16_workspace_bytes(C.byref(d)) + 3) // 4, c.x1.device)
        _launch('wino_gemm_bf16_kernel', self.flops(d.B, d.OH, d.OW), lib.iiseg_conv_gemm_bf16,
                C.byref(d), _ptr(c.x1), _ptr(self._W16, torch.bfloat16), _ptr(self.b), _ptr(ws), _ptr(c.out))

    def _run_gemm_f32(self, c):
        """im2col + split-K GEMM + output pass (iiseg_conv_gemm_f32): three kernels."""
        d = c.d
        wp, _ = self._packed(d)
        ws = _workspace('f32', self.lib.iiseg_conv_gemm_workspace_elems(C.byref(d)), c.x1.device)
        _launch_staged(self.lib.iiseg_conv_gemm_f32,
                       (C.byref(d), _ptr(c.x1), _ptr(wp), _ptr(self.b), _ptr(ws), _ptr(c.out)), 7,
                       (('gemm_im2col_kernel', 1, 0.0),
                        ('wino_gemm_kernel', 2, self.flops(d.B, d.OH, d.OW)),
                        ('gemm_output_kernel', 4, 0.0)))

    def _run_gemm_f64(self, c):
        """Deep 1x1 layers in float64: split-K GEMM on the Winograd path's kernel (iiseg_conv_gemm_f64)."""
        d, dt = c.d, self.dtype
        wp, _ = self._packed(d)
        x1 = self._source(c)
        ws = _workspace('f64', self.lib.iiseg_conv_gemm_f64_workspace_elems(C.byref(d)), x1.device)
        _launch('wino64_gemm_kernel', self.flops(d.B, d.OH, d.OW), self.lib.iiseg_conv_gemm_f64,
                C.byref(d), _ptr(x1, dt), _ptr(wp, dt), _ptr(self.b, dt), _ptr(ws, dt), _ptr(c.out, dt))

    def _run_halo_bf16(self, c):
        """Direct 3x3 form on the bf16 matrix pipe (include/iiseg.h, iiseg_conv_halo_bf16)."""
        lib, d = self.lib, c.d
        # (a fwd16 layer goes through the _fwd entries: the same kernel, C1 of a two-source launch free)
        nbytes, run = (lib.iiseg_conv_halo_bf16_fwd_weight_bytes, lib.iiseg_conv_halo_bf16_fwd) if self.fwd16 else \
            (lib.iiseg_conv_halo_bf16_weight_bytes, lib.iiseg_conv_halo_bf16)
        if self._W16 is None:
            self._W16 = torch.empty(nbytes(C.byref(d)) // 2, dtype=torch.bfloat16, device=self.W.device)
            self._W16_desc = d
            self._pack_halo_bf16(d)
        _launch('conv_halo_bf16_kernel', self.flops(d.B, d.OH, d.OW), run,
                C.byref(d), _ptr(c.x1), _ptr(c.x2), _ptr(c.pre), _ptr(c.pooled),
                _ptr(self._W16, torch.bfloat16), _ptr(self.b), _ptr(c.add), _ptr(c.out), _ptr(c.pool_out),
                _ptr(c.mask_in, torch.uint8), _ptr(c.mask_out, torch.uint8))

    def _pack_halo_bf16(self, d, profiled=False):
        """The bf16 image of the 3x3 filter (it depends on the channel counts only) into `_W16`: one launch, no host
        wait.  profiled: recorded under CONV_PROFILE (the per-step re-pack of `refresh`; first use never is)."""
        args = (C.byref(d), _ptr(self.W), C.c_int64(self.so), C.c_int64(self.sc), _ptr(self._W16, torch.bfloat16))
        pack = self.lib.iiseg_conv_halo_bf16_fwd_pack if self.fwd16 else self.lib.iiseg_conv_halo_bf16_pack
        if not profiled:
            check(pack(_stream(), *args), 'iiseg_conv_halo_bf16_pack')
            return
        kern = 'halo_pack_bf16_kernel'
        _launch(kern, 0.0, pack, *args)
        if CONV_PROFILE is not None:
            _add_bytes(kern, 4.0 * self.W.numel() + 2.0 * self._W16.numel())

    def _run_kxk_bf16(self, c):
        """fwd16: the 'valid' K x K layer on the parameter itself (conv_fwd_kxk, csrc/conv_kxk_bf16.hip)."""
        conv_fwd_kxk(c.x1, self.W, self.b, relu=self.relu, out=c.out)

    def _wino_gemm_flops(self, d, K):
        """Multiplies the 16 Winograd GEMMs of a launch actually issue: 16 * 2 * K * Cout * tiles."""
        r0, c0 = d.oy0 - ((d.oy0 - d.tile_y0) & 1), d.ox0 - ((d.ox0 - d.tile_x0) & 1)
        T = d.B * ((d.oy0 + d.OH - r0 + 1) // 2) * ((d.ox0 + d.OW - c0 + 1) // 2)
        return 16 * 2.0 * K * self.Cout * T

    def _run_wino_bf16(self, c):
        """bf16-operand Winograd form (include/iiseg.h, iiseg_conv_wino_bf16): input transform ->
        V16, then one kernel for the 16 GEMMs + output transform + epilogue."""
        lib, d = self.lib, c.d
        if self._U16 is None:
            self._U16 = torch.empty(lib.iiseg_conv_wino_bf16_weight_bytes(C.byref(d)) // 2,
                                    dtype=torch.bfloat16, device=self.W.device)
            check(lib.iiseg_conv_wino_bf16_pack(_stream(), C.byref(d), _ptr(self.W), self.so,
                                                self.sc, _ptr(self._U16, torch.bfloat16)),
                  'iiseg_conv_wino_bf16_pack')
        ws = _workspace('f32', (lib.iiseg_conv_wino_bf16_workspace_bytes(C.byref(d)) + 3) // 4, c.x1.device)
        _launch_staged(lib.iiseg_conv_wino_bf16,
                       (C.byref(d), _ptr(c.x1), _ptr(c.x2), _ptr(c.pre), _ptr(c.pooled),
                        _ptr(self._U16, torch.bfloat16), _ptr(self.b), _ptr(c.add), _ptr(ws), _ptr(c.out)), 3,
                       (('wino_input_bf16_kernel', 1, 0.0),      # (the GEMM's K is padded to 64)
                        ('wino_fused_bf16_kernel', 2, self._wino_gemm_flops(d, (self.Cin + 63) // 64 * 64))))

    def _run_wino_f64(self, c):
        """float64 Winograd form (include/iiseg.h, iiseg_conv_wino_f64)."""
        lib, d, dt = self.lib, c.d, torch.float64
        if self._U is None:
            self._U = torch.empty(lib.iiseg_conv_wino_f64_weight_elems(C.byref(d)), dtype=dt,
                                  device=self.W.device)
            check(lib.iiseg_conv_wino_pack_f64(_stream(), C.byref(d), _ptr(self.W, dt), self.so, self.sc,
                                               _ptr(self._U, dt)), 'iiseg_conv_wino_pack_f64')
        ws = _workspace('f64', lib.iiseg_conv_wino_f64_workspace_elems(C.byref(d)), c.x1.device)
        _launch('wino64_gemm_kernel', self.flops(d.B, d.OH, d.OW), lib.iiseg_conv_wino_f64,
                C.byref(d), _ptr(c.x1, dt), _ptr(c.x2, dt), _ptr(c.pre, dt), _ptr(c.pooled, dt),
                _ptr(self._U, dt), _ptr(self.b, dt), _ptr(c.add, dt), _ptr(ws, dt), _ptr(c.out, dt))

    def _run_wino_f32(self, c):
        """Winograd F(2x2,3x3) form of the layer (include/iiseg.h, iiseg_conv_wino_f32; with a
        fused pool or mask bytes iiseg_conv_wino_mask_f32)."""
        lib, d = self.lib, c.d
        if self._U is None:
            self._U = torch.empty(lib.iiseg_conv_wino_weight_elems(C.byref(d)), dtype=torch.float32,
                                  device=self.W.device)
            check(lib.iiseg_conv_wino_pack_f32(_stream(), C.byref(d), _ptr(self.W), self.so, self.sc,
                                               _ptr(self._U)), 'iiseg_conv_wino_pack_f32')
        ws = _workspace('f32', lib.iiseg_conv_wino_workspace_elems(C.byref(d)), c.x1.device)
        if c.mask_in is None and c.pool_out is None:
            fn = lib.iiseg_conv_wino_f32
            args = (C.byref(d), _ptr(c.x1), _ptr(c.x2), _ptr(c.pre), _ptr(c.pooled), _ptr(self._U),
                    _ptr(self.b), _ptr(c.add), _ptr(ws), _ptr(c.out))
        else:
            fn = lib.iiseg_conv_wino_mask_f32
            args = (C.byref(d), _ptr(c.x1), _ptr(c.x2), _ptr(c.pre), _ptr(c.pooled),
                    _ptr(c.mask_in, torch.uint8), _ptr(self._U), _ptr(self.b), _ptr(c.add), _ptr(ws),
                    _ptr(c.out), _ptr(c.pool_out), _ptr(c.mask_out, torch.uint8))
        gemm_flops = self._wino_gemm_flops(d, self.Cin)
        # (a skip-add would be read by the fused kernel's epilogue, uncoalesced and with nothing to
        # hide its latency: such layers keep the separate, coalesced output transform)
        if self.Cin <= WINO_FUSED_MAX_CIN and self.Cin % 32 == 0 and c.add is None:
            _launch_staged(fn, args, 7 | 8, (('wino_input_kernel', 1 | 8, 0.0),
                                             ('wino_fused_kernel', 2 | 8, gemm_flops)))
        else:
            _launch_staged(fn, args, 7, (('wino_input_kernel', 1, 0.0), ('wino_gemm_kernel', 2, gemm_flops),
                                         ('wino_output_kernel', 4, 0.0)))

    def bnrelu_conv(self, stack, n, bn, out, out_c0):
        """BN_ReLU_Conv as one kernel (iiseg_conv_bnrelu_f32): the conv reads the first `n`
        channels of `stack` (B, cap, H, W) and normalises + rectifies them while staging
        (bn = (beta, gamma, mean, inv_std), batch statistics); the result goes to channels
        [out_c0, out_c0 + Cout) of `out`.  Returns None when the layer has no such kernel (the
        caller then runs bn_relu + the plain conv)."""
        if self.dtype != torch.float32 or not BNRELU_FUSE or not self.plain3x3 or self.Cout > 16:
            return None
        B, cap, H, W = stack.shape
        d, wp, ktab = self._plan(B, n, 0, H, W, None, None, False, (out.shape[1], int(out_c0)), None)
        if not self.lib.iiseg_conv_bnrelu_supported(C.byref(d)) or \
                tuple(out.shape[2:]) != (d.OH, d.OW) or out_c0 + self.Cout > out.shape[1]:
            return None
        beta, gamma, mean, inv_std = bn
        _launch(self.kernel, self.flops(B, d.OH, d.OW), self.lib.iiseg_conv_bnrelu_f32,
                C.byref(d), _ptr(stack), cap * H * W, _ptr(beta), _ptr(gamma), _ptr(mean), _ptr(inv_std),
                _ptr(wp), _ptr(ktab, torch.int32), _ptr(self.b), _ptr(out))
        return out


    def c8_tiling(self, d, pool):
        """(kind, th, tw, quad) of a C8 launch: include/iiseg.h iiseg_conv_c8_tiling."""
        t = (C.c_int32 * 4)()
        check(self.lib.iiseg_conv_c8_tiling(C.byref(d), 1 if pool else 0, t), 'iiseg_conv_c8_tiling')
        return tuple(t)

    def _c8_weights(self):
        """The layer's weights packed for the C8 kernels, once per layer, for the REAL channel count (the
        rows of padding channels are zero); shared by `_run_c8` and `_run_c8_m16`.  A captured graph may
        point at them: never replaced after first use."""
        if self._W16c8 is None:
            lib = self.lib
            dp = self._fill(1, self.Cin, 0, 8, 8, (0, 0, 8, 8), None, 0, pad=1)      # (any 'same' geometry)
            Wsrc, so, sc = self.W, self.so, self.sc
            if self.x3:
                # two k-groups of whole 16-channel k-tiles [W_hi | W_lo]; the split values are bf16
                # numbers, the pack's rounding leaves them as they are
                Cp = (self.Cin + 15) // 16 * 16
                Wsrc = torch.empty((self.Cout, 2 * Cp, 3, 3), dtype=torch.float32, device=self.W.device)
                check(lib.iiseg_conv_c8_split_weights(_stream(), _ptr(self.W), self.so, self.sc,
                                                      self.Cout, self.Cin, _ptr(Wsrc)),
                      'iiseg_conv_c8_split_weights')
                dp.C1, so, sc = 2 * Cp, 2 * Cp * 9, 9
            self._W16c8 = torch.empty(lib.iiseg_conv_halo_bf16_weight_bytes(C.byref(dp)) // 2,
                                      dtype=torch.bfloat16, device=self.W.device)
            check(lib.iiseg_conv_halo_bf16_pack(_stream(), C.byref(dp), _ptr(Wsrc), so, sc,
                                                _ptr(self._W16c8, torch.bfloat16)),
                  'iiseg_conv_halo_bf16_pack')
        return _ptr(self._W16c8, torch.bfloat16)

    @staticmethod
    def _c8_unpool_hw(x1, mask_in, unpool_hw, chunks, ok):
        """(H, W) of a DePool2D input on C8: `mask_in` uint8 (B, chunks, h, w, 8) over x1's (h, w) planes,
        `unpool_hw` the unpooled size; `ok`: what else the kernel at hand demands of such a launch."""
        if not ok or unpool_hw is None or not is_c8_mask(mask_in) or \
                tuple(mask_in.shape) != (x1.shape[0], chunks) + tuple(x1.shape[2:]) or \
                (unpool_hw[0] // 2, unpool_hw[1] // 2) != tuple(x1.shape[2:4]):
            raise RuntimeError('C8 DePool2D input: up %s, mask %s, unpool_hw %s'
                               % (tuple(x1.shape), tuple(mask_in.shape), unpool_hw))
        return int(unpool_hw[0]), int(unpool_hw[1])

    def _choose_c8(self, x2, add, pool_out, store_out, out_format, zins, in_c, bn, stats, fold):
        """Step 1 on C8 input: which of C8_FORMS the call gets, from its facts alone -- 'c8_m16' (layers with
        at most 16 output channels, csrc/conv_c8_m16.hip) or 'c8' (csrc/conv_c8_bf16.hip); refuses what only
        the former can do on a launch of the latter."""
        if not self.c8:
            raise RuntimeError("C8 input needs a 3x3 layer built with mma='bf16c8'")
        if C8_M16 and self.Cout <= 16 and not self.x3 and x2 is None and add is None and pool_out is None and \
                store_out and (out_format or 'c8') in ('c8', 'nchw') and not zins:
            return 'c8_m16'
        if stats is not None or fold is not None:
            raise RuntimeError('stats: layers with at most 16 output channels')
        if in_c is not None or bn is not None:
            raise RuntimeError('in_c / bn on C8 input: layers with at most 16 output channels')
        return 'c8'

    def _c8_target(self, x1, OH, OW, fmt, out, out_c0, placed, store, m16):
        """Where a C8 launch writes: `out` in the format `fmt` ('c8' | 'c8f32' | 'nchw'), allocated here if the
        call gave none and the map is stored; an (OH, OW) map unless `placed`; whole, or with `out_c0` the
        chunk planes [out_c0 / 8, ...) of a wider C8 tensor.  Returns (out, (out_ctot, out_c0) or None).  m16,
        the 16-channel kernel's own rules: out_c0 needs a tensor to point into, any C8 tensor but a contiguous
        two-chunk one (a wider one, a two-chunk channel slice) is the slice at 0, one message for all."""
        B, c8 = x1.shape[0], fmt == 'c8'
        chunks = c8_chunks(self.Cout) * (2 if self.x3 and c8 else 1)
        dtype = torch.bfloat16 if c8 else torch.float32
        if out is None and store:
            if m16 and out_c0 is not None:
                raise RuntimeError('out_c0 needs a target')
            out = torch.empty((B, self.Cout, OH, OW) if fmt == 'nchw' else (B, chunks, OH, OW, 8), dtype=dtype,
                              device=x1.device)
        elif out is None and out_c0 is None:
            return None, None               # (only the pool is kept)
        c0 = out_c0
        if m16 and c0 is None and c8 and is_c8(out) and (out.shape[1] != 2 or not out.is_contiguous()):
            c0 = 0
        if c0 is None:
            ok = out.dtype == dtype and ((out.dim() == 4 and out.shape[1] == self.Cout) if fmt == 'nchw' else
                                         (out.dim() == 5 and out.shape[1] == chunks))
        else:
            ok = c8 and not self.x3 and is_c8(out) and c0 % 16 == 0 and c0 + chunks * 8 <= out.shape[1] * 8 and \
                not (m16 and out.shape[1] % 2)
        if not ok or out.shape[0] != B or not (placed or tuple(out.shape[2:4]) == (OH, OW)):
            shape = None if out is None else tuple(out.shape)
            raise RuntimeError('bad output target %s for a 16-channel C8 layer' % (shape,) if m16 else
                               'bad C8 output target %s' % (shape,) if c0 is None else
                               'bad C8 output slice %s @%s' % (shape, out_c0))
        return out, None if c0 is None else (c8_ctot(out), int(c0))

    def _describe_c8(self, form, x1, x2, add, add_off, window, out, out_c0, place, pool_out, mask_in, unpool_hw,
                     mask_out, store_out, out_format, in_c, bn, stats, fold, zins):
        """Step 2 on C8 input: `__call__`'s arguments checked for the kernel `form`, the launch described, `out`
        settled (shapes, dtypes and strides only).  x1 / x2 / pool_out: C8 tensors (`is_c8`); add: C8 bf16 or
        C8 fp32 (float32, same 5-D shape); mask_in / mask_out: uint8 (B, C/8, h, w, 8).  out_format: 'c8'
        (default), 'c8f32', or 'nchw' (fp32 NCHW, the class-score layer: default when Cout is not a multiple
        of 8).  x1 and `out` may be channel slices of wider C8 tensors; every other operand is contiguous.
        'c8_m16' only -- in_c: convolve only the first in_c channels of x1 (a dense block's stack); bn = (a, b):
        BatchNorm + ReLU x <- max(a x + b, 0) applied to the input on the way in (`bn_fold`); stats = (mean,
        inv_std, eps): the batch statistics of the 16 produced channels (bf16 C8 output) into entries [out_c0,
        out_c0 + 16) of the two vectors, out of the conv's epilogue; fold = (beta, gamma, a, b, n) (with stats):
        the reduction that finishes them also forms the (a, b) pair of the NEXT consumer's BatchNorm over the
        first n channels."""
        m16, x3, unpool = form == 'c8_m16', self.x3, mask_in is not None
        pair = 2 if x3 else 1                     # chunk planes of a kind-1 tensor per channel chunk
        B, H, W = x1.shape[0], x1.shape[2], x1.shape[3]
        C2, add_kind, add_geom = 0, 0, None
        if m16:
            x1_ctot = c8_ctot(x1)        # (x1 may be a channel slice of a wider tensor: the parent's count)
            C1, ok = c8_first_channels(x1, in_c, self.Cin)
            if not ok:
                raise RuntimeError('conv of %d input channels on the first %d of %d C8 channels'
                                   % (self.Cin, C1, x1_ctot))
            if unpool:
                H, W = self._c8_unpool_hw(x1, mask_in, unpool_hw, x1.shape[1], C1 == x1_ctot and x1.is_contiguous())
        else:
            for name, t in (('x2', x2), ('add', add), ('pool_out', pool_out), ('mask_out', mask_out)):
                if t is not None and not t.is_contiguous():
                    raise RuntimeError('C8 launch: %s must be contiguous' % name)
            if x1.shape[1] % pair or (x3 and x2 is not None):
                raise RuntimeError('bf16x3 layer: hi / lo pair input, no channel concat')
            C1 = x1.shape[1] // pair * 8
            if unpool:
                H, W = self._c8_unpool_hw(x1, mask_in, unpool_hw, C1 // 8, x2 is None)
            elif zins:
                # the logical input is x1 zero-inserted (include/iiseg.h IISEG_CONV_ZINS): TransitionUp
                if x3 or x2 is not None or self.pad != 0:
                    raise RuntimeError('zero-inserted input: plain single-source valid layers')
                H, W = 2 * H + 3, 2 * W + 3
            # x1 as a channel slice of a wider C8 tensor (a dense block's stack): the parent's channel count
            x1_ctot = 0 if x1.is_contiguous() else c8_ctot(x1)
            if x1_ctot and (x3 or unpool):
                raise RuntimeError('channel-slice input: plain bf16 launches only')
            if x2 is not None:
                if not is_c8(x2) or x2.shape[0] != B or tuple(x2.shape[2:4]) != (H, W):
                    raise RuntimeError('concat shapes %s vs %s' % (tuple(x1.shape), tuple(x2.shape)))
                C2 = x2.shape[1] * 8
                if C1 + C2 != self.Cin:
                    raise RuntimeError('C8 concat needs unpadded sources')
            if C1 + C2 < self.Cin or C1 % 16 or C2 % 16:
                raise RuntimeError('conv expects %d input channels in whole 16-channel groups, got '
                                   '%d + %d chunks' % (self.Cin, C1 // 8, C2 // 8))
        fullH, fullW = self.out_hw(H, W)
        oy0, ox0, OH, OW = window if window is not None else (0, 0, fullH, fullW)
        if not store_out and pool_out is not None:
            # only the pool is kept: the unpaired last row / column of an odd map (Pool2DLayer
            # ignore_border) feeds nothing -- do not compute it
            OH, OW = max(OH & ~1, 2 if OH > 1 else 1), max(OW & ~1, 2 if OW > 1 else 1)
        fmt = out_format or ('c8' if self.Cout % 8 == 0 else 'nchw')
        if m16 and fmt not in ('c8', 'nchw'):
            raise RuntimeError('16-channel C8 layer: bf16 C8 or fp32 NCHW output')
        kind = {'c8': 1, 'c8f32': 2, 'nchw': 3}[fmt]
        if add is not None:
            add_kind = 1 if is_c8(add) else 2
            if add.dim() != 5 or add.shape[0] != B or \
                    add.shape[1] != c8_chunks(self.Cout) * (pair if add_kind == 1 else 1) or \
                    add.dtype not in (torch.bfloat16, torch.float32):
                raise RuntimeError('add tensor shape %s' % (tuple(add.shape),))
            add_geom = (add.shape[2], add.shape[3], add_off[0], add_off[1])
        if place is not None:
            if out is None:
                raise RuntimeError('placement needs a target')
            place = (out.shape[2], out.shape[3], int(place[0]), int(place[1]))
        if not store_out:
            if pool_out is None:
                raise RuntimeError('store_out=False needs pool_out')
            out, kind = None, 0            # (placement geometry taken above; nothing is written)
        out, out_slice = self._c8_target(x1, OH, OW, fmt, out, out_c0, place is not None, store_out, m16)
        if bn is not None and (len(bn) != 2 or any(t.dtype != torch.float32 or t.numel() < C1 for t in bn)):
            raise RuntimeError('bn = (a, b): float32, at least %d entries' % C1)
        if stats is not None and (fmt != 'c8' or any(t.dtype != torch.float32 for t in stats[:2]) or
                                  min(stats[0].numel(), stats[1].numel()) < (out_c0 or 0) + 16):
            raise RuntimeError('stats = (mean, inv_std, eps): float32 vectors covering the produced slice, C8 output')
        if fold is not None and (stats is None or any(t.dtype != torch.float32 or t.numel() < fold[4]
                                                      for t in fold[:4])):
            raise RuntimeError('fold = (beta, gamma, a, b, n) needs stats and float32 vectors of n entries')
        if pool_out is not None:
            oc8 = c8_chunks(self.Cout)
            if not is_c8(pool_out) or tuple(pool_out.shape) != (B, oc8 * pair, fullH // 2, fullW // 2, 8):
                raise RuntimeError('pool_out shape %s' % (tuple(pool_out.shape),))
            if mask_out is not None and (not is_c8_mask(mask_out) or
                                         tuple(mask_out.shape) != (B, oc8, fullH // 2, fullW // 2, 8)):
                raise RuntimeError('mask_out: uint8 (B, Cout/8, H/2, W/2, 8)')
        elif mask_out is not None and not m16:
            raise RuntimeError('mask_out needs pool_out')
        if not m16 and out is not None and is_c8(out) and not out.is_contiguous():
            c8_ctot(out)                   # (validates the layout of a slice given without out_c0)
        flags = (CONV_RELU if self.relu else 0) | (CONV_UNPOOL if unpool else 0) | (CONV_X3 if x3 else 0) | \
            (CONV_ZINS if zins else 0)
        d = self._fill(B, C1, C2, H, W, (oy0, ox0, OH, OW), add_geom, flags, out_slice, place)
        return _Launch(d, x1, x2, None, None, add, out, pool_out, mask_in, mask_out, x1_ctot, add_kind, kind,
                       bn, stats, fold)

    def _c8_profile_info(self, c, m16=False):
        """The CONV_PROFILE_INFO record of a C8 launch (`flat`: its pixel tiling)."""
        if CONV_PROFILE is not None and CONV_PROFILE_INFO is not None:
            d = c.d
            CONV_PROFILE_INFO.append(dict(
                Cin=self.Cin, Cout=self.Cout, C1=d.C1, C2=d.C2, H=d.H, W=d.W, OH=d.OH, OW=d.OW, B=d.B,
                unpool=c.mask_in is not None, pool=c.pool_out is not None, add=c.add_kind, kind=c.kind,
                flat='m16' if m16 else self.c8_tiling(d, c.pool_out is not None)))

    def _run_c8(self, c):
        """The layer on bf16 C8 activations (include/iiseg.h, iiseg_conv_c8).  (The pool rides in the conv's
        epilogue on every pixel tiling: with pool_out the pixels of a tile are ordered by 2x2 pooling
        windows)"""
        d = c.d
        w16 = self._c8_weights()
        _launch('conv_c8_kernel<x3>' if self.x3 else 'conv_c8_kernel', self.flops(d.B, d.OH, d.OW),
                self.lib.iiseg_conv_c8_slice, C.byref(d), _operand(c.x1), int(c.x1_ctot), _operand(c.x2),
                _operand(c.mask_in), w16, _ptr(self.b), _operand(c.add), c.add_kind, _operand(c.out), c.kind,
                _operand(c.pool_out), _operand(c.mask_out))
        self._c8_profile_info(c)

    def _run_c8_m16(self, c):
        """Layers with at most 16 output channels on bf16 C8 activations (include/iiseg.h, iiseg_conv_c8_m16)."""
        d, (bn_a, bn_b) = c.d, c.bn or (None, None)
        mean, inv_std, eps = c.stats or (None, None, 0.0)
        beta, gamma, a, b, n = c.fold or (None, None, None, None, 0)
        w16 = self._c8_weights()
        # split-K launches (small maps, long channel loops) sum their slices through a scratch buffer
        nws = self.lib.iiseg_conv_c8_m16_workspace_bytes(C.byref(d))
        ws = _workspace('m16', nws, c.x1.device) if nws else None
        _launch('conv_c8_m16_kernel', self.flops(d.B, d.OH, d.OW), self.lib.iiseg_conv_c8_m16_ws,
                C.byref(d), _operand(c.x1), c.x1_ctot, _operand(c.mask_in), _ptr(bn_a), _ptr(bn_b),
                w16, _ptr(self.b), _operand(c.out), c.kind,
                None if ws is None else C.c_void_p(ws.data_ptr()), int(nws),
                _ptr(mean), _ptr(inv_std), float(eps), _ptr(beta), _ptr(gamma), _ptr(a), _ptr(b), int(n))
        self._c8_profile_info(c, m16=True)


DECONV_PHASE = True      # K = 2 stride layers on the output-phase kernel (csrc/deconv_phase.hip)


class Deconv:
    """Small-channel transposed convolution (Lasagne Deconv2DLayer W[in,out,k,k], P3)."""

    def __init__(self, W, b, stride, device='cuda', dtype=torch.float32):
        self.dtype = dtype
        self.W = torch.as_tensor(W).to(dtype).contiguous().to(device)
        self.b = None if b is None else torch.as_tensor(b).to(dtype).contiguous().to(device)
        self.Cin, self.Cout, self.K, k2 = self.W.shape
        if k2 != self.K:
            raise RuntimeError('square kernels only')
        self.stride = int(stride)
        self._wp = None             # weights packed for the output-phase kernel (first call)
        self._wp_desc = None        # the descriptor they were packed for (`refresh`)
        self.last_form = None

    def out_hw(self, H, W):
        return (H - 1) * self.stride + self.K, (W - 1) * self.stride + self.K

    def refresh(self):
        """After `self.W` has been changed IN PLACE (an optimizer step): the output-phase kernel's packed weights
        are made again in the buffer they already have.  No host wait."""
        if self._wp is not None:
            dt = self.dtype
            check(_fn('deconv_phase_pack', dt)(_stream(), C.byref(self._wp_desc), _ptr(self.W, dt),
                                               _ptr(self._wp, dt)), 'iiseg_deconv_phase_pack')

    def __call__(self, x, add=None, add_off=(0, 0), window=None, out=None):
        dt = self.dtype
        B, Cin, H, W = x.shape
        if Cin != self.Cin:
            raise RuntimeError('deconv expects %d channels, got %d' % (self.Cin, Cin))
        fullH, fullW = self.out_hw(H, W)
        oy0, ox0, OH, OW = window if window is not None else (0, 0, fullH, fullW)
        d = DeconvDesc()
        d.B, d.Cin, d.H, d.W, d.Cout, d.K, d.stride = B, Cin, H, W, self.Cout, self.K, self.stride
        d.oy0, d.ox0, d.OH, d.OW = oy0, ox0, OH, OW
        if add is not None:
            d.AH, d.AW, d.ay0, d.ax0 = add.shape[2], add.shape[3], add_off[0], add_off[1]
            if add.shape[0] != B or add.shape[1] != self.Cout:
                raise RuntimeError('add tensor shape %s' % (tuple(add.shape),))
        if out is None:
            out = torch.empty((B, self.Cout, OH, OW), dtype=dt, device=x.device)
        lib = _lib.load()
        # K = 2 stride (the FCN-8 upsamplers): the output-phase kernel, weights packed once per layer
        if DECONV_PHASE and lib.iiseg_deconv_phase_supported(C.byref(d), 0 if add is None else 1,
                                                             1 if dt == torch.float64 else 0):
            if self._wp is None:
                self._wp = torch.empty(lib.iiseg_deconv_phase_weight_elems(C.byref(d)), dtype=dt, device=x.device)
                check(_fn('deconv_phase_pack', dt)(_stream(), C.byref(d), _ptr(self.W, dt), _ptr(self._wp, dt)),
                      'iiseg_deconv_phase_pack')
                self._wp_desc = d
            check(_fn('deconv_phase', dt)(_stream(), C.byref(d), _ptr(x, dt), _ptr(self._wp, dt),
                                          _ptr(self.b, dt), _ptr(add, dt), _ptr(out, dt)), 'iiseg_deconv_phase')
            self.last_form = 'phase'
            return out
        check(_fn('deconv', dt)(_stream(), C.byref(d), _ptr(x, dt), _ptr(self.W, dt),
                                _ptr(self.b, dt), _ptr(add, dt), _ptr(out, dt)), 'iiseg_deconv')
        self.last_form = 'gather'
        return out


def is_c8(t):
    """True for a bf16 C8 activation tensor: (B, C/8, H, W, 8) bfloat16 (include/iiseg.h)."""
    return isinstance(t, torch.Tensor) and t.dtype == torch.bfloat16 and t.dim() == 5 and \
        t.shape[-1] == 8


def c8_ctot(t):
    """Channels per image of the C8 TENSOR the operand `t` lies in: `t` may be a channel slice
    `parent[:, c0 // 8:c1 // 8]` of a contiguous C8 tensor (a dense block's stack inside the buffer of its
    resolution) -- same image stride as the parent, data pointer at the slice's first chunk plane.  Raises
    for any other non-contiguous layout."""
    if not is_c8(t):
        raise RuntimeError('expected a bf16 C8 tensor')
    B, C8n, H, W, _ = t.shape
    st = t.stride()
    if tuple(st[1:]) != (H * W * 8, W * 8, 8, 1) or (B > 1 and (st[0] % (H * W * 8) or st[0] < C8n * H * W * 8)):
        raise RuntimeError('C8 operand: a contiguous tensor or a channel slice of one, got strides %s' % (st,))
    return C8n * 8 if B == 1 else st[0] // (H * W * 8) * 8


def c8_first_channels(x8, in_c, Cin):
    """(n, ok): the first `in_c` channels (None: all of them) of the C8 stack `x8` as the input of a layer
    with `Cin` input channels -- ok if they are whole 16-channel groups of the stack that cover the layer
    with less than one group of padding channels."""
    n = x8.shape[1] * 8 if in_c is None else int(in_c)
    return n, not (n % 16 or n > x8.shape[1] * 8 or n < Cin or n - Cin >= 16)


def _c8ptr(t, dtype=torch.bfloat16):
    """A C8 operand that may be a channel slice of a wider tensor (`c8_ctot` validates such layouts)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError('iiseg ops need device tensors (got %s)' % t.device)
    if t.dtype != dtype:
        raise RuntimeError('expected %s, got %s' % (dtype, t.dtype))
    return C.c_void_p(t.data_ptr())


def _operand(t):
    """An operand of a C8 launch: a bf16 C8 tensor (or channel slice), else a contiguous one of its dtype."""
    return None if t is None else (_c8ptr(t) if is_c8(t) else _ptr(t, t.dtype))


def is_c8_mask(t):
    return isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.dim() == 5 and t.shape[-1] == 8


def c8_chunks(channels):
    """Chunks of a C8 tensor holding `channels` channels: whole 16-channel k-tiles."""
    return (int(channels) + 15) // 16 * 2


def empty_c8(B, channels, H, W, device, dtype=torch.bfloat16, x3=False):
    """x3: the hi / lo pair of the 'bf16x3' mode, (B, 2 C/8, H, W, 8) (include/iiseg.h,
    IISEG_CONV_X3)."""
    return torch.empty((B, c8_chunks(channels) * (2 if x3 else 1), H, W, 8), dtype=dtype, device=device)


def nchw_to_c8(x, out=None, x3=False):
    """fp32 NCHW -> bf16 C8 (channels padded with zeros to a whole 16-channel group); x3: the
    hi / lo pair."""
    B, Cc, H, W = x.shape
    if out is None:
        out = empty_c8(B, Cc, H, W, x.device, x3=x3)
    if tuple(out.shape) != (B, c8_chunks(Cc) * (2 if x3 else 1), H, W, 8) or not is_c8(out):
        raise RuntimeError('nchw_to_c8 target %s' % (tuple(out.shape),))
    fn = _lib.load().iiseg_nchw_to_c8x3 if x3 else _lib.load().iiseg_nchw_to_c8
    check(fn(_stream(), _ptr(x), C.c_void_p(out.data_ptr()), B, Cc, H, W, c8_chunks(Cc)),
          'iiseg_nchw_to_c8')
    return out


def nchw_to_c8_slice(x, out8, c0):
    """fp32 NCHW (B, C, H, W) -> channels [c0, c0 + C) of the wider C8 tensor `out8` (c0 % 8 == 0; a
    partial last chunk is zero-padded)."""
    B, Cc, H, W = x.shape
    if not is_c8(out8) or c0 % 8 or tuple(out8.shape[2:4]) != (H, W) or out8.shape[0] != B:
        raise RuntimeError('nchw_to_c8_slice target %s @%d' % (tuple(out8.shape), c0))
    check(_lib.load().iiseg_nchw_to_c8_slice(_stream(), _ptr(x), C.c_void_p(out8.data_ptr()), B, Cc, H, W,
                                             c8_ctot(out8) // 8, c0 // 8), 'iiseg_nchw_to_c8_slice')
    return out8


def c8_slice_to_nchw(x8, c0, channels, out=None):
    """Channels [c0, c0 + channels) of the C8 tensor `x8` -> fp32 NCHW."""
    if not is_c8(x8) or c0 % 8:
        raise RuntimeError('c8_slice_to_nchw needs a C8 tensor and c0 % 8 == 0')
    B, _, H, W, _ = x8.shape
    C8n = c8_ctot(x8) // 8
    if out is None:
        out = torch.empty((B, int(channels), H, W), dtype=torch.float32, device=x8.device)
    check(_lib.load().iiseg_c8_slice_to_nchw(_stream(), C.c_void_p(x8.data_ptr()), _ptr(out), B, int(channels),
                                             H, W, C8n, c0 // 8), 'iiseg_c8_slice_to_nchw')
    return out


def c8x3_to_float(t):
    """hi / lo pair (B, 2 C/8, H, W, 8) -> float32 (B, C/8 * 8, H, W) (torch; tests and debugging)."""
    B, C2, H, W, _ = t.shape
    v = t[:, :C2 // 2].to(torch.float32) + t[:, C2 // 2:].to(torch.float32)
    return v.permute(0, 1, 4, 2, 3).reshape(B, C2 // 2 * 8, H, W)


def c8_to_nchw(x8, channels, out=None, x3=False):
    """bf16 C8 -> fp32 NCHW (first `channels` channels); x3: from the hi / lo pair."""
    if not is_c8(x8) or not x8.is_contiguous() or (x3 and x8.shape[1] % 2):
        raise RuntimeError('c8_to_nchw needs a contiguous C8 tensor')
    B, C8n, H, W, _ = x8.shape
    if x3:
        C8n //= 2
    if out is None:
        out = torch.empty((B, int(channels), H, W), dtype=torch.float32, device=x8.device)
    fn = _lib.load().iiseg_c8x3_to_nchw if x3 else _lib.load().iiseg_c8_to_nchw
    check(fn(_stream(), C.c_void_p(x8.data_ptr()), _ptr(out), B, int(channels), H, W, C8n),
          'iiseg_c8_to_nchw')
    return out


class ConvC8Dil:
    """One 'valid' K x K layer (K = 1 or 3, dilation 1, 2, 4, 8 or 16, at most 16 channels on either side) on
    bf16 C8 activations: the context module's 16-bit leg (csrc/conv_c8_dil.hip).  `W` is
    the layer's float32 parameter on the device in layout 'oihw' (W[out,in,k,k]) or 'iohw' (W[in,out,k,k]); it may
    be a VIEW of a larger buffer, and a slice of it along the input channels (conv1's y half): it is read
    through its strides and never copied.  The bf16 operand images are packed once, here; `refresh()` packs
    them again, into the same buffer, after `W` has been changed in place."""
    kernel = 'conv_c8_dil_kernel'

    def __init__(self, W, b, relu, dil=1, layout='oihw', device='cuda'):
        self.lib = _lib.load()
        if layout not in ('oihw', 'iohw'):
            raise ValueError(layout)
        if not isinstance(W, torch.Tensor) or W.dtype != torch.float32 or W.dim() != 4 or W.shape[2] != W.shape[3] \
                or (b is not None and (not isinstance(b, torch.Tensor) or b.dtype != torch.float32)):
            raise RuntimeError('ConvC8Dil needs float32 tensors W (4-d, square filter) and b')
        if not bool(torch.isfinite(W).all()) or (b is not None and not bool(torch.isfinite(b).all())):
            raise ValueError('non-finite convolution parameters (NaN / Inf in W or b)')
        self.W = W.to(device)
        self.b = None if b is None else b.to(device).contiguous()
        self.layout, self.relu, self.dil = layout, bool(relu), int(dil)
        self.K = int(W.shape[2])
        st = self.W.stride()
        if st[3] != 1 or st[2] != self.K:
            raise RuntimeError('ConvC8Dil: the filter taps of W must be contiguous (strides %s)' % (st,))
        if layout == 'oihw':
            (self.Cout, self.Cin), (self.so, self.sc) = W.shape[:2], st[:2]
        else:
            (self.Cin, self.Cout), (self.sc, self.so) = W.shape[:2], st[:2]
        # (the smallest legal map: what the packer's argument check needs of a geometry)
        self._pack_desc = self._desc(1, self.dil * (self.K - 1) + 1, self.dil * (self.K - 1) + 1, None, False)
        nbytes = _count(self.lib.iiseg_conv_c8_dil_pack_bytes(self.K), 'iiseg_conv_c8_dil_pack_bytes')
        self.wpack = torch.empty(nbytes // 2, dtype=torch.bfloat16, device=device)
        self._descs = {}
        self.refresh()

    def _desc(self, B, H, W, place, nchw):
        d = _lib.C8DilDesc()
        d.B, d.Cin, d.Cout, d.H, d.W, d.K, d.dil = int(B), self.Cin, self.Cout, int(H), int(W), self.K, self.dil
        if place is not None:
            d.out_H, d.out_W, d.out_y0, d.out_x0 = (int(v) for v in place)
        d.flags = (CONV_RELU if self.relu else 0) | (_lib.C8DIL_OUT_NCHW if nchw else 0)
        check(self.lib.iiseg_conv_c8_dil_check(C.byref(d)), 'iiseg_conv_c8_dil_check')
        return d

    def refresh(self):
        """Packs the bf16 operand images again from `self.W`, into the buffer it already has (launches that
        hold its address -- a captured graph -- see the new weights).  No host wait."""
        check(self.lib.iiseg_conv_c8_dil_pack(_stream(), C.byref(self._pack_desc), _ptr_strided(self.W),
                                              self.so, self.sc, C.c_void_p(self.wpack.data_ptr())),
              'iiseg_conv_c8_dil_pack')

    def out_hw(self, H, W):
        return H - self.dil * (self.K - 1), W - self.dil * (self.K - 1)

    def flops(self, B, OH, OW):
        """Nominal 2*Cin*Cout*k*k*OH*OW*B (SURVEY 6.2 convention)."""
        return 2.0 * self.Cin * self.Cout * self.K * self.K * OH * OW * B

    def __call__(self, x8, add=None, out=None, place=None, out_format='c8'):
        """x8: bf16 C8 (B, 2, H, W, 8), channels >= Cin zeros.  add: fp32 (B, Cout, OH, OW), added behind the
        bias.  out_format 'c8': a bf16 C8 tensor of two chunks -- `out` with `place=(y0, x0)`: the map goes to
        that offset of the larger `out`, whose other elements are not touched -- or 'nchw': fp32
        (B, Cout, OH, OW)."""
        if out_format not in ('c8', 'nchw'):
            raise ValueError("out_format must be 'c8' or 'nchw'")
        nchw = out_format == 'nchw'
        if not is_c8(x8) or x8.shape[1] != 2 or not x8.is_contiguous():
            raise RuntimeError('ConvC8Dil needs a contiguous bf16 C8 tensor of two chunks, got %s'
                               % (tuple(x8.shape),))
        B, _, H, W, _ = x8.shape
        OH, OW = self.out_hw(H, W)
        if place is not None and (out is None or nchw):
            raise RuntimeError('ConvC8Dil: `place` needs a C8 `out`')
        geom = None if place is None else (out.shape[2], out.shape[3], place[0], place[1])
        key = (B, H, W, geom, nchw)
        d = self._descs.get(key)
        if d is None:
            d = self._descs[key] = self._desc(B, H, W, geom, nchw)
        if nchw:
            if out is None:
                out = torch.empty((B, self.Cout, OH, OW), dtype=torch.float32, device=x8.device)
            if tuple(out.shape) != (B, self.Cout, OH, OW):
                raise RuntimeError('ConvC8Dil: out %s' % (tuple(out.shape),))
            optr = _ptr(out)
        else:
            if out is None:
                out = empty_c8(B, 16, OH, OW, x8.device)
            want = (B, 2, OH, OW, 8) if place is None else (B, 2, out.shape[2], out.shape[3], 8)
            if not is_c8(out) or tuple(out.shape) != want or not out.is_contiguous():
                raise RuntimeError('ConvC8Dil: out %s' % (tuple(out.shape),))
            optr = _c8ptr(out)
        if add is not None and tuple(add.shape) != (B, self.Cout, OH, OW):
            raise RuntimeError('ConvC8Dil: add %s for an output (%d, %d, %d, %d)'
                               % (tuple(add.shape), B, self.Cout, OH, OW))
        if CONV_PROFILE is not None:
            _add_bytes(self.kernel, B * (32 * H * W + (4 * self.Cout if nchw else 32) * OH * OW))
        _launch(self.kernel, self.flops(B, OH, OW), self.lib.iiseg_conv_c8_dil, C.byref(d), _c8ptr(x8),
                C.c_void_p(self.wpack.data_ptr()), _ptr(self.b), _ptr(add), optr)
        return out


def _ptr_strided(t):
    """Device address of a float32 tensor that is read through explicit strides (a view of a parameter)."""
    if not t.is_cuda:
        raise RuntimeError('iiseg ops need device tensors (got %s)' % t.device)
    if t.dtype != torch.float32:
        raise RuntimeError('expected %s, got %s' % (torch.float32, t.dtype))
    return C.c_void_p(t.data_ptr())


def unpool_c8(up, mask, out, window=None):
    """DePool2D materialised on C8 tensors (include/iiseg.h iiseg_unpool_c8): `out` (B, C8, H, W, 8) <- up
    (B, C8, H/2, W/2, 8) under the mask bytes, for the pooled-coordinate `window` (y0, x0, h, w) (default: all);
    the rest of `out` is left as it is."""
    B, C8n, H, W, _ = out.shape
    if not (is_c8(up) and is_c8(out) and is_c8_mask(mask)) or tuple(up.shape) != (B, C8n, H // 2, W // 2, 8) or \
            tuple(mask.shape) != tuple(up.shape) or not (up.is_contiguous() and out.is_contiguous() and
                                                          mask.is_contiguous()):
        raise RuntimeError('unpool_c8: up %s mask %s out %s' % (tuple(up.shape), tuple(mask.shape), tuple(out.shape)))
    y0, x0, wh, ww = window if window is not None else (0, 0, H // 2, W // 2)
    check(_lib.load().iiseg_unpool_c8(_stream(), _c8ptr(up), C.c_void_p(mask.data_ptr()), _c8ptr(out), B * C8n,
                                      H, W, int(y0), int(x0), int(wh), int(ww)), 'iiseg_unpool_c8')
    return out


def _c8_pooled_out(like, out, window, what):
    """`out` of a windowed element-wise C8 launch: a bf16 C8 tensor of `like`'s shape.  None: a new one, zeros when
    a window leaves part of it unwritten."""
    if out is None:
        return torch.empty(like, dtype=torch.bfloat16, device=what.device) if window is None else \
            torch.zeros(like, dtype=torch.bfloat16, device=what.device)
    if not is_c8(out) or tuple(out.shape) != tuple(like) or not out.is_contiguous():
        raise RuntimeError('C8 output target %s for %s' % (tuple(out.shape), tuple(like)))
    return out


def depool_bwd_c8(gu, mask, out=None, window=None, gate=None):
    """Adjoint of DePool2D on C8 tensors (include/iiseg.h iiseg_depool_bwd_c8): gu (B, C8, PH, PW, 8) bf16, the
    gradient w.r.t. the unpooled map, summed over the positions each mask byte selects into `out` (B, C8, h2, w2, 8)
    -- `mask`'s shape, PH >= 2 h2, PW >= 2 w2 -- on the pooled-coordinate `window` (y0, x0, h, w) (default: all; the
    rest of a given `out` is left as it is).  `gate` (out's shape): zero where gate <= 0, `relu_gate_c8` in the
    same launch."""
    if not (is_c8(gu) and is_c8_mask(mask)) or tuple(gu.shape[:2]) != tuple(mask.shape[:2]) or \
            not (gu.is_contiguous() and mask.is_contiguous()) or \
            (gate is not None and (not is_c8(gate) or tuple(gate.shape) != tuple(mask.shape) or
                                   not gate.is_contiguous())):
        raise RuntimeError('depool_bwd_c8: gu %s mask %s gate %s' % (tuple(gu.shape), tuple(mask.shape),
                                                                     None if gate is None else tuple(gate.shape)))
    B, C8n, PH, PW, _ = gu.shape
    h2, w2 = mask.shape[2], mask.shape[3]
    out = _c8_pooled_out(mask.shape, out, window, gu)
    y0, x0, wh, ww = window if window is not None else (0, 0, h2, w2)
    if CONV_PROFILE is not None:
        _add_bytes('depool_bwd_c8_kernel', B * C8n * wh * ww * (4 * 16 + 8 + 16 + (16 if gate is not None else 0)))
    _launch('depool_bwd_c8_kernel', 0.0, _lib.load().iiseg_depool_bwd_c8, _c8ptr(gu), C.c_void_p(mask.data_ptr()),
            _c8ptr(gate), _c8ptr(out), B, C8n, PH, PW, h2, w2, int(y0), int(x0), int(wh), int(ww))
    return out


def relu_gate_c8(g, pooled, out=None, window=None):
    """out = g where pooled > 0, else +0, on C8 tensors of one shape (include/iiseg.h iiseg_relu_gate_c8): the ReLU
    half of max-pool + ReLU backward, at pooled resolution (the pool half is DePool2D of the result under the
    level's mask bytes).  `window` as in `depool_bwd_c8`; `out` may be `g`."""
    if not (is_c8(g) and is_c8(pooled)) or tuple(g.shape) != tuple(pooled.shape) or \
            not (g.is_contiguous() and pooled.is_contiguous()):
        raise RuntimeError('relu_gate_c8: g %s pooled %s' % (tuple(g.shape), tuple(pooled.shape)))
    B, C8n, h2, w2, _ = g.shape
    out = _c8_pooled_out(g.shape, out, window, g)
    y0, x0, wh, ww = window if window is not None else (0, 0, h2, w2)
    if CONV_PROFILE is not None:
        _add_bytes('relu_gate_c8_kernel', B * C8n * wh * ww * 48)
    _launch('relu_gate_c8_kernel', 0.0, _lib.load().iiseg_relu_gate_c8, _c8ptr(g), _c8ptr(pooled), _c8ptr(out),
            B, C8n, h2, w2, int(y0), int(x0), int(wh), int(ww))
    return out


def pool_mask_c8(pre, pooled, mask, origin, full_hw, window, x3=False):
    """2x2 max-pool (+ DePool2D mask bytes, `mask` may be None) of the pooled-coordinate `window`
    (y0, x0, h, w) from the stored piece `pre` (C8 bf16, or C8 fp32: the unrounded conv results)
    whose corner sits at `origin` of the `full_hw` map, into the full-size `pooled` / `mask` tensors."""
    B, C8n, PH, PW, _ = pre.shape
    y0, x0, wh, ww = window
    if wh <= 0 or ww <= 0:
        return pooled
    if x3:
        check(_lib.load().iiseg_pool_mask_c8x3(
            _stream(), C.c_void_p(pre.data_ptr()), C.c_void_p(pooled.data_ptr()),
            None if mask is None else C.c_void_p(mask.data_ptr()), B, C8n, PH, PW, int(origin[0]),
            int(origin[1]), int(full_hw[0]), int(full_hw[1]), int(y0), int(x0), int(wh), int(ww)),
            'iiseg_pool_mask_c8x3')
        return pooled
    check(_lib.load().iiseg_pool_mask_c8(
        _stream(), C.c_void_p(pre.data_ptr()), 1 if pre.dtype == torch.float32 else 0,
        C.c_void_p(pooled.data_ptr()),
        None if mask is None else C.c_void_p(mask.data_ptr()), B * C8n, PH, PW, int(origin[0]),
        int(origin[1]), int(full_hw[0]), int(full_hw[1]), int(y0), int(x0), int(wh), int(ww)),
        'iiseg_pool_mask_c8')
    return pooled


def maxpool2x2(x, out=None, window=None, mask=None):
    """`window` = (y0, x0, h, w) in pooled coordinates: only that region of `out` is written.
    `mask` (uint8, out's shape; float32): also the DePool2D mask bytes of those windows (bit
    (y&1)*2+(x&1) = x == out, as a conv's `mask_out`)."""
    B, Cc, H, W = x.shape
    if out is None:
        out = torch.empty((B, Cc, H // 2, W // 2), dtype=x.dtype, device=x.device)
    if mask is not None:
        if x.dtype != torch.float32 or mask.dtype != torch.uint8 or mask.shape != out.shape:
            raise RuntimeError('maxpool2x2 mask: float32 input, uint8 of the pooled shape')
        y0, x0, wh, ww = window if window is not None else (0, 0, H // 2, W // 2)
        check(_lib.load().iiseg_maxpool2x2_mask_window_f32(_stream(), _ptr(x), _ptr(out),
                                                            _ptr(mask, torch.uint8), B * Cc, H, W,
                                                            y0, x0, wh, ww),
              'iiseg_maxpool2x2_mask_window_f32')
        return out
    if window is not None:
        y0, x0, wh, ww = window
        check(_fn('maxpool2x2_window', x.dtype)(_stream(), _ptr(x, x.dtype), _ptr(out, x.dtype),
                                                B * Cc, H, W, y0, x0, wh, ww),
              'iiseg_maxpool2x2_window')
        return out
    check(_fn('maxpool2x2', x.dtype)(_stream(), _ptr(x, x.dtype), _ptr(out, x.dtype), B * Cc, H, W),
          'iiseg_maxpool2x2')
    return out


def unpool_eqmask(up, pre, pooled, out=None, window=None):
    """DePool2D, materialised.  `window` = (y0, x0, h, w): only that region of the (H, W) planes
    is produced (in place in `out`, the rest is left as it is)."""
    B, Cc, H, W = pre.shape
    if tuple(up.shape) != (B, Cc, H // 2, W // 2) or up.shape != pooled.shape:
        raise RuntimeError('unpool shapes: up %s pre %s pooled %s'
                           % (tuple(up.shape), tuple(pre.shape), tuple(pooled.shape)))
    if out is None:
        out = torch.empty_like(pre)
    dt = pre.dtype
    if window is not None:
        y0, x0, wh, ww = window
        check(_fn('unpool_eqmask_window', dt)(_stream(), _ptr(up, dt), _ptr(pre, dt),
                                              _ptr(pooled, dt), _ptr(out, dt), B * Cc, H, W, y0, x0,
                                              wh, ww), 'iiseg_unpool_eqmask_window')
        return out
    check(_fn('unpool_eqmask', dt)(_stream(), _ptr(up, dt), _ptr(pre, dt), _ptr(pooled, dt),
                                   _ptr(out, dt), B * Cc, H, W), 'iiseg_unpool_eqmask')
    return out


def crop_softmax(score, H, W, off=None, out=None, minuend=None):
    """softmax over channels of the (H,W) window of score; `off` defaults to the center crop
    offset (dim - target)//2 (P6).  With `minuend` returns minuend - softmax (de_fn)."""
    B, Cc, SH, SW = score.shape
    sy0, sx0 = off if off is not None else ((SH - H) // 2, (SW - W) // 2)
    dt = score.dtype
    if out is None:
        out = torch.empty((B, Cc, H, W), dtype=dt, device=score.device)
    check(_fn('crop_softmax', dt)(_stream(), _ptr(score, dt), _ptr(minuend, dt), _ptr(out, dt), B,
                                  Cc, SH, SW, sy0, sx0, H, W), 'iiseg_crop_softmax')
    return out


class RefineState:
    """Device-side state of the batched refinement loop: per-image active flag, iteration
    count, last norm and the per-block norm partials (reference loop state of
    iterative_inference.py:258-284 for a whole batch)."""

    def __init__(self, B, H, W, device):
        lib = _lib.load()
        self.B, self.H, self.W = B, H, W
        self.nblk = lib.iiseg_refine_partials(H, W)
        self.active = torch.ones(B, dtype=torch.int32, device=device)
        self.iters = torch.zeros(B, dtype=torch.int32, device=device)
        self.last_norm = torch.zeros(B, dtype=torch.float64, device=device)
        self.partial = torch.zeros(B * self.nblk, dtype=torch.float64, device=device)

    def reset(self):
        self.active.fill_(1)
        self.iters.zero_()
        self.last_norm.zero_()


def refine_update(score, y, state, step, off=None, y8=None):
    """One fused refinement step on y (in place) from the DAE's pre-softmax score map.  `y8`: a
    bf16 C8 tensor (B, chunks, H, W, 8) that also receives the updated map (the DAE's input format
    under mma='bf16c8'; float32 only)."""
    B, Cc, SH, SW = score.shape
    H, W = y.shape[2], y.shape[3]
    sy0, sx0 = off if off is not None else ((SH - H) // 2, (SW - W) // 2)
    dt = y.dtype
    if y8 is not None:
        if dt != torch.float32 or not is_c8(y8) or tuple(y8.shape) != (B, y8.shape[1], H, W, 8) or \
                y8.shape[1] * 8 < Cc:
            raise RuntimeError('y8: bf16 C8 tensor of y\'s geometry')
        check(_lib.load().iiseg_refine_update_c8_f32(
            _stream(), _ptr(score), _ptr(y), _ptr(state.active, torch.int32),
            _ptr(state.partial, torch.float64), C.c_void_p(y8.data_ptr()), y8.shape[1], B, Cc, SH, SW,
            sy0, sx0, H, W, float(step)), 'iiseg_refine_update_c8_f32')
        return
    check(_fn('refine_update', dt)(_stream(), _ptr(score, dt), _ptr(y, dt),
                                   _ptr(state.active, torch.int32),
                                   _ptr(state.partial, torch.float64), B, Cc, SH, SW, sy0, sx0,
                                   H, W, float(step)), 'iiseg_refine_update')


def sqerr_softmax_bwd(score, y, off=None):
    """dE/dscore for E = sum (softmax(score window) - y)^2 (true-gradient mode)."""
    B, Cc, SH, SW = score.shape
    H, W = y.shape[2], y.shape[3]
    sy0, sx0 = off if off is not None else ((SH - H) // 2, (SW - W) // 2)
    dt = y.dtype
    g = torch.empty_like(y)
    check(_fn('sqerr_softmax_bwd', dt)(_stream(), _ptr(score, dt), _ptr(y, dt), _ptr(g, dt), B, Cc,
                                       SH, SW, sy0, sx0, H, W), 'iiseg_sqerr_softmax_bwd')
    return g


def depool_bwd(gout, pre, pooled):
    """Adjoint of DePool2D w.r.t. its input: masked 2x2 sum of gout (B,C,H,W) -> (B,C,H/2,W/2)."""
    dt = gout.dtype
    B, Cc, H, W = pre.shape
    out = torch.empty_like(pooled)
    check(_fn('depool_bwd', dt)(_stream(), _ptr(gout, dt), _ptr(pre, dt), _ptr(pooled, dt),
                                _ptr(out, dt), B * Cc, H, W), 'iiseg_depool_bwd')
    return out


def pool_relu_bwd(gpool, pre, pooled):
    """Adjoint of maxpool2x2(relu(z)) w.r.t. z, given pre = relu(z) and pooled."""
    dt = gpool.dtype
    B, Cc, H, W = pre.shape
    out = torch.empty_like(pre)
    check(_fn('pool_relu_bwd', dt)(_stream(), _ptr(gpool, dt), _ptr(pre, dt), _ptr(pooled, dt),
                                   _ptr(out, dt), B * Cc, H, W), 'iiseg_pool_relu_bwd')
    return out


def grad_update(score, gthrough, y, state, step, off=None):
    """True-gradient step on y (in place): grad = gthrough - 2 (softmax(score) - y)."""
    B, Cc, SH, SW = score.shape
    H, W = y.shape[2], y.shape[3]
    sy0, sx0 = off if off is not None else ((SH - H) // 2, (SW - W) // 2)
    dt = y.dtype
    check(_fn('grad_update', dt)(_stream(), _ptr(score, dt), _ptr(gthrough, dt), _ptr(y, dt),
                                 _ptr(state.active, torch.int32),
                                 _ptr(state.partial, torch.float64), B, Cc, SH, SW, sy0, sx0, H, W,
                                 float(step)), 'iiseg_grad_update')


def refine_finalize(state, eps, nblk=None):
    """`nblk`: partials per image the update kernel wrote (default: those of iiseg_refine_update_*; the context
    module's fused tail writes one per 16 x 64 tile, `ctx_tail`)."""
    lib = _lib.load()
    check(lib.iiseg_refine_finalize(_stream(), _ptr(state.partial, torch.float64),
                                    _ptr(state.active, torch.int32),
                                    _ptr(state.iters, torch.int32),
                                    _ptr(state.last_norm, torch.float64), state.B,
                                    state.nblk if nblk is None else int(nblk),
                                    state.H * state.W, float(eps)), 'iiseg_refine_finalize')


CTX_TAIL = os.environ.get('IISEG_CTX_TAIL', '1') != '0'


def ctx_tail_supported(conv6, conv7, y):
    """Can `ctx_tail` run these two layers on this map?  (fp32, 3x3 'valid' dilation 1 + ReLU, then 1x1
    linear, 12 to 16 padded channels on either side.)"""
    Cc = y.shape[1]
    return (CTX_TAIL and y.dtype == torch.float32 and conv6.dtype == torch.float32 and
            (conv6.KH, conv6.KW, conv6.dil, conv6.pad, conv6.relu) == (3, 3, 1, 0, True) and
            (conv7.KH, conv7.KW, conv7.pad, conv7.relu) == (1, 1, 0, False) and
            conv6.Cin == conv6.Cout == conv7.Cin == conv7.Cout == Cc and 9 <= Cc <= 16 and
            not conv6.transposed and not conv7.transposed)


def ctx_tail(conv6, conv7, x, y, state, step, ycat=None, cat_c0=0, cat_off=(0, 0)):
    """The context module's last two layers + the refinement update as ONE launch (include/iiseg.h,
    iiseg_ctx_tail_f32): x (B, C, H + 2, W + 2) -> y (B, C, H, W) updated in place (and mirrored into channels
    [cat_c0, cat_c0 + C) of `ycat` at `cat_off`).  Returns the number of norm partials per image it wrote
    (pass it to `refine_finalize`)."""
    lib = _lib.load()
    B, Cc, H, W = y.shape
    if tuple(x.shape) != (B, Cc, H + 2, W + 2):
        raise RuntimeError('ctx_tail: x %s for y %s' % (tuple(x.shape), tuple(y.shape)))
    d6, wp6, _ = conv6._plan(B, Cc, 0, H + 2, W + 2, None, None, False)
    d7, wp7, _ = conv7._plan(B, Cc, 0, H, W, None, None, False)
    nblk = lib.iiseg_ctx_tail_partials(H, W)
    if B * nblk > state.partial.numel():
        raise RuntimeError('ctx_tail: the state holds %d partials, %d needed' % (state.partial.numel(), B * nblk))
    cat = (0, 0, 0, 0, 0, 0)
    if ycat is not None:
        if ycat.dim() != 4 or ycat.shape[0] != B or ycat.dtype != torch.float32:
            raise RuntimeError('ctx_tail: ycat %s' % (tuple(ycat.shape),))
        cat = (ycat.shape[1], int(cat_c0), ycat.shape[2], ycat.shape[3], int(cat_off[0]), int(cat_off[1]))
    kern = 'ctx_tail_kernel'
    _launch(kern, conv6.flops(B, H, W) + conv7.flops(B, H, W), lib.iiseg_ctx_tail_f32,
            _ptr(x), _ptr(wp6), d6.Mpad, _ptr(conv6.b), _ptr(wp7), d7.Mpad, _ptr(conv7.b), _ptr(y),
            _ptr(state.active, torch.int32), _ptr(state.partial, torch.float64), _ptr(ycat), *cat, B, Cc, H, W,
            float(step))
    if CONV_PROFILE is not None:
        # algorithmic bytes: x planes read, y read and written, the mirror written
        _add_bytes(kern, 4.0 * B * Cc * ((H + 2) * (W + 2) + (3 if ycat is not None else 2) * H * W))
    return nblk


def count_nonfinite(x, counter):
    """counter (int32, 1 element, device) += NaN / Inf elements of x (no synchronisation)."""
    check(_fn('count_nonfinite', x.dtype)(_stream(), _ptr(x, x.dtype), int(x.numel()),
                                          _ptr(counter, torch.int32)), 'iiseg_count_nonfinite')


def confusion_accumulate(y, t, cm, sums, active=None):
    """cm (C*(C+1)) int64 and sums (2) float64 are accumulated in place; with `active` (B int32)
    only images whose flag is non-zero are counted."""
    B, Cc, H, W = y.shape
    if tuple(t.shape) != (B, Cc + 1, H, W):
        raise RuntimeError('target must be one-hot (B,C+1,H,W) with void last, got %s'
                           % (tuple(t.shape),))
    dt = y.dtype
    if active is not None:
        check(_fn('confusion_masked', dt)(_stream(), _ptr(y, dt), _ptr(t, dt),
                                          _ptr(active, torch.int32), _ptr(cm, torch.int64),
                                          _ptr(sums, torch.float64), B, Cc, H * W),
              'iiseg_confusion_masked')
        return
    check(_fn('confusion', dt)(_stream(), _ptr(y, dt), _ptr(t, dt), _ptr(cm, torch.int64),
                               _ptr(sums, torch.float64), B, Cc, H * W), 'iiseg_confusion')




class Conv1x1C8:
    """A 1x1 layer on a bf16 C8 tensor (csrc/conv1x1_c8.hip; include/iiseg.h iiseg_conv1x1_c8): FC-DenseNet's
    TransitionDown (`bn` + `pool=True`: BN -> ReLU -> 1x1 conv -> 2x2 max-pool into a slice of the next
    stack) and its 1x1 class-score layer (`pool=False`: fp32 NCHW).  W (Cout, Cin, 1, 1), b (Cout) or None."""

    def __init__(self, W, b, device='cuda'):
        self.lib = _lib.load()
        self.W = torch.as_tensor(W).to(torch.float32).contiguous().to(device)
        self.b = None if b is None else torch.as_tensor(b).to(torch.float32).contiguous().to(device)
        if self.W.dim() != 4 or tuple(self.W.shape[2:]) != (1, 1):
            raise ValueError('Conv1x1C8 takes (Cout, Cin, 1, 1) filters')
        self.Cout, self.Cin = int(self.W.shape[0]), int(self.W.shape[1])
        self._wp = {}

    def flops(self, B, H, W):
        return 2.0 * self.Cin * self.Cout * H * W * B

    def __call__(self, x8, in_c=None, bn=None, pool=False, out=None, out_c0=0):
        in_ctot = c8_ctot(x8)            # (a contiguous C8 tensor or a channel slice of one)
        B, C8n, H, W, _ = x8.shape
        cin, ok = c8_first_channels(x8, in_c, self.Cin)
        if not ok:
            raise RuntimeError('Conv1x1C8: %d input channels of %d (layer: %d)' % (cin, C8n * 8, self.Cin))
        wp = self._wp.get(cin)
        if wp is None:
            n = self.lib.iiseg_conv1x1_c8_weight_bytes(self.Cout, cin)
            wp = self._wp[cin] = torch.empty(int(n) // 2, dtype=torch.bfloat16, device=self.W.device)
            check(self.lib.iiseg_conv1x1_c8_pack(_stream(), _ptr(self.W), self.Cin, 1, self.Cout, self.Cin, cin,
                                                 _ptr(wp, torch.bfloat16)), 'iiseg_conv1x1_c8_pack')
        if pool:
            if out is None:
                out = torch.zeros((B, c8_chunks(self.Cout), H // 2, W // 2, 8), dtype=torch.bfloat16,
                                  device=x8.device)
                out_c0 = 0
            if not is_c8(out) or out.shape[0] != B or tuple(out.shape[2:4]) != (H // 2, W // 2) or \
                    out_c0 + self.Cout > out.shape[1] * 8:
                raise RuntimeError('Conv1x1C8 pool target %s' % (tuple(out.shape),))
            octot = c8_ctot(out)
        else:
            if out is None:
                out = torch.empty((B, self.Cout, H, W), dtype=torch.float32, device=x8.device)
            if tuple(out.shape) != (B, self.Cout, H, W) or out.dtype != torch.float32 or not out.is_contiguous():
                raise RuntimeError('Conv1x1C8 target %s' % (tuple(out.shape),))
            octot = 0
        a, b_ = bn if bn is not None else (None, None)
        if a is not None and (a.numel() < cin or b_.numel() < cin):
            raise RuntimeError('Conv1x1C8: folded BN vectors shorter than the input')
        _launch('conv1x1_c8_kernel', self.flops(B, H, W), self.lib.iiseg_conv1x1_c8,
                C.c_void_p(x8.data_ptr()), B, cin, in_ctot, H, W, _ptr(a), _ptr(b_), _ptr(wp, torch.bfloat16),
                _ptr(self.b), self.Cout, 1 if pool else 0, C.c_void_p(out.data_ptr()), octot, int(out_c0))
        return out


def bn_fold(beta, gamma, mean, inv_std, n, a=None, b=None, cap=None):
    """(a, b) with max(a x + b, 0) == relu(BatchNorm(x)) for the first n channels (float32 vectors of
    `cap` >= n entries, zero beyond n): the input-side BN + ReLU of the 16-channel C8 layers."""
    cap = int(cap or n)
    if a is None:
        a = torch.zeros(cap, dtype=torch.float32, device=beta.device)
        b = torch.zeros(cap, dtype=torch.float32, device=beta.device)
    check(_lib.load().iiseg_bn_fold_f32(_stream(), _ptr(beta), _ptr(gamma), _ptr(mean), _ptr(inv_std),
                                        _ptr(a), _ptr(b), int(n)), 'iiseg_bn_fold_f32')
    return a, b


def bn_stats_c8(buf8, c0, n, mean, inv_std, eps=1e-4):
    """Batch statistics (P10) of channels [c0, c0 + n) of the C8 tensor `buf8` into mean[c0:c0+n],
    inv_std[c0:c0+n] (float32 vectors)."""
    lib = _lib.load()
    B, C8n, H, W, _ = buf8.shape
    ctot = c8_ctot(buf8)
    ws = _workspace('bn', lib.iiseg_bn_stats_c8_workspace_elems(int(n)), buf8.device)
    check(lib.iiseg_bn_stats_c8(_stream(), _c8ptr(buf8), B, ctot, int(c0), int(n), H, W,
                                float(eps), _ptr(mean), _ptr(inv_std), _ptr(ws, torch.float64)),
          'iiseg_bn_stats_c8')


def bn_stats(buf, c0, n, mean, inv_std, eps=1e-4):
    """Batch statistics (P10) of channels [c0, c0+n) of `buf` (B, Ctot, H, W) into
    mean[c0:c0+n], inv_std[c0:c0+n] (1-D tensors of length >= c0+n)."""
    B, Ctot, H, W = buf.shape
    dt = buf.dtype
    item = buf.element_size()
    _ptr(buf, dt), _ptr(mean, dt), _ptr(inv_std, dt)
    xp = C.c_void_p(buf.data_ptr() + c0 * H * W * item)
    ws = _workspace('bn', _lib.load().iiseg_bn_stats_workspace_elems(n), buf.device)
    check(_fn('bn_stats', dt)(_stream(), xp, Ctot * H * W, B, n, H * W, float(eps),
                              C.c_void_p(mean.data_ptr() + c0 * item),
                              C.c_void_p(inv_std.data_ptr() + c0 * item),
                              _ptr(ws, torch.float64)), 'iiseg_bn_stats')


def bn_relu(buf, n, beta, gamma, mean, inv_std, out=None):
    """relu((x - mean) * (gamma * inv_std) + beta) of the first n channels of `buf`
    (B, Ctot, H, W) -> dense (B, n, H, W)."""
    B, Ctot, H, W = buf.shape
    dt = buf.dtype
    if out is None:
        out = torch.empty((B, n, H, W), dtype=dt, device=buf.device)
    check(_fn('bn_relu', dt)(_stream(), _ptr(buf, dt), Ctot * H * W, B, n, H * W, _ptr(beta, dt),
                             _ptr(gamma, dt), _ptr(mean, dt), _ptr(inv_std, dt), _ptr(out, dt)),
          'iiseg_bn_relu')
    return out


def bn_relu_bwd(stack, n, bn, g_t, gstack, dbeta, dgamma):
    """Backward of t = relu(BatchNorm(stack[:, :n])) with batch statistics for one consumer of the stack (DESIGN.md
    section 21): bn = (beta, gamma, mean, inv_std), g_t = dL/dt dense (B, n, H, W); writes dbeta, dgamma (n entries)
    and ADDS g_x into the first n channels of `gstack` (the stack's shape).  y is recomputed from the stack.  Two
    launches (reduce, apply), deterministic; nothing else is written."""
    B, cap, H, W = stack.shape
    dt = stack.dtype
    n = int(n)
    beta, gamma, mean, inv_std = bn
    if not 0 < n <= cap or tuple(g_t.shape) != (B, n, H, W) or gstack.shape != stack.shape or \
            min(beta.numel(), gamma.numel(), mean.numel(), inv_std.numel(), dbeta.numel(), dgamma.numel()) < n:
        raise RuntimeError('bn_relu_bwd: stack %s n %d g_t %s gstack %s' % (tuple(stack.shape), n, tuple(g_t.shape),
                                                                            tuple(gstack.shape)))
    nws = _count(_lib.load().iiseg_bn_relu_bwd_workspace_elems(n, H * W), 'iiseg_bn_relu_bwd_workspace_elems')
    ws = _workspace('bn', nws, stack.device)
    item = float(stack.element_size())
    planes = item * B * n * H * W
    _launch_staged(_fn('bn_relu_bwd', dt),
                   (_ptr(stack, dt), cap * H * W, _ptr(g_t, dt), _ptr(gstack, dt), B, n, H * W, _ptr(beta, dt),
                    _ptr(gamma, dt), _ptr(mean, dt), _ptr(inv_std, dt), _ptr(dbeta, dt), _ptr(dgamma, dt),
                    _ptr(ws, torch.float64)), _lib.BN_BWD_REDUCE | _lib.BN_BWD_APPLY,
                   (('bn_relu_bwd_reduce_kernel', _lib.BN_BWD_REDUCE, 0.0),
                    ('bn_relu_bwd_apply_kernel', _lib.BN_BWD_APPLY, 0.0)))
    if CONV_PROFILE is not None:
        # byte models: x and g_t read; x, g_t and gstack read, gstack written
        _add_bytes('bn_relu_bwd_reduce_kernel', 2 * planes)
        _add_bytes('bn_relu_bwd_apply_kernel', 4 * planes)


def maxpool2x2_bwd(gpool, pre, pooled):
    """Adjoint of maxpool2x2 alone (no ReLU gate: `pool_relu_bwd` without the > 0 test), given the pooled map's
    input `pre` (B,C,H,W) and `pooled`: every position equal to its window's maximum receives gpool, a trailing
    odd row / column zero."""
    dt = gpool.dtype
    B, Cc, H, W = pre.shape
    if tuple(pooled.shape) != (B, Cc, H // 2, W // 2) or gpool.shape != pooled.shape:
        raise RuntimeError('maxpool2x2_bwd: gpool %s pre %s pooled %s' % (tuple(gpool.shape), tuple(pre.shape),
                                                                         tuple(pooled.shape)))
    out = torch.empty_like(pre)
    kern = 'maxpool2x2_bwd_kernel'
    _launch(kern, 0.0, _fn('maxpool2x2_bwd', dt), _ptr(gpool, dt), _ptr(pre, dt), _ptr(pooled, dt), _ptr(out, dt),
            B * Cc, H, W)
    if CONV_PROFILE is not None:
        _add_bytes(kern, float(pre.element_size()) * (2 * pre.numel() + 2 * pooled.numel()))
    return out


def bn_affine(x, bnp, window=None):
    """In place x = (x - mean) * (gamma * inv_std) + beta per channel (stored-average BatchNorm),
    on the window (y0, x0, h, w) of x's planes or everywhere.  bnp = (beta, gamma, mean, inv_std)."""
    B, Cc, H, W = x.shape
    dt = x.dtype
    y0, x0, wh, ww = window if window is not None else (0, 0, H, W)
    if wh <= 0 or ww <= 0:
        return x
    beta, gamma, mean, inv_std = bnp
    check(_fn('bn_affine_window', dt)(_stream(), _ptr(x, dt), B, Cc, H, W, y0, x0, wh, ww,
                                      _ptr(beta, dt), _ptr(gamma, dt), _ptr(mean, dt),
                                      _ptr(inv_std, dt)), 'iiseg_bn_affine_window')
    return x


def add_noise(x, eps, sigma):
    """x + sigma * eps (GaussianNoiseLayer with the caller's standard-normal sample eps)."""
    dt = x.dtype
    out = torch.empty_like(x)
    check(_fn('add_noise', dt)(_stream(), _ptr(x, dt), _ptr(eps, dt), float(sigma), _ptr(out, dt),
                               x.numel()), 'iiseg_add_noise')
    return out


def gaussian_noise(y, noise, generator=None, eps=None):
    """GaussianNoiseLayer in training mode: y + noise * eps, formed ONCE (`add_noise`); eps = the caller's
    standard-normal sample, else drawn from `generator`.  noise = 0: y itself."""
    if not noise > 0:
        return y
    if eps is None:
        eps = torch.randn(y.shape, generator=generator, device=y.device, dtype=y.dtype)
    return add_noise(y, eps, float(noise))


def dropout_apply(x, keep, p):
    """In place x * keep / (1 - p) (DropoutLayer, rescale=True, with the caller's 0/1 mask)."""
    dt = x.dtype
    check(_fn('dropout_apply', dt)(_stream(), _ptr(x, dt), _ptr(keep, dt), float(p), x.numel()),
          'iiseg_dropout_apply')
    return x


# ---- training the context-module DAE (csrc/ctx_train.hip) ----
LOSS_FLAGS = {'crossentropy': _lib.LOSS_CROSSENTROPY, 'squared_error': _lib.LOSS_SQUARED_ERROR}
OPTIMIZERS = {'rmsprop': _lib.OPT_RMSPROP, 'adam': _lib.OPT_ADAM}


def layout_strides(Cin, Cout, K, layout):
    """(so, sc) of a layer parameter with K x K taps stored as `layout` ('oihw': W[out,in,k,k]; 'iohw':
    W[in,out,k,k]): element (co, ci, tap) lies at co so + ci sc + tap (include/iiseg.h)."""
    if layout == 'oihw':
        return Cin * K * K, K * K
    if layout == 'iohw':
        return K * K, Cout * K * K
    raise ValueError(layout)


def ctx_loss(score, target, losses=('crossentropy',), lmb=1.0, grad=True, res=None, cnt=None, g=None):
    """The reference's training loss on the score map (B,C,H,W) of the context module and the one-hot target
    (B,C+1,H,W; void channel last): returns (res, g, cnt) -- res (3 doubles on the device) = [loss,
    crossentropy, squared_error], g = dloss/dscore (normalised by the batch's mask sums; None with
    grad=False), cnt = [N_ce, N_se, 1/N_ce, 1/N_se].  Two launches on the target (mask counts), two on the
    score map; no host wait."""
    dt = score.dtype
    B, Cc, H, W = score.shape
    if tuple(target.shape) != (B, Cc + 1, H, W) or target.dtype != dt:
        raise RuntimeError('ctx_loss: target %s %s for score %s %s' % (tuple(target.shape), target.dtype,
                                                                      tuple(score.shape), dt))
    flags = 0
    for name in losses:
        if name not in LOSS_FLAGS:
            raise ValueError('ctx_loss: loss %r is not built (crossentropy, squared_error)' % (name,))
        flags |= LOSS_FLAGS[name]
    nblk = _count(_lib.load().iiseg_ctx_loss_partials(B, H, W), 'iiseg_ctx_loss_partials')
    partial = _workspace('bn', 2 * nblk, score.device)
    f64 = torch.float64
    if cnt is None:
        cnt = torch.empty(4, dtype=f64, device=score.device)
    if res is None:
        res = torch.empty(3, dtype=f64, device=score.device)
    if grad and g is None:
        g = torch.empty_like(score)
    _launch('ctx_loss_count_kernel', 0.0, _fn('ctx_loss_count', dt), _ptr(target, dt), _ptr(partial, f64),
            _ptr(cnt, f64), B, Cc, H, W)
    _launch('ctx_loss_kernel', 0.0, _fn('ctx_loss', dt), _ptr(score, dt), _ptr(target, dt), _ptr(cnt, f64),
            _ptr(g, dt) if grad else None, _ptr(partial, f64), _ptr(res, f64), B, Cc, H, W, flags, float(lmb))
    return res, (g if grad else None), cnt


def wgrad_desc(x_shape, Cout, K, dil, layout, gz_place=None):
    """The iiseg_wgrad_desc of a 'valid' layer on x (B,Cin,H,W); gz_place = (gz_H, gz_W, y0, x0)."""
    B, Cin, H, W = x_shape
    d = _lib.WgradDesc()
    d.B, d.Cin, d.Cout, d.H, d.W, d.K, d.dil = int(B), int(Cin), int(Cout), int(H), int(W), int(K), int(dil)
    OH, OW = H - dil * (K - 1), W - dil * (K - 1)
    d.gz_H, d.gz_W, d.gz_y0, d.gz_x0 = (OH, OW, 0, 0) if gz_place is None else tuple(int(v) for v in gz_place)
    d.so, d.sc = layout_strides(Cin, Cout, K, layout)
    return d


def conv_small_wgrad(x, gout, out, dW, db, dil=1, layout='oihw', gz=None, gz_off=(0, 0)):
    """dW, db (written in place, the layer's own parameter layout) of the 'valid' layer that maps x
    (B,Cin,H,W) to `out` (B,Cout,OH,OW) = relu(...) -- or, with out=None, a linear layer -- given gout =
    dL/dout.  gz (optional): receives g_z = gout * [out > 0] at `gz_off` of its (larger) planes."""
    dt = x.dtype
    K = dW.shape[2]
    Cout = dW.shape[0] if layout == 'oihw' else dW.shape[1]
    place = None if gz is None else (gz.shape[2], gz.shape[3], gz_off[0], gz_off[1])
    d = wgrad_desc(tuple(x.shape), Cout, K, dil, layout, place)
    OH, OW = x.shape[2] - dil * (K - 1), x.shape[3] - dil * (K - 1)
    if tuple(gout.shape) != (x.shape[0], Cout, OH, OW) or (out is not None and out.shape != gout.shape) or \
            (gz is not None and tuple(gz.shape[:2]) != (x.shape[0], Cout)) or dW.numel() != x.shape[1] * Cout * K * K \
            or db.numel() != Cout:
        raise RuntimeError('conv_small_wgrad: shapes x %s gout %s dW %s' % (tuple(x.shape), tuple(gout.shape),
                                                                            tuple(dW.shape)))
    nslab = _count(_lib.load().iiseg_conv_small_wgrad_partials(C.byref(d), dW.element_size()),
                   'iiseg_conv_small_wgrad_partials')
    slab = _workspace(_SUFFIX[dt], nslab * (dW.numel() + Cout), x.device)
    kern = 'conv_small_wgrad_kernel'
    _launch(kern, 2.0 * dW.numel() * x.shape[0] * OH * OW, _fn('conv_small_wgrad', dt), C.byref(d), _ptr(x, dt),
            _ptr(gout, dt), _ptr(out, dt), _ptr(gz, dt), _ptr(slab, dt), _ptr(dW, dt), _ptr(db, dt))
    if CONV_PROFILE is not None:
        # byte model: x and g_out read, g_z written, once each
        _add_bytes(kern, float(dW.element_size()) * (x.shape[1] + 2 * Cout) * x.shape[0] * x.shape[2] * x.shape[3])


def opt_step(kind, p, g, s1, s2, lr, state, grid=False):
    """One optimizer step on the flat buffers p, g, s1 (, s2) in place; lr: one element on the device;
    state (adam): [t, 0.9^t, 0.999^t], start [0, 1, 1].  grid=True: the many-workgroup form (the same bits;
    adam's state advanced by a one-thread launch after it) for buffers of millions of scalars."""
    dt = p.dtype
    if not (p.numel() == g.numel() == s1.numel()) or (s2 is not None and s2.numel() != p.numel()):
        raise RuntimeError('opt_step: buffers of different sizes')
    kern, fn = ('opt_step_grid_kernel', 'opt_step_grid') if grid else ('opt_step_kernel', 'opt_step')
    _launch(kern, 0.0, _fn(fn, dt), OPTIMIZERS[kind], _ptr(p, dt), _ptr(g, dt), _ptr(s1, dt),
            _ptr(s2, dt), _ptr(lr, dt), _ptr(state, dt), p.numel())


# ---- training the standard DAE (csrc/conv_wgrad.hip) ----
def conv_wgrad_desc(x_shape, Cout, pad, Cin_tot=None, ci0=0, layout='oihw'):
    """The iiseg_conv_wgrad_desc of a zero-padded 3x3 layer on x (B,Cin,H,W) whose parameter array has Cin_tot
    input channels, this source's at [ci0, ci0 + Cin)."""
    B, Cin, H, W = (int(v) for v in x_shape)
    Cin_tot = Cin if Cin_tot is None else int(Cin_tot)
    d = _lib.ConvWgradDesc()
    d.B, d.Cin, d.Cout, d.H, d.W, d.K, d.pad = B, Cin, int(Cout), H, W, 3, int(pad)
    d.ci0, d.Cin_tot = int(ci0), Cin_tot
    d.so, d.sc = layout_strides(Cin_tot, int(Cout), 3, layout)
    return d


WGRAD_MODES = DGRAD_MODES = KXK_MODES = FWD_MODES = MODES_16BIT
WGRAD_CO_BLOCKS = (64, 16)      # output channels per workgroup of the weight-gradient kernels (16: mma='bf16' only)
# (mma, co_block) -> (workspace entry point, profile name, launch function or None: the dtype's iiseg_conv_wgrad_*);
# each form has a plan, and a profile name, of its own
_WGRAD_FORMS = {
    ('f32', 64): ('iiseg_conv_wgrad_workspace_elems', 'conv_wgrad_kernel', None),
    ('bf16', 64): ('iiseg_conv_wgrad_bf16_workspace_elems', 'conv_wgrad_bf16_kernel', 'iiseg_conv_wgrad_bf16'),
    ('bf16', 16): ('iiseg_conv_wgrad_bf16_co16_workspace_elems', 'conv_wgrad_bf16_co16_kernel',
                   'iiseg_conv_wgrad_bf16_co16'),
}


def conv_wgrad(x, gz, dW, db=None, pad=1, ci0=0, layout='oihw', mma='f32', co_block=64):
    """dW[:, ci0:ci0 + Cin] (and db, unless None) of the zero-padded 3x3 layer out = conv(xpad, W) + b, written
    in place into the layer's own parameter layout, from its input x (B,Cin,H,W) and gz = dL/dout (ReLU mask
    applied) (B,Cout,H + 2 pad - 2,W + 2 pad - 2).  The other input channels of dW are not touched (the second
    source of a concat layer is a second call).  float32: v_mfma_f32_32x32x2_f32; float64: vector ALU.
    mma='bf16' (float32 tensors only; csrc/conv_wgrad_bf16.hip): x and gz are rounded once to bf16 as they are
    staged and multiplied by v_mfma_f32_32x32x16_bf16 with fp32 accumulators; db stays the sum of the unrounded
    gz.  co_block=16 (with mma='bf16' only; the same source's co16 form): the same sums
    in blocks of 16 output x 64 input channels on v_mfma_f32_16x16x32_bf16, the form for layers with few output
    channels; the caller chooses, nothing here does."""
    dt = x.dtype
    if mma not in WGRAD_MODES:
        raise ValueError("conv_wgrad: mma=%r is not one of %s" % (mma, WGRAD_MODES))
    if co_block not in WGRAD_CO_BLOCKS:
        raise ValueError("conv_wgrad: co_block=%r is not one of %s" % (co_block, WGRAD_CO_BLOCKS))
    if co_block == 16 and mma != 'bf16':
        raise ValueError("conv_wgrad: co_block=16 is a form of mma='bf16' (got mma=%r)" % (mma,))
    if mma == 'bf16' and not (dt == gz.dtype == dW.dtype == torch.float32 and (db is None or db.dtype == dt)):
        raise ValueError("conv_wgrad: mma='bf16' takes float32 tensors only (x %s, gz %s, dW %s)"
                         % (x.dtype, gz.dtype, dW.dtype))
    if dW.dim() != 4 or tuple(dW.shape[2:]) != (3, 3):
        raise RuntimeError('conv_wgrad: dW %s is not a 3x3 parameter' % (tuple(dW.shape),))
    Cout, Cin_tot = (dW.shape[0], dW.shape[1]) if layout == 'oihw' else (dW.shape[1], dW.shape[0])
    B, Cin, H, W = x.shape
    OH, OW = H + 2 * pad - 2, W + 2 * pad - 2
    if tuple(gz.shape) != (B, Cout, OH, OW) or (db is not None and db.numel() != Cout):
        raise RuntimeError('conv_wgrad: shapes x %s gz %s dW %s' % (tuple(x.shape), tuple(gz.shape), tuple(dW.shape)))
    d = conv_wgrad_desc(tuple(x.shape), Cout, pad, Cin_tot, ci0, layout)
    ws_elems, kern, launch = _WGRAD_FORMS[mma, co_block]
    # (the fp32 / f64 entry points take the element size, and there is one launch function per dtype)
    n = _count(getattr(_lib.load(), ws_elems)(C.byref(d), *(() if launch else (dW.element_size(),))), ws_elems)
    fn = getattr(_lib.load(), launch) if launch else _fn('conv_wgrad', dt)
    ws = _workspace(_SUFFIX[dt], n, x.device) if n else None
    _launch(kern, 2.0 * Cin * Cout * 9 * B * OH * OW, fn, C.byref(d), _ptr(x, dt), _ptr(gz, dt),
            _ptr(ws, dt), _ptr(dW, dt), _ptr(db, dt))
    if CONV_PROFILE is not None:
        # byte model: x and g_z read once, the slabs written and read once
        _add_bytes(kern, float(dW.element_size()) * (x.numel() + gz.numel() + 2 * n))


def conv_wgrad_db(gz, db, Cin, pad=1):
    """db of ops.conv_wgrad(x, gz, dW, db, pad, mma='f32') alone -- the same bits, for any x of Cin channels (the
    kernel's plan, hence the order of its sums, depends on Cin) -- from gz (B,Cout,OH,OW), float32.  What a caller
    pairs with conv_wgrad(..., db=None, mma='bf16') to leave the bias gradient as the fp32 mode has it."""
    _need_f32('conv_wgrad_db', (('gz', gz), ('db', db)), required=('gz', 'db'))
    B, Cout, OH, OW = gz.shape
    if db.numel() != Cout or not gz.is_contiguous() or not db.is_contiguous():
        raise RuntimeError('conv_wgrad_db: gz %s db %s' % (tuple(gz.shape), tuple(db.shape)))
    d = conv_wgrad_desc((B, int(Cin), OH - 2 * pad + 2, OW - 2 * pad + 2), Cout, pad)
    n = _count(_lib.load().iiseg_conv_wgrad_db_workspace_elems(C.byref(d)), 'iiseg_conv_wgrad_db_workspace_elems')
    ws = _workspace('f32', n, gz.device) if n else None
    _launch('conv_wgrad_db_kernel', 0.0, _lib.load().iiseg_conv_wgrad_db_f32, C.byref(d), _ptr(gz, gz.dtype),
            _ptr(ws, gz.dtype), _ptr(db, gz.dtype))
    if CONV_PROFILE is not None:
        _add_bytes('conv_wgrad_db_kernel', 4.0 * (gz.numel() + 2 * n))


# ---- data gradients on the 16-bit matrix pipe (csrc/conv_dgrad_bf16.hip, conv_kxk_bf16.hip) ----
def _need_f32(what, named, required=()):
    """The `named` (name, argument) pairs of `what` must be float32 tensors; None is a left-out argument unless the
    name is `required`."""
    for name, t in named:
        if (t is not None or name in required) and (not torch.is_tensor(t) or t.dtype != torch.float32):
            raise ValueError('%s: %s must be a float32 tensor (got %s)'
                             % (what, name, t.dtype if torch.is_tensor(t) else type(t).__name__))


# The two data-gradient kernels, both on iiseg_conv_dgrad_desc.  name: the public function; k_ok, k_what: the K check
# and its wording; pad(K): the zero padding of the layer's forward as the descriptor names it -- gx is (H + 2 pad -
# K + 1) square-wise: g_z's own size at pad 1, OH + K - 1 for a 'valid' layer; gz_dims: how g_z is described; stem:
# the library symbols stem, stem_pack, stem_pack_elems (stem_workspace_elems) and, less 'iiseg_', the profile names
# stem_kernel and stem_pack_kernel; slabs: the reduction may be split (a workspace, and its term of the byte model).
_DgradKind = collections.namedtuple('_DgradKind', 'name k_ok k_what pad gz_dims stem slabs')
_DGRAD_3X3 = _DgradKind('conv_dgrad', lambda W: tuple(W.shape[2:]) == (3, 3), 'a 3x3 parameter', lambda K: 1,
                        '(B, Cout, H, W)', 'iiseg_conv_dgrad_bf16', False)
_DGRAD_KXK = _DgradKind('conv_dgrad_kxk', lambda W: W.shape[2] == W.shape[3] and 1 <= W.shape[2] <= 7,
                        'a K x K parameter, 1 <= K <= 7', lambda K: K - 1, '(B, Cout, OH, OW)',
                        'iiseg_conv_dgrad_kxk_bf16', True)


def _dgrad_desc(kind, gz_shape, Wshape, ci0, cin, layout, accumulate=False):
    B, Cout, H, W = (int(v) for v in gz_shape)
    Cin_tot, Co, K, so, sc = _param_strides(Wshape, layout)
    d = _lib.ConvDgradDesc()
    d.B, d.Cin, d.Cout, d.H, d.W, d.K, d.pad = B, Cin_tot - int(ci0) if cin is None else int(cin), Cout, H, W, K, kind.pad(K)
    d.ci0, d.Cin_tot, d.accumulate = int(ci0), Cin_tot, int(bool(accumulate))
    d.so, d.sc = so, sc
    return d


def _dgrad_args(kind, gz, W, layout, what):
    """What the data gradient and its pack refuse before the library is called."""
    _need_f32(what, (('gz', gz), ('W', W)))
    if layout not in ('oihw', 'iohw'):
        raise ValueError('%s: layout %r' % (what, layout))
    if W.dim() != 4 or not kind.k_ok(W):
        raise ValueError('%s: W %s is not %s' % (what, tuple(W.shape), kind.k_what))


def _dgrad_pack(kind, W, gz_shape, ci0, cin, layout, out):
    what = kind.name + '_pack'
    _dgrad_args(kind, None, W, layout, what)
    d = _dgrad_desc(kind, gz_shape, tuple(W.shape), ci0, cin, layout)
    n = _count(getattr(_lib.load(), kind.stem + '_pack_elems')(C.byref(d)), kind.stem + '_pack_elems')
    if out is None:
        out = torch.empty(n, dtype=torch.bfloat16, device=W.device)
    elif out.dtype != torch.bfloat16 or out.numel() != n:
        raise ValueError('%s: out holds %d %s elements, the image %d bfloat16' % (what, out.numel(), out.dtype, n))
    kern = kind.stem[6:] + '_pack_kernel'
    _launch(kern, 0.0, getattr(_lib.load(), kind.stem + '_pack'), C.byref(d), _ptr(W), _ptr(out, torch.bfloat16))
    if CONV_PROFILE is not None:
        _add_bytes(kern, 4.0 * d.Cout * d.Cin * d.K * d.K + 2.0 * n)
    return out


def _dgrad_run(kind, gz, W, ci0, cin, layout, out, accumulate, gate, packed):
    what = kind.name
    _dgrad_args(kind, gz, W, layout, what)
    _need_f32(what, (('out', out), ('gate', gate)))
    if packed is not None and (not torch.is_tensor(packed) or packed.dtype != torch.bfloat16):
        raise ValueError('%s: packed must be the bfloat16 tensor of %s_pack' % (what, what))
    if accumulate and out is None:
        raise ValueError('%s: accumulate=True needs the map to add to (out=)' % what)
    if gz.dim() != 4:
        raise ValueError('%s: gz %s is not %s' % (what, tuple(gz.shape), kind.gz_dims))
    d = _dgrad_desc(kind, tuple(gz.shape), tuple(W.shape), ci0, cin, layout, accumulate)
    Cout_w = W.shape[0] if layout == 'oihw' else W.shape[1]
    if gz.shape[1] != Cout_w or d.Cin < 1 or d.ci0 < 0 or d.ci0 + d.Cin > d.Cin_tot:
        raise ValueError('%s: gz %s, W %s (%s), input channels [%d, %d)'
                         % (what, tuple(gz.shape), tuple(W.shape), layout, d.ci0, d.ci0 + d.Cin))
    shape = (d.B, d.Cin, d.H + 2 * d.pad - d.K + 1, d.W + 2 * d.pad - d.K + 1)
    for name, t in (('out', out), ('gate', gate)):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError('%s: %s %s, the gradient is %s' % (what, name, tuple(t.shape), shape))
    lib = _lib.load()
    n = _count(getattr(lib, kind.stem + '_pack_elems')(C.byref(d)), kind.stem + '_pack_elems')
    if packed is None:
        packed = _dgrad_pack(kind, W, tuple(gz.shape), ci0, cin, layout, None)
    elif packed.numel() != n:
        raise ValueError('%s: packed holds %d elements, the image of this slice %d' % (what, packed.numel(), n))
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=gz.device)
    nws, ws = 0, ()
    if kind.slabs:
        nws = _count(getattr(lib, kind.stem + '_workspace_elems')(C.byref(d)), kind.stem + '_workspace_elems')
        ws = (_ptr(_workspace('f32', nws, gz.device) if nws else None),)
    kern = kind.stem[6:] + '_kernel'
    _launch(kern, 2.0 * d.Cin * d.Cout * d.K * d.K * d.B * d.H * d.W, getattr(lib, kind.stem), C.byref(d), _ptr(gz),
            _ptr(packed, torch.bfloat16), _ptr(gate), *ws, _ptr(out))
    if CONV_PROFILE is not None:
        # byte model: g_z and the image read once, the slabs written and read once, gx written once (read once more
        # when it is added to), the gate read
        _add_bytes(kern, 4.0 * gz.numel() + 2.0 * n + 8.0 * nws +
                   4.0 * out.numel() * (1 + int(bool(accumulate)) + (gate is not None)))
    return out


def conv_dgrad_desc(gz_shape, Wshape, ci0=0, cin=None, layout='oihw', accumulate=False):
    """The iiseg_conv_dgrad_desc of the pad-1 3x3 layer with parameter `Wshape` stored as `layout`, for g_z
    (B,Cout,H,W) and the input channels [ci0, ci0 + cin) (default: all from ci0 on)."""
    return _dgrad_desc(_DGRAD_3X3, gz_shape, Wshape, ci0, cin, layout, accumulate)


def conv_dgrad_pack(W, gz_shape, ci0=0, cin=None, layout='oihw', out=None):
    """The bf16 image of the input channels [ci0, ci0 + cin) of the fp32 3x3 parameter W (read in place: the flip
    and the transpose are indices) that conv_dgrad multiplies by; into `out` (a bfloat16 tensor of the size a
    previous call returned: the address stays) or a new tensor.  One small launch; again whenever W has changed."""
    return _dgrad_pack(_DGRAD_3X3, W, gz_shape, ci0, cin, layout, out)


def conv_dgrad(gz, W, ci0=0, cin=None, layout='oihw', out=None, accumulate=False, gate=None, packed=None):
    """The data gradient of the zero-padded 3x3 stride-1 pad-1 layer with fp32 parameter W, on the 16-bit matrix
    pipe (csrc/conv_dgrad_bf16.hip): gx[b,ci,y,x] = sum_{co,ky,kx} bf16(W[co,ci0+ci,ky,kx]) bf16(gz[b,co,y+1-ky,
    x+1-kx]), every operand rounded once (nearest, ties to even), fp32 accumulation in a fixed order by
    v_mfma_f32_32x32x16_bf16.  gz (B,Cout,H,W) = dL/dout with the ReLU mask applied.  ci0, cin: the slice of W's
    input channels whose gradient is formed (a concat layer's goes to the features only).  out: the destination
    (B,cin,H,W); accumulate=True adds to what it holds (it must be given).  gate: a map of gx's shape -- the result
    is gx * [gate > 0], relu'(0) = 0.  packed: what conv_dgrad_pack returned for this W, slice and layout (default:
    packed here, one more launch).  float32 tensors only."""
    return _dgrad_run(_DGRAD_3X3, gz, W, ci0, cin, layout, out, accumulate, gate, packed)


# ---- true-gradient refinement through the context-module DAE (csrc/ctx_grad.hip) ----
def _param_strides(Wshape, layout):
    """(Cin, Cout, K, so, sc) of a layer parameter in its own layout."""
    Cout, Cin = (int(Wshape[0]), int(Wshape[1])) if layout == 'oihw' else (int(Wshape[1]), int(Wshape[0]))
    K = int(Wshape[2])
    return (Cin, Cout, K) + layout_strides(Cin, Cout, K, layout)


def dgrad_desc(gout_shape, Wshape, dil, layout, out_place=None, window=None, ci=None, gx_place=None):
    """The iiseg_dgrad_desc of the masked data gradient of a 'valid' layer: gout (B,Cout,OH,OW); out_place =
    (out_H, out_W, y0, x0) of the planes the layer's output lives in; window = (y0, x0, h, w) of g_x; ci =
    (first, count) of the input channels; gx_place = (C, H, W, c0, y0, x0) of the destination (default: dense)."""
    B, Cout, OH, OW = (int(v) for v in gout_shape)
    Cin, Co, K, so, sc = _param_strides(Wshape, layout)
    if Co != Cout:
        raise RuntimeError('dgrad: gout has %d channels, the layer %d' % (Cout, Co))
    d = _lib.DgradDesc()
    d.B, d.Cin, d.Cout, d.K, d.dil, d.OH, d.OW = B, Cin, Cout, K, int(dil), OH, OW
    d.out_H, d.out_W, d.out_y0, d.out_x0 = (OH, OW, 0, 0) if out_place is None else tuple(int(v) for v in out_place)
    span = int(dil) * (K - 1)
    d.wy0, d.wx0, d.WH, d.WW = (0, 0, OH + span, OW + span) if window is None else tuple(int(v) for v in window)
    d.ci0, d.nci = (0, Cin) if ci is None else (int(ci[0]), int(ci[1]))
    d.gx_C, d.gx_H, d.gx_W, d.gx_c0, d.gx_y0, d.gx_x0 = (d.nci, d.WH, d.WW, 0, 0, 0) if gx_place is None else \
        tuple(int(v) for v in gx_place)
    d.so, d.sc = so, sc
    return d


def conv_small_dgrad(gout, out, W, dil=1, layout='iohw', out_off=(0, 0), window=None, ci=None, gx=None,
                     gx_off=(0, 0, 0)):
    """g_x of the 'valid' layer with parameter W (its own `layout`) from gout = dL/d(layer output) and the
    layer's rectified output `out` (None: a linear layer): g_z = gout [out > 0] is formed while gout is read.
    `out` may be a larger tensor holding the (OH, OW) map at `out_off`.  Only `window` = (y0, x0, h, w) of g_x
    and the input channels `ci` = (first, count) are computed; they go to a new dense tensor, or into `gx` at
    gx_off = (c0, y0, x0) (the rest of `gx` is not touched).  Returns the tensor written."""
    dt = gout.dtype
    B, Cout, OH, OW = gout.shape
    out_place = None
    if out is not None:
        if out.dim() != 4 or out.shape[0] != B or out.shape[1] != Cout:
            raise RuntimeError('dgrad: out %s for gout %s' % (tuple(out.shape), tuple(gout.shape)))
        out_place = (out.shape[2], out.shape[3], out_off[0], out_off[1])
    d = dgrad_desc(tuple(gout.shape), tuple(W.shape), dil, layout, out_place, window, ci)
    if gx is None:
        gx = torch.empty((B, d.nci, d.WH, d.WW), dtype=dt, device=gout.device)
    else:
        if gx.dim() != 4 or gx.shape[0] != B:
            raise RuntimeError('dgrad: gx %s' % (tuple(gx.shape),))
        d.gx_C, d.gx_H, d.gx_W = gx.shape[1], gx.shape[2], gx.shape[3]
        d.gx_c0, d.gx_y0, d.gx_x0 = (int(v) for v in gx_off)
    _count(_lib.load().iiseg_conv_small_dgrad_blocks(C.byref(d)), 'iiseg_conv_small_dgrad_blocks')
    kern = 'conv_small_dgrad_kernel'
    _launch(kern, 2.0 * d.nci * Cout * d.K * d.K * B * d.WH * d.WW, _fn('conv_small_dgrad', dt), C.byref(d),
            _ptr(gout, dt), _ptr(out, dt), _ptr(W, dt), _ptr(gx, dt))
    if CONV_PROFILE is not None:
        # byte model: g_out (and out) read once, the window of g_x written
        _add_bytes(kern, float(gout.element_size()) * B *
                   ((2 if out is not None else 1) * Cout * OH * OW + d.nci * d.WH * d.WW))
    return gx


def ctx_grad_head(score, y, out6, W7, layout='iohw', want_gs=False):
    """(score, y, out6) -> the masked gradient at dilconv6's output in one launch: r = softmax(score), g_s =
    dE/dscore of E = sum (r - y)^2 (the bits of `sqerr_softmax_bwd`), g6 = [out6 > 0] W7^T g_s.  Returns g6, or
    (g6, g_s) with want_gs."""
    dt = y.dtype
    B, Cc, H, W = y.shape
    Cin, Cout, K, so, sc = _param_strides(tuple(W7.shape), layout)
    if K != 1 or Cout != Cc or tuple(score.shape) != tuple(y.shape) or \
            (out6 is not None and tuple(out6.shape) != (B, Cin, H, W)):
        raise RuntimeError('ctx_grad_head: score %s y %s out6 %s W7 %s' % (
            tuple(score.shape), tuple(y.shape), None if out6 is None else tuple(out6.shape), tuple(W7.shape)))
    g6 = torch.empty((B, Cin, H, W), dtype=dt, device=y.device)
    gs = torch.empty_like(y) if want_gs else None
    kern = 'ctx_grad_head_kernel'
    _launch(kern, 2.0 * Cin * Cc * B * H * W, _fn('ctx_grad_head', dt), _ptr(score, dt), _ptr(y, dt), _ptr(out6, dt),
            _ptr(W7, dt), so, sc, _ptr(gs, dt), _ptr(g6, dt), B, Cc, Cin, H, W)
    if CONV_PROFILE is not None:
        _add_bytes(kern, float(y.element_size()) * B * H * W *
                   ((3 if want_gs else 2) * Cc + (2 if out6 is not None else 1) * Cin))
    return (g6, gs) if want_gs else g6


# ---- training FCN-8 (csrc/conv_wgrad_kxk.hip, deconv_grad.hip, fcn8_train.hip) ----
def conv_wgrad_kxk_desc(x, Cout, K, window=None, Cin_tot=None, ci0=0, layout='oihw'):
    """The iiseg_conv_wgrad_kxk_desc of a 'valid' K x K layer on `window` = (y0, x0, h, w) of the planes of x
    (B,Cin,H,W; any strides with unit column stride), default the whole map; x may also be a shape (dense)."""
    if isinstance(x, torch.Tensor):
        B, Cin, H, W = (int(v) for v in x.shape)
        si, sp, sr, s1 = (int(v) for v in x.stride())
        if s1 != 1:
            raise RuntimeError('conv_wgrad_kxk: x needs unit column stride (strides %s)' % (x.stride(),))
    else:
        B, Cin, H, W = (int(v) for v in x)
        si, sp, sr = Cin * H * W, H * W, W
    y0, x0, h, w = (0, 0, H, W) if window is None else (int(v) for v in window)
    if y0 < 0 or x0 < 0 or y0 + h > H or x0 + w > W:
        raise RuntimeError('conv_wgrad_kxk: window %s outside the %d x %d map' % ((y0, x0, h, w), H, W))
    Cin_tot = Cin if Cin_tot is None else int(Cin_tot)
    d = _lib.ConvWgradKxKDesc()
    d.B, d.Cin, d.Cout, d.H, d.W, d.K = B, Cin, int(Cout), h, w, int(K)
    d.ci0, d.Cin_tot, d.x_y0, d.x_x0 = int(ci0), Cin_tot, y0, x0
    d.x_row, d.x_plane, d.x_image = sr, sp, si
    d.so, d.sc = layout_strides(Cin_tot, int(Cout), int(K), layout)
    return d


def conv_wgrad_kxk(x, gz, dW, db=None, window=None, ci0=0, layout='oihw', mma='f32'):
    """dW[:, ci0:ci0 + Cin] (and db, unless None) of the 'valid' K x K stride-1 layer (1 <= K <= 7) out = conv(x,
    W) + b, written in place into the layer's own parameter layout, from the `window` = (y0, x0, h, w) of its
    input's planes x (B,Cin,H,W), read in place, and gz = dL/dout (ReLU mask applied) (B,Cout,h - K + 1,w - K + 1).
    The other input channels of dW are not touched.  float32: v_mfma_f32_32x32x2_f32; float64: vector ALU.
    mma='bf16' (float32 device tensors only; csrc/conv_kxk_bf16.hip): x and gz are rounded
    once to bf16 as they are staged and multiplied by v_mfma_f32_32x32x16_bf16 with fp32 accumulators; db stays the
    sum of the unrounded gz."""
    dt = x.dtype
    if mma not in KXK_MODES:
        raise ValueError("conv_wgrad_kxk: mma=%r is not one of %s" % (mma, KXK_MODES))
    # one pass over the arguments: what mma='bf16' refuses is a ValueError, the float modes' refusals RuntimeError
    bf16 = mma == 'bf16'
    err = ValueError if bf16 else RuntimeError
    if bf16:
        _need_f32("conv_wgrad_kxk: mma='bf16'", (('x', x), ('gz', gz), ('dW', dW), ('db', db)))
        if layout not in ('oihw', 'iohw'):
            raise ValueError('conv_wgrad_kxk: layout %r' % (layout,))
    if dW.dim() != 4 or dW.shape[2] != dW.shape[3] or (bf16 and not 1 <= dW.shape[2] <= 7):
        raise err('conv_wgrad_kxk: dW %s is not a K x K parameter%s' % (tuple(dW.shape), ', 1 <= K <= 7' * bf16))
    if bf16 and (x.dim() != 4 or gz.dim() != 4):
        raise ValueError('conv_wgrad_kxk: x %s, gz %s' % (tuple(x.shape), tuple(gz.shape)))
    K = int(dW.shape[2])
    Cout, Cin_tot = (dW.shape[0], dW.shape[1]) if layout == 'oihw' else (dW.shape[1], dW.shape[0])
    h, w = (x.shape[2], x.shape[3]) if window is None else (int(window[2]), int(window[3]))
    OH, OW = h - K + 1, w - K + 1
    if tuple(gz.shape) != (x.shape[0], Cout, OH, OW) or (db is not None and db.numel() != Cout) or \
            (bf16 and (h < K or w < K or ci0 < 0 or ci0 + x.shape[1] > Cin_tot)):
        raise err('conv_wgrad_kxk: shapes x %s window %s gz %s dW %s (%s) ci0 %d' % (
            tuple(x.shape), window, tuple(gz.shape), tuple(dW.shape), layout, ci0))
    if not x.is_cuda or gz.dtype != dt or dW.dtype != dt or (bf16 and not (gz.is_cuda and dW.is_cuda)):
        raise err('conv_wgrad_kxk needs device tensors of one dtype')
    d = conv_wgrad_kxk_desc(x, Cout, K, window, Cin_tot, ci0, layout)   # (refuses a window outside x)
    if bf16:                                             # a plan, and a profile name, of its own
        n = _count(_lib.load().iiseg_conv_wgrad_kxk_bf16_workspace_elems(C.byref(d)),
                   'iiseg_conv_wgrad_kxk_bf16_workspace_elems')
        kern, fn = 'conv_wgrad_kxk_bf16_kernel', _lib.load().iiseg_conv_wgrad_kxk_bf16
    else:
        n = _count(_lib.load().iiseg_conv_wgrad_kxk_workspace_elems(C.byref(d), dW.element_size()),
                   'iiseg_conv_wgrad_kxk_workspace_elems')
        kern, fn = 'conv_wgrad_kxk_kernel', _fn('conv_wgrad_kxk', dt)
    ws = _workspace(_SUFFIX[dt], n, x.device) if n else None
    _launch(kern, 2.0 * d.Cin * Cout * K * K * d.B * OH * OW, fn, C.byref(d),
            C.c_void_p(x.data_ptr()), _ptr(gz, dt), _ptr(ws, dt), _ptr(dW, dt), _ptr(db, dt))
    if CONV_PROFILE is not None:
        # byte model: the window of x and g_z read once, the slabs written and read once
        _add_bytes(kern, float(dW.element_size()) * (d.B * d.Cin * d.H * d.W + gz.numel() + 2 * n))


def conv_dgrad_kxk_desc(gz_shape, Wshape, ci0=0, cin=None, layout='oihw', accumulate=False):
    """The iiseg_conv_dgrad_desc of the 'valid' K x K layer with parameter `Wshape` stored as `layout`, for g_z
    (B,Cout,OH,OW) and the input channels [ci0, ci0 + cin) (default: all from ci0 on)."""
    return _dgrad_desc(_DGRAD_KXK, gz_shape, Wshape, ci0, cin, layout, accumulate)


def conv_dgrad_kxk_pack(W, gz_shape, ci0=0, cin=None, layout='oihw', out=None):
    """The bf16 image of the input channels [ci0, ci0 + cin) of the fp32 K x K parameter W (read in place: the flip
    and the transpose are indices) that conv_dgrad_kxk multiplies by; into `out` (a bfloat16 tensor of the size a
    previous call returned: the address stays) or a new tensor.  One launch; again whenever W has changed."""
    return _dgrad_pack(_DGRAD_KXK, W, gz_shape, ci0, cin, layout, out)


def conv_dgrad_kxk(gz, W, ci0=0, cin=None, layout='oihw', out=None, accumulate=False, gate=None, packed=None):
    """The data gradient of the 'valid' K x K stride-1 layer (1 <= K <= 7) with fp32 parameter W, on the 16-bit
    matrix pipe (csrc/conv_kxk_bf16.hip): gx[b,ci,y,x] = sum_{co,ky,kx} bf16(W[co,ci0+ci,ky,
    kx]) bf16(gz[b,co,y-ky,x-kx]), gz (B,Cout,OH,OW) zero outside its plane (no embedded copy), gx (B,cin,OH+K-1,
    OW+K-1); every operand rounded once (nearest, ties to even), fp32 accumulation in a fixed order by
    v_mfma_f32_32x32x16_bf16, the slabs of output channels added in slab order.  ci0, cin, out, accumulate, gate:
    as conv_dgrad.  packed: what conv_dgrad_kxk_pack returned for this W, slice and layout (default: packed here,
    one more launch).  float32 tensors only."""
    return _dgrad_run(_DGRAD_KXK, gz, W, ci0, cin, layout, out, accumulate, gate, packed)


def conv_fwd_kxk_desc(x_shape, Wshape, relu=True):
    """The iiseg_conv_fwd_kxk_desc of the 'valid' K x K stride-1 layer with 'oihw' parameter `Wshape` on an x of
    `x_shape` = (B,Cin,H,W)."""
    d = _lib.ConvFwdKxKDesc()
    d.B, d.Cin, d.H, d.W = (int(v) for v in x_shape)
    d.Cout, d.K, d.relu = int(Wshape[0]), int(Wshape[2]), int(bool(relu))
    return d


def conv_fwd_kxk(x, W, b=None, relu=True, out=None):
    """The forward of the 'valid' K x K stride-1 layer (1 <= K <= 7) with fp32 'oihw' parameter W (read as it is: no
    im2col image, no packed copy) and bias b (or None), on the 16-bit matrix pipe (csrc/conv_kxk_bf16.hip, DESIGN.md
    section 18): z[b,co,y,x] = relu(sum_{ci,ky,kx} bf16(W[co,ci,ky,kx]) bf16(x[b,ci,y+ky,x+kx]) + b[co]), every
    operand rounded once (nearest, ties to even) as it is staged, fp32 accumulation in a fixed order by
    v_mfma_f32_32x32x16_bf16, the slabs of a split reduction added in slab order, the bias added in fp32.  Into
    `out` (B,Cout,H-K+1,W-K+1) or a new tensor.  float32 contiguous device tensors only."""
    _need_f32('conv_fwd_kxk', (('x', x), ('W', W), ('b', b), ('out', out)), required=('x', 'W'))
    if W.dim() != 4 or W.shape[2] != W.shape[3] or not 1 <= W.shape[2] <= 7:
        raise ValueError('conv_fwd_kxk: W %s is not a K x K parameter, 1 <= K <= 7' % (tuple(W.shape),))
    K = int(W.shape[2])
    if x.dim() != 4 or x.shape[1] != W.shape[1] or x.shape[2] < K or x.shape[3] < K or x.shape[0] < 1:
        raise ValueError("conv_fwd_kxk: x %s, W %s ('oihw')" % (tuple(x.shape), tuple(W.shape)))
    if b is not None and tuple(b.shape) != (W.shape[0],):
        raise ValueError('conv_fwd_kxk: b %s for %d output channels' % (tuple(b.shape), W.shape[0]))
    shape = (x.shape[0], W.shape[0], x.shape[2] - K + 1, x.shape[3] - K + 1)
    if out is not None and tuple(out.shape) != shape:
        raise ValueError('conv_fwd_kxk: out %s, the map is %s' % (tuple(out.shape), shape))
    for name, t in (('x', x), ('W', W), ('b', b), ('out', out)):
        if t is not None and not t.is_cuda:
            raise ValueError('conv_fwd_kxk: %s must be a device tensor (got %s)' % (name, t.device))
        if t is not None and not t.is_contiguous():
            raise ValueError('conv_fwd_kxk: %s must be contiguous' % name)
    d = conv_fwd_kxk_desc(tuple(x.shape), tuple(W.shape), relu)
    lib = _lib.load()
    nws = _count(lib.iiseg_conv_fwd_kxk_bf16_workspace_elems(C.byref(d)), 'iiseg_conv_fwd_kxk_bf16_workspace_elems')
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    ws = _workspace('f32', nws, x.device) if nws else None
    kern = 'conv_fwd_kxk_bf16_kernel'
    _launch(kern, 2.0 * d.Cin * d.Cout * K * K * out.shape[0] * out.shape[2] * out.shape[3],
            lib.iiseg_conv_fwd_kxk_bf16, C.byref(d), _ptr(x), _ptr(W), _ptr(b), _ptr(ws), _ptr(out))
    if CONV_PROFILE is not None:
        # byte model: x and the parameter read once, the slabs written and read once, z written once
        _add_bytes(kern, 4.0 * (x.numel() + W.numel() + 2 * nws + out.numel()))
    return out


def bnrelu_conv_desc(stack_shape, n, Cout, out_cap=None, out_c0=0):
    """The iiseg_bnrelu_conv_desc of a dense-block layer with `Cout` filters on the first `n` channels of a stack of
    `stack_shape` = (B,cap,H,W), written at channel `out_c0` of a tensor with `out_cap` channels (default: a dense
    (B,Cout,H,W) one)."""
    d = _lib.BnReluConvDesc()
    d.B, d.cap, d.H, d.W = (int(v) for v in stack_shape)
    d.n, d.Cout, d.out_c0 = int(n), int(Cout), int(out_c0)
    d.out_cap = int(Cout) if out_cap is None else int(out_cap)
    return d


def bnrelu_conv_fwd(stack, n, bn, W, b, out=None, out_c0=0, keep=None, p=0.0):
    """The training forward of a dense-block layer of FC-DenseNet as ONE launch on the 16-bit matrix pipe
    (csrc/bnrelu_conv_bf16.hip): t = relu(BatchNorm(stack[:, :n])) with bn = (beta, gamma,
    mean, inv_std) -- `bn_relu`'s expression, the padding ring zeros of t --, the zero-padded 3x3 layer with the fp32
    'oihw' parameter W (Cout,n,3,3), read as it is, and bias b, then `dropout_apply`'s expression with the 0/1 mask
    `keep` (B,Cout,H,W) and p (keep=None: no factor): z = (sum bf16(W) bf16(t) + b) * keep / (1 - p).  W and t are
    rounded once (nearest, ties to even) as they are staged, v_mfma_f32_16x16x32_bf16 accumulates in fp32 in a fixed
    order, the slabs of a split reduction are added in slab order before bias, mask and scale.  Into channels
    [out_c0, out_c0 + Cout) of `out` (B,out_cap,H,W) -- which may be `stack` itself with out_c0 >= n -- and nothing
    else of it; out=None: a new dense (B,Cout,H,W) tensor.  float32 contiguous device tensors only."""
    what = 'bnrelu_conv_fwd'
    if not isinstance(bn, (tuple, list)) or len(bn) != 4:
        raise ValueError('%s: bn must be (beta, gamma, mean, inv_std)' % what)
    beta, gamma, mean, inv_std = bn
    named = (('stack', stack), ('beta', beta), ('gamma', gamma), ('mean', mean), ('inv_std', inv_std), ('W', W),
             ('b', b), ('out', out), ('keep', keep))
    _need_f32(what, named, required=('stack', 'beta', 'gamma', 'mean', 'inv_std', 'W', 'b'))
    n, out_c0 = int(n), int(out_c0)
    if stack.dim() != 4 or min(stack.shape) < 1 or not 1 <= n <= stack.shape[1]:
        raise ValueError('%s: the first %d channels of a stack %s' % (what, n, tuple(stack.shape)))
    B, cap, H, Wd = (int(v) for v in stack.shape)
    if W.dim() != 4 or tuple(W.shape[1:]) != (n, 3, 3) or W.shape[0] < 1:
        raise ValueError("%s: W %s is not a 3x3 'oihw' parameter on %d channels" % (what, tuple(W.shape), n))
    Cout = int(W.shape[0])
    if tuple(b.shape) != (Cout,):
        raise ValueError('%s: b %s for %d output channels' % (what, tuple(b.shape), Cout))
    for name, v in (('beta', beta), ('gamma', gamma), ('mean', mean), ('inv_std', inv_std)):
        if v.dim() != 1 or v.numel() < n:
            raise ValueError('%s: %s %s for %d channels' % (what, name, tuple(v.shape), n))
    if out is None:
        if out_c0 != 0:
            raise ValueError('%s: out_c0 = %d without `out`' % (what, out_c0))
    else:
        if out.dim() != 4 or (out.shape[0], out.shape[2], out.shape[3]) != (B, H, Wd) or out_c0 < 0 or \
                out_c0 + Cout > out.shape[1]:
            raise ValueError('%s: channels [%d, %d) of out %s, the map is %s' % (what, out_c0, out_c0 + Cout,
                                                                               tuple(out.shape), (B, Cout, H, Wd)))
        if out.data_ptr() == stack.data_ptr() and (out.shape[1] != cap or out_c0 < n):
            raise ValueError('%s: out is the stack and out_c0 = %d < n = %d: the channels read and written would '
                             'overlap' % (what, out_c0, n))
    if keep is not None and tuple(keep.shape) != (B, Cout, H, Wd):
        raise ValueError('%s: keep %s, the map is %s' % (what, tuple(keep.shape), (B, Cout, H, Wd)))
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError('%s: p = %r is not in [0, 1)' % (what, p))
    for name, t in named:
        if t is not None and not t.is_contiguous():
            raise ValueError('%s: %s must be contiguous' % (what, name))
    for name, t in named:
        if t is not None and not t.is_cuda:
            raise ValueError('%s: %s must be a device tensor (got %s)' % (what, name, t.device))
    d = bnrelu_conv_desc((B, cap, H, Wd), n, Cout, None if out is None else out.shape[1], out_c0)
    lib = _lib.load()
    nws = _count(lib.iiseg_bnrelu_conv_fwd_bf16_workspace_elems(C.byref(d)),
                 'iiseg_bnrelu_conv_fwd_bf16_workspace_elems')
    if out is None:
        out = torch.empty((B, Cout, H, Wd), dtype=torch.float32, device=stack.device)
    ws = _workspace('f32', nws, stack.device) if nws else None
    kern = 'bnrelu_conv_bf16_kernel'
    _launch(kern, 2.0 * n * Cout * 9 * B * H * Wd, lib.iiseg_bnrelu_conv_fwd_bf16, C.byref(d), _ptr(stack),
            _ptr(beta), _ptr(gamma), _ptr(mean), _ptr(inv_std), _ptr(W), _ptr(b), _ptr(keep), p, _ptr(ws), _ptr(out))
    if CONV_PROFILE is not None:
        _add_bytes(kern, bnrelu_conv_bytes(B, n, Cout, H, Wd, keep is not None) + 8.0 * nws)
    return out


def bnrelu_conv_bytes(B, n, Cout, H, W, keep):
    """The byte model of one `bnrelu_conv_fwd` launch without a split: the n stack planes read once, the Cout planes
    written once (the mask's read once), the parameter read once."""
    return 4.0 * (B * H * W * (n + Cout * (2 if keep else 1)) + Cout * n * 9)


def deconv_desc(x_shape, Cout, K, stride, window=None):
    """The iiseg_deconv_desc of a transposed convolution on x (B,Cin,H,W); window = (oy0, ox0, OH, OW) of its
    full output, default all of it."""
    B, Cin, H, W = (int(v) for v in x_shape)
    d = _lib.DeconvDesc()
    d.B, d.Cin, d.H, d.W, d.Cout, d.K, d.stride = B, Cin, H, W, int(Cout), int(K), int(stride)
    full = ((H - 1) * int(stride) + int(K), (W - 1) * int(stride) + int(K))
    d.oy0, d.ox0, d.OH, d.OW = (0, 0) + full if window is None else tuple(int(v) for v in window)
    return d


DECONV_MODES = MODES_16BIT


def _deconv_bf16_kind(what, K, stride, mma):
    """The 16-bit transposed-convolution gradients are the K = 3, stride-2 layer's (refused before the library)."""
    if int(K) != 3 or int(stride) != 2:
        raise ValueError("%s: mma=%r is the K = 3, stride-2 layer's (got K = %d, stride %d)" % (what, mma, K, stride))


def _deconv_bf16_tensors(what, named, mma):
    """... and take contiguous device tensors (the last check before the library is touched)."""
    for name, t in named:
        if t is not None and not t.is_contiguous():
            raise ValueError("%s: mma=%r takes contiguous tensors (%s)" % (what, mma, name))
        if t is not None and not t.is_cuda:
            raise ValueError("%s: mma=%r takes device tensors (%s is on %s)" % (what, mma, name, t.device))


def _deconv3_products(d):
    """The products x . gf of a K = 3 stride-2 layer whose gf element lies in the window, per channel pair."""
    rows = sum(1 for i in range(d.H) for a in range(3) if d.oy0 <= 2 * i + a < d.oy0 + d.OH)
    cols = sum(1 for j in range(d.W) for c in range(3) if d.ox0 <= 2 * j + c < d.ox0 + d.OW)
    return float(d.B) * rows * cols


def deconv_dgrad(g, W, stride, x_hw, window=None, mma='f32'):
    """g_x (B,Cin,H,W) of the transposed convolution ops.Deconv(W[in,out,k,k], stride) on an input of x_hw = (H,
    W), from g = dL/d(`window` of its full output) (B,Cout,OH,OW); outside the window the gradient is zero.
    mma='bf16' (float32 device tensors, K = 3 and stride 2 only; csrc/deconv_grad_bf16.hip):
    g and W -- the layer's own fp32 parameter -- are rounded once to bf16 as they are staged and multiplied by
    v_mfma_f32_16x16x32_bf16 with fp32 accumulators in a fixed order."""
    if mma not in DECONV_MODES:
        raise ValueError("deconv_dgrad: mma=%r is not one of %s" % (mma, DECONV_MODES))
    dt = g.dtype if torch.is_tensor(g) else None
    if mma == 'bf16':
        _need_f32('deconv_dgrad', (('g', g), ('W', W)), required=('g', 'W'))
        if g.dim() != 4 or W.dim() != 4 or W.shape[2] != W.shape[3] or g.shape[1] != W.shape[1]:
            raise ValueError('deconv_dgrad: g %s W %s' % (tuple(g.shape), tuple(W.shape)))
        _deconv_bf16_kind('deconv_dgrad', W.shape[2], stride, mma)
    Cin, Cout, K = int(W.shape[0]), int(W.shape[1]), int(W.shape[2])
    d = deconv_desc((g.shape[0], Cin, x_hw[0], x_hw[1]), Cout, K, stride, window)
    if tuple(g.shape) != (d.B, Cout, d.OH, d.OW) or W.shape[2] != W.shape[3]:
        if mma == 'bf16':
            raise ValueError('deconv_dgrad: g %s W %s window %s' % (tuple(g.shape), tuple(W.shape), window))
        raise RuntimeError('deconv_dgrad: g %s W %s window %s' % (tuple(g.shape), tuple(W.shape), window))
    if mma == 'bf16':
        _deconv_bf16_tensors('deconv_dgrad', (('g', g), ('W', W)), mma)
    gx = torch.empty((d.B, Cin, d.H, d.W), dtype=dt, device=g.device)
    if mma == 'bf16':
        lib = _lib.load()
        n = _count(lib.iiseg_deconv_dgrad_bf16_workspace_elems(C.byref(d)), 'iiseg_deconv_dgrad_bf16_workspace_elems')
        ws = _workspace('f32', n, g.device) if n else None
        kern = 'deconv_dgrad_bf16_kernel'
        _launch(kern, 2.0 * Cin * Cout * _deconv3_products(d), lib.iiseg_deconv_dgrad_bf16, C.byref(d), _ptr(g),
                _ptr(W), _ptr(ws), _ptr(gx))
        if CONV_PROFILE is not None:
            # byte model: g and the parameter read once, the slabs written and read once, gx written once
            _add_bytes(kern, 4.0 * (g.numel() + W.numel() + 2 * n + gx.numel()))
        return gx
    kern = 'deconv_dgrad_kernel'
    _launch(kern, 2.0 * Cin * Cout * (K // int(stride)) ** 2 * g.shape[0] * d.OH * d.OW, _fn('deconv_dgrad', dt),
            C.byref(d), _ptr(g, dt), _ptr(W, dt), _ptr(gx, dt))
    if CONV_PROFILE is not None:
        _add_bytes(kern, float(g.element_size()) * (g.numel() + gx.numel()))
    return gx


def deconv_wgrad(x, g, dW, db, stride, window=None, mma='f32'):
    """dW (Cin,Cout,K,K) and db (Cout, or None) of the transposed convolution on x (B,Cin,H,W), written in place,
    from g = dL/d(`window` of its full output).
    mma='bf16' (float32 device tensors, K = 3 and stride 2 only; csrc/deconv_grad_bf16.hip):
    x and g are rounded once to bf16 as they are staged, v_mfma_f32_16x16x32_bf16, fp32 accumulation, slabs added in
    slab order; db is that kernel's own deterministic sum of the unrounded g -- not the bits of the 'f32' mode."""
    if mma not in DECONV_MODES:
        raise ValueError("deconv_wgrad: mma=%r is not one of %s" % (mma, DECONV_MODES))
    dt = x.dtype if torch.is_tensor(x) else None
    if mma == 'bf16':
        named = (('x', x), ('g', g), ('dW', dW), ('db', db))
        _need_f32('deconv_wgrad', named, required=('x', 'g', 'dW'))
        if x.dim() != 4 or g.dim() != 4 or dW.dim() != 4 or dW.shape[2] != dW.shape[3]:
            raise ValueError('deconv_wgrad: x %s g %s dW %s' % (tuple(x.shape), tuple(g.shape), tuple(dW.shape)))
        _deconv_bf16_kind('deconv_wgrad', dW.shape[2], stride, mma)
    Cin, Cout, K = int(dW.shape[0]), int(dW.shape[1]), int(dW.shape[2])
    d = deconv_desc(tuple(x.shape), Cout, K, stride, window)
    if x.shape[1] != Cin or tuple(g.shape) != (d.B, Cout, d.OH, d.OW) or dW.shape[2] != dW.shape[3] or \
            (db is not None and db.numel() != Cout):
        what = 'deconv_wgrad: x %s g %s dW %s window %s' % (tuple(x.shape), tuple(g.shape), tuple(dW.shape), window)
        if mma == 'bf16':
            raise ValueError(what)
        raise RuntimeError(what)
    if mma == 'bf16':
        _deconv_bf16_tensors('deconv_wgrad', named, mma)
        lib = _lib.load()
        n = _count(lib.iiseg_deconv_wgrad_bf16_workspace_elems(C.byref(d)), 'iiseg_deconv_wgrad_bf16_workspace_elems')
        ws = _workspace('f32', n, x.device) if n else None
        kern = 'deconv_wgrad_bf16_kernel'
        _launch(kern, 2.0 * Cin * Cout * _deconv3_products(d), lib.iiseg_deconv_wgrad_bf16, C.byref(d), _ptr(x),
                _ptr(g), _ptr(ws), _ptr(dW), _ptr(db))
        if CONV_PROFILE is not None:
            # byte model: x and g read once, the slabs written and read once
            _add_bytes(kern, 4.0 * (x.numel() + g.numel() + 2 * n))
        return
    nslab = _count(_lib.load().iiseg_deconv_wgrad_partials(C.byref(d)), 'iiseg_deconv_wgrad_partials')
    ws = _workspace(_SUFFIX[dt], nslab * (dW.numel() + Cout), x.device)
    kern = 'deconv_wgrad_kernel'
    _launch(kern, 2.0 * Cin * Cout * (K // int(stride)) ** 2 * x.shape[0] * d.OH * d.OW, _fn('deconv_wgrad', dt),
            C.byref(d), _ptr(x, dt), _ptr(g, dt), _ptr(ws, dt), _ptr(dW, dt), _ptr(db, dt))
    if CONV_PROFILE is not None:
        _add_bytes(kern, float(g.element_size()) * (g.numel() + x.numel() + 2 * ws.numel()))


def relu_gate(g, out, dst=None):
    """g * [out > 0] (relu'(0) = 0) for maps of one shape; into `dst` (default a new tensor; may be g itself)."""
    dt = g.dtype
    if g.shape != out.shape or (dst is not None and dst.shape != g.shape):
        raise RuntimeError('relu_gate: g %s out %s' % (tuple(g.shape), tuple(out.shape)))
    if dst is None:
        dst = torch.empty_like(g)
    kern = 'relu_gate_kernel'
    _launch(kern, 0.0, _fn('relu_gate', dt), _ptr(g, dt), _ptr(out, dt), _ptr(dst, dt), g.numel())
    if CONV_PROFILE is not None:
        _add_bytes(kern, float(g.element_size()) * 3 * g.numel())
    return dst


def l2_term(flat, gflat, ranges, weight_decay, penalty=None):
    """lasagne's regularize_network_params(l2) over the weight ranges [(lo, hi), ...] (ascending, disjoint) of the
    flat parameter buffer: gflat += 2 weight_decay flat there, and penalty (one double on the device, returned) =
    sum flat^2 in a fixed order.  Elements outside the ranges (the biases) are not touched."""
    dt = flat.dtype
    if flat.numel() != gflat.numel():
        raise RuntimeError('l2_term: buffers of different sizes')
    nr = len(ranges)
    npart = _count(_lib.load().iiseg_l2_term_partials(nr), 'iiseg_l2_term_partials')
    table = (C.c_int64 * (2 * nr))(*[int(v) for r in ranges for v in r])
    partial = _workspace('bn', npart, flat.device)
    if penalty is None:
        penalty = torch.empty(1, dtype=torch.float64, device=flat.device)
    kern = 'l2_term_kernel'
    _launch(kern, 0.0, _fn('l2_term', dt), _ptr(flat, dt), _ptr(gflat, dt), flat.numel(), table, nr,
            float(weight_decay), _ptr(partial, torch.float64), _ptr(penalty, torch.float64))
    if CONV_PROFILE is not None:
        _add_bytes(kern, float(flat.element_size()) * 3 * sum(hi - lo for lo, hi in ranges))
    return penalty
