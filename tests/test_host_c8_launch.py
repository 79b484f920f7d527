"""CPU: every argument of every bf16 C8 launch of ops.Conv (and Conv1x1C8's shared `in_c` rule), no GPU.

The library is built and loaded on the host; `ops._launch`, `ops._operand`, `ops._ptr`, `ops._workspace` and
`Conv._c8_weights` are replaced with recorders (and `ops.CONV_PROFILE` / `CONV_PROFILE_INFO` set, so the
profile record is seen too); the layers live on the CPU and are called through `Conv.__call__` on `meta`
tensors: nothing is computed, only Conv's public call is used.  A valid call walks through every check and
reaches the recorder with the kernel label, the flops, the entry point, the ConvDesc and every scalar; the
16-channel kernel's workspace size comes from the real iiseg_conv_c8_m16_workspace_bytes; an invalid call
raises its RuntimeError before any pointer is taken.

EXPECTED was recorded by this very file from the commit BEFORE the C8 launches were split into describe /
choose / run (845b08b), where it passes as written.  A row is five strings:
  kernel label, flops, entry point | the non-zero ConvDesc fields | the arguments after the descriptor, in
  order (op: / ptr: a tensor operand as dtype[shape]/[strides], ptr with the dtype asked for; addr the
  workspace; - a null pointer) | the CONV_PROFILE_INFO record | the returned tensor."""
import ctypes as C
import functools

import pytest
import torch

BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
NAMES = {BF: 'bf16', F32: 'f32', U8: 'u8', torch.float16: 'f16', torch.float64: 'f64'}
WS_ADDR = 0x5ca7c4


def c8(B, ch, H, W, dtype=BF):
    """A C8 tensor of `ch` channels (B, ch / 8, H, W, 8) without storage."""
    return torch.empty((B, ch // 8, H, W, 8), device='meta', dtype=dtype)


def m8(B, ch, H, W):
    return c8(B, ch, H, W, U8)


def t(*shape, dtype=F32):
    return torch.empty(shape, device='meta', dtype=dtype)


@functools.lru_cache(maxsize=None)
def layer(cin, cout, pad=1, mma='bf16c8', relu=True):
    from iterative_inference_segm_amd import ops
    return ops.Conv(torch.zeros(cout, cin, 3, 3), torch.zeros(cout), pad, relu, device='cpu', mma=mma)


def stack64():
    return c8(2, 64, 8, 8)


def dense(**kw):
    """The dense-block call: the first 48 channels of a 64-channel stack (a 40-channel layer: 8 of padding),
    BatchNorm + ReLU on the way in, the 16 produced channels into the stack's last slice."""
    s = stack64()
    return layer(40, 16), s, dict(in_c=48, bn=(t(48), t(48)), out=s, out_c0=48, **kw)


X3 = dict(mma='bf16x3')
# name -> () -> (layer, x1, keyword arguments); B = 2, maps of 8 x 8 or 9 x 9
CASES = {
    # the main kernel, 16 -> 32 channels (the concat: 16 + 16 -> 32)
    'main_plain': lambda: (layer(16, 32), c8(2, 16, 8, 8), {}),
    'main_concat': lambda: (layer(32, 32), c8(2, 16, 9, 9), dict(x2=c8(2, 16, 9, 9))),
    'main_window_place': lambda: (layer(16, 32), c8(2, 16, 9, 9),
                                  dict(window=(2, 3, 4, 5), out=c8(2, 32, 9, 9), place=(2, 3))),
    'main_x1_slice': lambda: (layer(16, 32), c8(2, 48, 8, 8)[:, 2:4], {}),
    'main_out_c0': lambda: (layer(16, 32), c8(2, 16, 8, 8), dict(out=c8(2, 80, 8, 8), out_c0=16)),
    'main_add_bf16_off': lambda: (layer(16, 32), c8(2, 16, 8, 8), dict(add=c8(2, 32, 10, 11), add_off=(1, 2))),
    'main_add_f32_c8f32': lambda: (layer(16, 32), c8(2, 16, 8, 8),
                                   dict(add=c8(2, 32, 8, 8, F32), out_format='c8f32')),
    'main_pool_mask_only_5x5': lambda: (layer(16, 32), c8(2, 16, 9, 9),
                                        dict(window=(2, 2, 5, 5), pool_out=c8(2, 32, 4, 4),
                                             mask_out=m8(2, 32, 4, 4), store_out=False)),
    'main_pool_mask_only_1x1': lambda: (layer(16, 32), c8(2, 16, 9, 9),
                                        dict(window=(4, 6, 1, 1), pool_out=c8(2, 32, 4, 4),
                                             mask_out=m8(2, 32, 4, 4), store_out=False)),
    'main_pool_only_placed': lambda: (layer(16, 32), c8(2, 16, 9, 9),
                                      dict(window=(2, 2, 5, 3), out=c8(2, 32, 9, 9), place=(2, 2),
                                           pool_out=c8(2, 32, 4, 4), mask_out=m8(2, 32, 4, 4), store_out=False)),
    'main_pool_stored': lambda: (layer(16, 32), c8(2, 16, 8, 8), dict(pool_out=c8(2, 32, 4, 4))),
    'main_depool': lambda: (layer(16, 32), c8(2, 16, 4, 4), dict(mask_in=m8(2, 16, 4, 4), unpool_hw=(9, 9))),
    'main_zins': lambda: (layer(16, 32, 0), c8(2, 16, 3, 4), dict(zins=True)),
    'main_cout11_add_nchw': lambda: (layer(16, 11, 1, 'bf16c8', False), c8(2, 16, 8, 8),
                                     dict(add=c8(2, 16, 8, 8))),
    'main_out_given': lambda: (layer(16, 32), c8(2, 16, 8, 8), dict(out=c8(2, 32, 8, 8))),
    # the bf16x3 layer: hi / lo pairs
    'x3_plain': lambda: (layer(16, 32, **X3), c8(2, 32, 8, 8), {}),
    'x3_pool_mask': lambda: (layer(16, 32, **X3), c8(2, 32, 8, 8),
                             dict(pool_out=c8(2, 64, 4, 4), mask_out=m8(2, 32, 4, 4))),
    'x3_depool': lambda: (layer(16, 32, **X3), c8(2, 32, 4, 4), dict(mask_in=m8(2, 16, 4, 4), unpool_hw=(9, 9))),
    'x3_add_bf16_pair': lambda: (layer(16, 32, **X3), c8(2, 32, 8, 8), dict(add=c8(2, 64, 8, 8))),
    # the 16-channel kernel
    'm16_c8': lambda: (layer(16, 16), c8(2, 16, 8, 8), {}),
    'm16_cout11_nchw': lambda: (layer(16, 11, 1, 'bf16c8', False), c8(2, 16, 9, 9), {}),
    'm16_cout16_nchw': lambda: (layer(16, 16), c8(2, 16, 8, 8), dict(out_format='nchw')),
    'm16_depool_window': lambda: (layer(16, 16), c8(2, 16, 4, 4),
                                  dict(mask_in=m8(2, 16, 4, 4), unpool_hw=(9, 9), window=(1, 2, 5, 4))),
    'm16_place': lambda: (layer(16, 16), c8(2, 16, 8, 8), dict(out=c8(2, 16, 9, 10), place=(1, 2))),
    'm16_place_nchw': lambda: (layer(16, 11), c8(2, 16, 8, 8), dict(out=t(2, 11, 9, 10), place=(1, 2))),
    'm16_wide_out_is_slice_0': lambda: (layer(16, 16), c8(2, 16, 8, 8), dict(out=c8(2, 32, 8, 8))),
    'm16_two_chunk_slice_out': lambda: (layer(16, 16), c8(2, 16, 8, 8), dict(out=c8(2, 48, 8, 8)[:, 2:4])),
    'm16_dense': lambda: dense(),
    'm16_dense_stats': lambda: dense(stats=(t(64), t(64), 1e-4)),
    'm16_dense_stats_fold': lambda: dense(stats=(t(64), t(64), 1e-4), fold=(t(64), t(64), t(64), t(64), 64)),
    # iiseg_conv_c8_m16_workspace_bytes: every launch it accepts has the per-tile statistics (512 bytes here);
    # 512 input channels on a 8 x 8 map split K and add their slabs (524800 bytes); a window past the map is
    # what it answers 0 to (no workspace is taken; the launch itself is the library's to refuse)
    'm16_workspace': lambda: (layer(512, 16), c8(2, 512, 8, 8), {}),
    'm16_no_workspace': lambda: (layer(16, 16), c8(2, 16, 8, 8), dict(window=(4, 4, 8, 8))),
}

# the choice between the two kernels: one eligible call, then every term of the condition flipped once
CHOICE = {
    'eligible': (lambda: (layer(16, 16), c8(2, 16, 8, 8), {}), 'conv_c8_m16_kernel'),
    'eligible_pad0': (lambda: (layer(16, 16, 0), c8(2, 16, 8, 8), {}), 'conv_c8_m16_kernel'),
    'eligible_concat_layer': (lambda: (layer(32, 16), c8(2, 32, 8, 8), {}), 'conv_c8_m16_kernel'),
    'cout_32': (lambda: (layer(16, 32), c8(2, 16, 8, 8), {}), 'conv_c8_kernel'),
    'x3_layer': (lambda: (layer(16, 16, **X3), c8(2, 32, 8, 8), {}), 'conv_c8_kernel<x3>'),
    'x2': (lambda: (layer(32, 16), c8(2, 16, 8, 8), dict(x2=c8(2, 16, 8, 8))), 'conv_c8_kernel'),
    'add': (lambda: (layer(16, 16), c8(2, 16, 8, 8), dict(add=c8(2, 16, 8, 8))), 'conv_c8_kernel'),
    'pool_out': (lambda: (layer(16, 16), c8(2, 16, 8, 8), dict(pool_out=c8(2, 16, 4, 4))), 'conv_c8_kernel'),
    'store_out_false': (lambda: (layer(16, 16), c8(2, 16, 8, 8),
                                 dict(pool_out=c8(2, 16, 4, 4), store_out=False)), 'conv_c8_kernel'),
    'c8f32': (lambda: (layer(16, 16), c8(2, 16, 8, 8), dict(out_format='c8f32')), 'conv_c8_kernel'),
    'zins': (lambda: (layer(16, 16, 0), c8(2, 16, 3, 3), dict(zins=True)), 'conv_c8_kernel'),
}

L, L0, M, D = (16, 32), (16, 32, 0), (16, 16), (40, 16)
X = lambda h=8, w=8, ch=16: c8(2, ch, h, w)
POOL = lambda **kw: dict(pool_out=c8(2, 32, 4, 4), **kw)
STATS = lambda **kw: dict(stats=(t(64), t(64), 1e-4), **kw)
wide = lambda ch=32, h=8, w=16: c8(2, ch, h, w)[:, :, :, :8]          # rows cut out of wider ones: no C8 operand
# name -> (a fragment of the message, () -> (layer, x1, keyword arguments)): every condition of every `raise`
REFUSALS = {
    # which layer, which kernel
    'not_a_c8_layer': ("C8 input needs a 3x3 layer built with mma='bf16c8'",
                       lambda: (layer(16, 32, 1, 'bf16'), X(), {})),
    'stats_main': ('stats: layers with at most 16 output channels', lambda: (layer(*L), X(), STATS())),
    'fold_main': ('stats: layers with at most 16 output channels',
                  lambda: (layer(*L), X(), dict(fold=(t(64), t(64), t(64), t(64), 64)))),
    'stats_not_eligible': ('stats: layers with at most 16 output channels',
                           lambda: (layer(*M), X(), STATS(add=c8(2, 16, 8, 8)))),
    'in_c_main': ('in_c / bn on C8 input: layers with at most 16', lambda: (layer(*L), X(), dict(in_c=16))),
    'bn_main': ('in_c / bn on C8 input: layers with at most 16',
                lambda: (layer(*L), X(), dict(bn=(t(16), t(16))))),
    'bn_not_eligible': ('in_c / bn on C8 input: layers with at most 16',
                        lambda: (layer(*M), X(), dict(bn=(t(16), t(16)), out_format='c8f32'))),
    'store_out_false_alone_m16_layer': ('store_out=False needs pool_out',
                                        lambda: (layer(*M), X(), dict(store_out=False))),
    # operand strides (the main kernel takes x1 and `out` as channel slices, nothing else)
    'x2_strided': ('C8 launch: x2 must be contiguous',
                   lambda: (layer(32, 32), X(), dict(x2=c8(2, 48, 8, 8)[:, 2:4]))),
    'add_strided': ('C8 launch: add must be contiguous', lambda: (layer(*L), X(), dict(add=c8(2, 64, 8, 8)[:, :4]))),
    'pool_out_strided': ('C8 launch: pool_out must be contiguous',
                         lambda: (layer(*L), X(), dict(pool_out=c8(2, 64, 4, 4)[:, :4]))),
    'mask_out_strided': ('C8 launch: mask_out must be contiguous',
                         lambda: (layer(*L), X(), POOL(mask_out=m8(2, 64, 4, 4)[:, :4]))),
    'x1_rows_cut': ('C8 operand: a contiguous tensor or a channel slice', lambda: (layer(*L), wide(16), {})),
    'out_rows_cut': ('C8 operand: a contiguous tensor or a channel slice', lambda: (layer(*L), X(), dict(out=wide()))),
    'm16_x1_rows_cut': ('C8 operand: a contiguous tensor or a channel slice', lambda: (layer(*M), wide(16), {})),
    'm16_out_rows_cut': ('C8 operand: a contiguous tensor or a channel slice',
                         lambda: (layer(*M), X(), dict(out=wide(16)))),
    # bf16x3
    'x3_odd_planes': ('bf16x3 layer: hi / lo pair input', lambda: (layer(16, 32, **X3), c8(2, 24, 8, 8), {})),
    'x3_concat': ('bf16x3 layer: hi / lo pair input',
                  lambda: (layer(32, 32, **X3), c8(2, 32, 8, 8), dict(x2=c8(2, 32, 8, 8)))),
    # DePool2D input
    'depool_with_x2': ('C8 DePool2D input: up', lambda: (layer(32, 32), X(4, 4), dict(
        x2=c8(2, 16, 9, 9), mask_in=m8(2, 16, 4, 4), unpool_hw=(9, 9)))),
    'depool_no_hw': ('C8 DePool2D input: up', lambda: (layer(*L), X(4, 4), dict(mask_in=m8(2, 16, 4, 4)))),
    'depool_mask_dtype': ('C8 DePool2D input: up', lambda: (layer(*L), X(4, 4), dict(
        mask_in=c8(2, 16, 4, 4), unpool_hw=(9, 9)))),
    'depool_mask_shape': ('C8 DePool2D input: up', lambda: (layer(*L), X(4, 4), dict(
        mask_in=m8(2, 32, 4, 4), unpool_hw=(9, 9)))),
    'depool_hw_mismatch': ('C8 DePool2D input: up', lambda: (layer(*L), X(4, 4), dict(
        mask_in=m8(2, 16, 4, 4), unpool_hw=(10, 9)))),
    'x3_depool_mask_planes': ('C8 DePool2D input: up', lambda: (layer(16, 32, **X3), c8(2, 32, 4, 4), dict(
        mask_in=m8(2, 32, 4, 4), unpool_hw=(9, 9)))),
    'm16_depool_in_c': ('C8 DePool2D input: up', lambda: (layer(*M), c8(2, 32, 4, 4), dict(
        in_c=16, mask_in=m8(2, 32, 4, 4), unpool_hw=(9, 9)))),
    'm16_depool_x1_slice': ('C8 DePool2D input: up', lambda: (layer(*M), c8(2, 32, 4, 4)[:, :2], dict(
        mask_in=m8(2, 16, 4, 4), unpool_hw=(9, 9)))),
    'm16_depool_no_hw': ('C8 DePool2D input: up', lambda: (layer(*M), X(4, 4), dict(mask_in=m8(2, 16, 4, 4)))),
    'm16_depool_mask_dtype': ('C8 DePool2D input: up', lambda: (layer(*M), X(4, 4), dict(
        mask_in=c8(2, 16, 4, 4), unpool_hw=(9, 9)))),
    'm16_depool_mask_shape': ('C8 DePool2D input: up', lambda: (layer(*M), X(4, 4), dict(
        mask_in=m8(2, 16, 4, 5), unpool_hw=(9, 9)))),
    'm16_depool_hw_mismatch': ('C8 DePool2D input: up', lambda: (layer(*M), X(4, 4), dict(
        mask_in=m8(2, 16, 4, 4), unpool_hw=(9, 11)))),
    # zero-inserted input
    'zins_x3': ('zero-inserted input: plain single-source valid layers',
                lambda: (layer(16, 32, 0, 'bf16x3'), c8(2, 32, 3, 3), dict(zins=True))),
    'zins_x2': ('zero-inserted input: plain single-source valid layers',
                lambda: (layer(32, 32, 0), X(3, 3), dict(x2=X(3, 3), zins=True))),
    'zins_padded_layer': ('zero-inserted input: plain single-source valid layers',
                          lambda: (layer(*L), X(3, 3), dict(zins=True))),
    # x1 as a channel slice
    'x1_slice_x3': ('channel-slice input: plain bf16 launches only',
                    lambda: (layer(16, 32, **X3), c8(2, 64, 8, 8)[:, :4], {})),
    'x1_slice_depool': ('channel-slice input: plain bf16 launches only', lambda: (
        layer(*L), c8(2, 48, 4, 4)[:, 2:4], dict(mask_in=m8(2, 16, 4, 4), unpool_hw=(9, 9)))),
    # concat
    'x2_not_c8': ('concat shapes', lambda: (layer(32, 32), X(), dict(x2=c8(2, 16, 8, 8, F32)))),
    'x2_batch': ('concat shapes', lambda: (layer(32, 32), X(), dict(x2=c8(3, 16, 8, 8)))),
    'x2_map': ('concat shapes', lambda: (layer(32, 32), X(), dict(x2=c8(2, 16, 8, 9)))),
    'x2_padded_sources': ('C8 concat needs unpadded sources', lambda: (layer(24, 32), X(), dict(x2=X()))),
    'too_few_channels': ('input channels in whole 16-channel groups', lambda: (layer(32, 32), X(), {})),
    'x1_odd_chunks': ('input channels in whole 16-channel groups', lambda: (layer(*L), X(ch=24), {})),
    'x2_odd_chunks': ('input channels in whole 16-channel groups', lambda: (layer(24, 32), X(), dict(x2=X(ch=8)))),
    # add
    'add_4d': ('add tensor shape', lambda: (layer(*L), X(), dict(add=t(2, 32, 8, 8)))),
    'add_batch': ('add tensor shape', lambda: (layer(*L), X(), dict(add=c8(3, 32, 8, 8)))),
    'add_chunks': ('add tensor shape', lambda: (layer(*L), X(), dict(add=c8(2, 16, 8, 8)))),
    'add_f32_pair_chunks_x3': ('add tensor shape',
                               lambda: (layer(16, 32, **X3), X(ch=32), dict(add=c8(2, 64, 8, 8, F32)))),
    'add_dtype': ('add tensor shape', lambda: (layer(*L), X(), dict(add=c8(2, 32, 8, 8, torch.float16)))),
    # the main kernel's output target
    'place_no_target': ('placement needs a target', lambda: (layer(*L), X(), dict(place=(0, 0)))),
    'store_out_false_no_pool': ('store_out=False needs pool_out', lambda: (layer(*L), X(), dict(store_out=False))),
    'slice_no_target': ('bad C8 output slice None', lambda: (layer(*L), X(), POOL(store_out=False, out_c0=0))),
    'slice_c8f32': ('bad C8 output slice', lambda: (layer(*L), X(), dict(
        out=c8(2, 64, 8, 8, F32), out_c0=0, out_format='c8f32'))),
    'slice_x3': ('bad C8 output slice', lambda: (layer(16, 32, **X3), X(ch=32), dict(out=c8(2, 128, 8, 8), out_c0=0))),
    'slice_not_c8': ('bad C8 output slice', lambda: (layer(*L), X(), dict(out=c8(2, 64, 8, 8, F32), out_c0=0))),
    'slice_c0_8': ('bad C8 output slice', lambda: (layer(*L), X(), dict(out=c8(2, 64, 8, 8), out_c0=8))),
    'slice_too_far': ('bad C8 output slice', lambda: (layer(*L), X(), dict(out=c8(2, 64, 8, 8), out_c0=48))),
    'slice_batch': ('bad C8 output slice', lambda: (layer(*L), X(), dict(out=c8(3, 64, 8, 8), out_c0=16))),
    'slice_map': ('bad C8 output slice', lambda: (layer(*L), X(), dict(out=c8(2, 64, 8, 9), out_c0=16))),
    'nchw_target_5d': ('bad C8 output target', lambda: (layer(16, 11), X(), dict(add=X(), out=c8(2, 16, 8, 8, F32)))),
    'nchw_target_dtype': ('bad C8 output target',
                          lambda: (layer(16, 11), X(), dict(add=X(), out=t(2, 11, 8, 8, dtype=BF)))),
    'nchw_target_channels': ('bad C8 output target', lambda: (layer(16, 11), X(), dict(add=X(), out=t(2, 16, 8, 8)))),
    'c8_target_4d': ('bad C8 output target', lambda: (layer(*L), X(), dict(out=t(2, 32, 8, 8, dtype=BF)))),
    'c8_target_chunks': ('bad C8 output target', lambda: (layer(*L), X(), dict(out=c8(2, 64, 8, 8)))),
    'c8_target_dtype': ('bad C8 output target', lambda: (layer(*L), X(), dict(out=c8(2, 32, 8, 8, F32)))),
    'c8f32_target_dtype': ('bad C8 output target',
                           lambda: (layer(*L), X(), dict(out=c8(2, 32, 8, 8), out_format='c8f32'))),
    'x3_target_not_a_pair': ('bad C8 output target', lambda: (layer(16, 32, **X3), X(ch=32), dict(out=c8(2, 32, 8, 8)))),
    'target_batch': ('bad C8 output target', lambda: (layer(*L), X(), dict(out=c8(3, 32, 8, 8)))),
    'target_map': ('bad C8 output target', lambda: (layer(*L), X(), dict(out=c8(2, 32, 9, 8)))),
    # pool and mask bytes
    'pool_out_not_c8': ('pool_out shape', lambda: (layer(*L), X(), dict(pool_out=c8(2, 32, 4, 4, F32)))),
    'pool_out_map': ('pool_out shape', lambda: (layer(*L), X(9, 9), dict(pool_out=c8(2, 32, 5, 5)))),
    'pool_out_x3_not_a_pair': ('pool_out shape', lambda: (layer(16, 32, **X3), X(ch=32), dict(pool_out=c8(2, 32, 4, 4)))),
    'mask_out_dtype': ('mask_out: uint8', lambda: (layer(*L), X(), POOL(mask_out=c8(2, 32, 4, 4)))),
    'mask_out_shape': ('mask_out: uint8', lambda: (layer(*L), X(), POOL(mask_out=m8(2, 16, 4, 4)))),
    'mask_out_no_pool': ('mask_out needs pool_out', lambda: (layer(*L), X(), dict(mask_out=m8(2, 32, 4, 4)))),
    # the 16-channel kernel: the first in_c channels of a stack
    'm16_in_c_24': ('conv of 16 input channels on the first 24 of 32', lambda: (layer(*M), X(ch=32), dict(in_c=24))),
    'm16_in_c_too_wide': ('conv of 16 input channels on the first 32 of 16', lambda: (layer(*M), X(), dict(in_c=32))),
    'm16_in_c_below_cin': ('conv of 40 input channels on the first 32 of 64',
                           lambda: (layer(*D), stack64(), dict(in_c=32))),
    'm16_in_c_16_over': ('conv of 16 input channels on the first 32 of 32', lambda: (layer(*M), X(ch=32), {})),
    # ... its output target
    'm16_place_no_target': ('placement needs a target', lambda: (layer(*M), X(), dict(place=(0, 0)))),
    'm16_out_c0_no_target': ('out_c0 needs a target', lambda: (layer(*M), X(), dict(out_c0=0))),
    'm16_nchw_5d': ('for a 16-channel C8 layer', lambda: (layer(16, 11), X(), dict(out=c8(2, 16, 8, 8, F32)))),
    'm16_nchw_dtype': ('for a 16-channel C8 layer', lambda: (layer(16, 11), X(), dict(out=t(2, 11, 8, 8, dtype=BF)))),
    'm16_nchw_channels': ('for a 16-channel C8 layer', lambda: (layer(16, 11), X(), dict(out=t(2, 16, 8, 8)))),
    'm16_nchw_out_c0': ('for a 16-channel C8 layer', lambda: (layer(16, 11), X(), dict(out=t(2, 11, 8, 8), out_c0=0))),
    'm16_c8_4d': ('for a 16-channel C8 layer', lambda: (layer(*M), X(), dict(out=t(2, 16, 8, 8, dtype=BF)))),
    'm16_c8_dtype': ('for a 16-channel C8 layer', lambda: (layer(*M), X(), dict(out=c8(2, 16, 8, 8, F32)))),
    'm16_c8_odd_chunks': ('for a 16-channel C8 layer', lambda: (layer(*M), X(), dict(out=c8(2, 24, 8, 8)))),
    'm16_slice_c0_8': ('for a 16-channel C8 layer', lambda: (layer(*M), X(), dict(out=stack64(), out_c0=8))),
    'm16_slice_too_far': ('for a 16-channel C8 layer', lambda: (layer(*M), X(), dict(out=stack64(), out_c0=64))),
    'm16_target_batch': ('for a 16-channel C8 layer', lambda: (layer(*M), X(), dict(out=c8(3, 16, 8, 8)))),
    'm16_target_map': ('for a 16-channel C8 layer', lambda: (layer(*M), X(), dict(out=c8(2, 16, 8, 9)))),
    # ... its BatchNorm input, statistics and fold
    'm16_bn_three': (r'bn = \(a, b\): float32, at least 16', lambda: (layer(*M), X(), dict(bn=(t(16), t(16), t(16))))),
    'm16_bn_dtype': (r'bn = \(a, b\): float32, at least 16',
                     lambda: (layer(*M), X(), dict(bn=(t(16), t(16, dtype=torch.float64))))),
    'm16_bn_short': (r'bn = \(a, b\): float32, at least 48', lambda: dense()[:2] + (dict(in_c=48, bn=(t(48), t(47))),)),
    'm16_stats_nchw': ('stats = ', lambda: (layer(*M), X(), STATS(out_format='nchw'))),
    'm16_stats_mean_dtype': ('stats = ', lambda: (layer(*M), X(), dict(stats=(t(16, dtype=torch.float64), t(16), 1e-4)))),
    'm16_stats_inv_std_dtype': ('stats = ', lambda: (layer(*M), X(), dict(stats=(t(16), t(16, dtype=BF), 1e-4)))),
    'm16_stats_short': ('stats = ', lambda: dense(stats=(t(64), t(63), 1e-4))),
    'm16_fold_no_stats': ('fold = ', lambda: (layer(*M), X(), dict(fold=(t(16), t(16), t(16), t(16), 16)))),
    'm16_fold_dtype': ('fold = ', lambda: (layer(*M), X(), dict(
        stats=(t(16), t(16), 1e-4), fold=(t(16), t(16), t(16, dtype=torch.float64), t(16), 16)))),
    'm16_fold_short': ('fold = ', lambda: (layer(*M), X(), dict(
        stats=(t(16), t(16), 1e-4), fold=(t(16), t(15), t(16), t(16), 16)))),
}

EXPECTED = {
    'main_plain': (
        'conv_c8_kernel 1179648.0 iiseg_conv_c8_slice',
        'B=2 C1=16 H=8 W=8 Cout=32 KH=3 KW=3 pad=1 dil=1 OH=8 OW=8 flags=1',
        'op:bf16[2, 2, 8, 8, 8]/[1024, 512, 64, 8, 1] 0 - - w16 ptr:f32[32]/[1]:f32 - 0 op:bf16[2, 4, 8, 8, 8]/[2048, 512, 64, 8, 1] 1 - -',
        'B=2 C1=16 C2=0 Cin=16 Cout=32 H=8 OH=8 OW=8 W=8 add=0 flat=(0,8,8,0) kind=1 pool=False unpool=False',
        'bf16[2, 4, 8, 8, 8]/[2048, 512, 64, 8, 1]',
    ),
    'main_concat': (
        'conv_c8_kernel 2985984.0 iiseg_conv_c8_slice',
        'B=2 C1=16 C2=16 H=9 W=9 Cout=32 KH=3 KW=3 pad=1 dil=1 OH=9 OW=9 flags=1',
        'op:bf16[2, 2, 9, 9, 8]/[1296, 648, 72, 8, 1] 0 op:bf16[2, 2, 9, 9, 8]/[1296, 648, 72, 8, 1] - w16 ptr:f32[32]/[1]:f32 - 0 op:bf16[2, 4, 9, 9, 8]/[2592, 648, 72, 8, 1] 1 - -',
        'B=2 C1=16 C2=16 Cin=32 Cout=32 H=9 OH=9 OW=9 W=9 add=0 flat=(0,9,9,0) kind=1 pool=False unpool=False',
        'bf16[2, 4, 9, 9, 8]/[2592, 648, 72, 8, 1]',
    ),
    'main_window_place': (
        'conv_c8_kernel 368640.0 iiseg_conv_c8_slice',
        'B=2 C1=16 H=9 W=9 Cout=32 KH=3 KW=3 pad=1 dil=1 oy0=2 ox0=3 OH=4 OW=5 flags=1 out_H=9 out_W=9 out_y0=2 out_x0=3',
        'op:bf16[2, 2, 9, 9, 8]/[1296, 648, 72, 8, 1] 0 - - w16 ptr:f32[32]/[1]:f32 - 0 op:bf16[2, 4, 9, 9, 8]/[2592, 648, 72, 8, 1] 1 - -',
        'B=2 C1=16 C2=0 Cin=16 Cout=32 H=9 OH=4 OW=5 W=9 add=0 flat=(0,4,5,0) kind=1 pool=False unpool=False',
        'bf16[2, 4, 9, 9, 8]/[2592, 648, 72, 8, 1] (the out given)',
    ),
    'main_x1_slice': (
        'conv_c8_kernel 1179648.0 iiseg_conv_c8_slice',
        'B=2 C1=16 H=8 W=8 Cout=32 KH=3 KW=3 pad=1 dil=1 OH=8 OW=8 flags=1',
        'op:bf16[2, 2, 8, 8, 8]/[3072, 512, 64, 8, 1] 48 - - w16 ptr:f32[32]/[1]:f32 - 0 op:bf16[2, 4, 8, 8, 8]/[2048, 512, 64, 8, 1] 1 - -',
        'B=2 C1=16 C2=0 Cin=16 Cout=32 H=8 OH=8 OW=8 W=8 add=0 flat=(0,8,8,0) kind=1 pool=False unpool=False',
        'bf16[2, 4, 8, 8, 8]/[2048, 512, 64, 8, 1]',
    ),
    'main_out_c0': (
        'conv_c8_kernel 1179648.0 iiseg_conv_c8_slice',
        'B=2 C1=16 H=8 W=8 Cout=32 KH=3 KW=3 pad=1 dil=1 OH=8 OW=8 flags=1 out_ctot=80 out_c0=16',
        'op:bf16[2, 2, 8, 8, 8]/[1024, 512, 64, 8, 1] 0 - - w16 ptr:f32[32]/[1]:f32 - 0 op:bf16[2, 10, 8, 8, 8]/[5120, 512, 64, 8, 1] 1 - -',
        'B=2 C1=16 C2=0 Cin=16 Cout=32 H=8 OH=8 OW=8 W=8 add=0 flat=(0,8,8,0) kind=1 pool=False unpool=False',
        'bf16[2, 10, 8, 8, 8]/[5120, 512, 64, 8, 1] (the out given)',
    ),
    'main_add_bf16_off': (
        'conv_c8_kernel 1179648.0 iiseg_conv_c8_slice',
        'B=2 C1=16 H=8 W=8 Cout=32 KH=3 KW=3 pad=1 dil=1 OH=8 OW=8 AH=10 AW=11 ay0=1 ax0=2 flags=1',
        'op:bf16[2, 2, 8, 8, 8]/[1024, 512, 64, 8, 1] 0 - - w16 ptr:f32[32]/[1]:f32 op:bf16[2, 4, 10, 11, 8]/[3520, 880, 88, 8, 1] 1 op:bf16[2, 4, 8, 8, 8]/[2048, 512, 64, 8, 1] 1 - -',
        'B=2 C1=16 C2=0 Cin=16 Cout=32 H=8 OH=8 OW=8 W=8 add=1 flat=(0,8,8,0) kind=1 pool=False unpool=False',
        'bf16[2, 4, 8, 8, 8]/[2048, 512, 64, 8, 1]',
    ),
    'main_add_f32_c8f32': (
        'conv_c8_kernel 1179648.0 iiseg_conv_c8_slice',
        'B=2 C1=16 H=8 W=8 Cout=32 KH=3 KW=3 pad=1 dil=1 OH=8 OW=8 AH=8 AW=8 flags=1',
        'op:bf16[2, 2, 8, 8, 8]/[1024, 512, 64, 8, 1] 0 - - w16 ptr:f32[32]/[1]:f32 op:f32[2, 4, 8, 8, 8]/[2048, 512, 64, 8, 1] 2 op:f32[2, 4, 8, 8, 8]/[2048, 512, 64, 8, 1] 2 - -',
        'B=2 C1=16 C2=0 Cin=16 Cout=32 H=8 OH=8 OW=8 W=8 add=2 flat=(0,8,8,0) kind=2 pool=False unpool=False',
        'f32[2, 4, 8, 8, 8]/[2048, 512, 64, 8, 1]',
    ),
    'main_pool_mask_only_5x5': (
        'conv_c8_kernel 294912.0 iiseg_conv_c8_slice',
        'B=2 C1=16 H=9 W=9 Cout=32 KH=3 KW=3 pad=1 dil=1 oy0=2 ox0=2 OH=4 OW=4 flags=1',
        'op:bf16[2, 2, 9, 9, 8]/[1296, 648, 72, 8, 1] 0 - - w16 ptr:f32[32]/[1]:f32 - 0 - 0 op:bf16[2, 4, 4, 4, 8]/[512, 128, 32, 8, 1] op:u8[2, 4, 4, 4, 8]/[512, 128, 32, 8, 1]',
        'B=2 C1=16 C2=0 Cin=16 Cout=32 H=9 OH=4 OW=4 W=9 add=0 flat=(0,4,4,1) kind=0 pool=True unpool=False',
        '-',
    ),
    'main_pool_mask_only_1x1': (
        'conv_c8_kernel 18432.0 iiseg_conv_c8_slice',
        'B=2 C1=16 H=9 W=9 Cout=32 KH=3 KW=3 pad=1 dil=1 oy0=4 ox0=6 OH=1 OW=1 flags=1',
        'op:bf16[2, 2, 9, 9, 8]/[1296, 648, 72, 8, 1] 0 - - w16 ptr:f32[32]/[1]:f32 - 0 - 0 op:bf16[2, 4, 4, 4, 8]/[512, 128, 32, 8, 1] op:u8[2, 4, 4, 4, 8]/[512, 128, 32, 8, 1]',
        'B=2 C1=16 C2=0 Cin=16 Cout=32 H=9 OH=1 OW=1 W=9 add=0 flat=(0,2,2,1) kind=0 pool=True unpool=False',
        '-',
    ),
    'main_pool_only_placed': (
        'conv_c8_kernel 147456.0 iiseg_conv_c8_slice',
        'B=2 C1=16 H=9 W=9 Cout=32 KH=3 KW=3 pad=1 dil=1 oy0=2 ox0=2 OH=4 OW=2 flags=1 out_H=9 out_W=9 out_y0=2 out_x0=2',
        'op:bf16[2, 2, 9, 9, 8]/[1296, 648, 72, 8, 1] 0 - - w16 ptr:f32[32]/[1]:f32 - 0 - 0 op:bf16[2, 4, 4, 4, 8]/[512, 128, 32, 8, 1] op:u8[2, 4, 4, 4, 8]/[512, 128, 32, 8, 1]',
        'B=2 C1=16 C2=0 Cin=16 Cout=32 H=9 OH=4 OW=2 W=9 add=0 flat=(0,4,2,1) kind=0 pool=True unpool=False',
        '-',
    ),
    'main_pool_stored': (
        'conv_c8_kernel 1179648.0 iiseg_conv_c8_slice',
        'B=2 C1=16 H=8 W=8 Cout=32 KH=3 KW=3 pad=1 dil=1 OH=8 OW=8 flags=1',
        'op:bf16[2, 2, 8, 8, 8]/[1024, 512, 64, 8, 1] 0 - - w16 ptr:f32[32]/[1]:f32 - 0 op:bf16[2, 4, 8, 8, 8]/[2048, 512, 64, 8, 1] 1 op:bf16[2, 4, 4, 4, 8]/[512, 128, 32, 8, 1] -',
        'B=2 C1=16 C2=0 Cin=16 Cout=32 H=8 OH=8 OW=8 W=8 add=0 flat=(0,8,8,1) kind=1 pool=True unpool=False',
        'bf16[2, 4, 8, 8, 8]/[2048, 512, 64, 8, 1]',
    ),
    'main_depool': (
        'conv_c8_kernel 1492992.0 iiseg_conv_c8_slice',
        'B=2 C1=16 H=9 W=9 Cout=32 KH=3 KW=3 pad=1 dil=1 OH=9 OW=9 flags=3',
        'op:bf16[2, 2, 4, 4, 8]/[256, 128, 32, 8, 1] 0 - op:u8[2, 2, 4, 4, 8]/[256, 128, 32, 8, 1] w16 ptr:f32[32]/[1]:f32 - 0 op:bf16[2, 4, 9, 9, 8]/[2592, 648, 72, 8, 1] 1 - -',
        'B=2 C1=16 C2=0 Cin=16 Cout=32 H=9 OH=9 OW=9 W=9 add=0 flat=(0,9,9,0) kind=1 pool=False unpool=True',
        'bf16[2, 4, 9, 9, 8]/[2592, 648, 72, 8, 1]',
    ),
    'main_zins': (
        'conv_c8_kernel 1161216.0 iiseg_conv_c8_slice',
        'B=2 C1=16 H=9 W=11 Cout=32 KH=3 KW=3 dil=1 OH=7 OW=9 flags=17',
        'op:bf16[2, 2, 3, 4, 8]/[192, 96, 32, 8, 1] 0 - - w16 ptr:f32[32]/[1]:f32 - 0 op:bf16[2, 4, 7, 9, 8]/[2016, 504, 72, 8, 1] 1 - -',
        'B=2 C1=16 C2=0 Cin=16 Cout=32 H=9 OH=7 OW=9 W=11 add=0 flat=(0,7,9,0) kind=1 pool=False unpool=False',
        'bf16[2, 4, 7, 9, 8]/[2016, 504, 72, 8, 1]',
    ),
    'main_cout11_add_nchw': (
        'conv_c8_kernel 405504.0 iiseg_conv_c8_slice',
        'B=2 C1=16 H=8 W=8 Cout=11 KH=3 KW=3 pad=1 dil=1 OH=8 OW=8 AH=8 AW=8',
        'op:bf16[2, 2, 8, 8, 8]/[1024, 512, 64, 8, 1] 0 - - w16 ptr:f32[11]/[1]:f32 op:bf16[2, 2, 8, 8, 8]/[1024, 512, 64, 8, 1] 1 op:f32[2, 11, 8, 8]/[704, 64, 8, 1] 3 - -',
        'B=2 C1=16 C2=0 Cin=16 Cout=11 H=8 OH=8 OW=8 W=8 add=1 flat=(0,8,8,0) kind=3 pool=False unpool=False',
        'f32[2, 11, 8, 8]/[704, 64, 8, 1]',
    ),
    'main_out_given': (
        'conv_c8_kernel 1179648.0 iiseg_conv_c8_slice',
        'B=2 C1=16 H=8 W=8 Cout=32 KH=3 KW=3 pad=1 dil=1 OH=8 OW=8 flags=1',
        'op:bf16[2, 2, 8, 8, 8]/[1024, 512, 64, 8, 1] 0 - - w16 ptr:f32[32]/[1]:f32 - 0 op:bf16[2, 4, 8, 8, 8]/[2048, 512, 64, 8, 1] 1 - -',
        'B=2 C1=16 C2=0 Cin=16 Cout=32 H=8 OH=8 OW=8 W=8 add=0 flat=(0,8,8,0) kind=1 pool=False unpool=False',
        'bf16[2, 4, 8, 8, 8]/[2048, 512, 64, 8, 1] (the out given)',
    ),
    'x3_plain': (
        'conv_c8_kernel<x3> 1179648.0 iiseg_conv_c8_slice',
        'B=2 C1=16 H=8 W=8 Cout=32 KH=3 KW=3 pad=1 dil=1 OH=8 OW=8 flags=9',
        'op:bf16[2, 4, 8, 8, 8]/[2048, 512, 64, 8, 1] 0 - - w16 ptr:f32[32]/[1]:f32 - 0 op:bf16[2, 8, 8, 8, 8]/[4096, 512, 64, 8, 1] 1 - -',
        'B=2 C1=16 C2=0 Cin=16 Cout=32 H=8 OH=8 OW=8 W=8 add=0 flat=(0,8,8,0) kind=1 pool=False unpool=False',
        'bf16[2, 8, 8, 8, 8]/[4096, 512, 64, 8, 1]',
    ),
    'x3_pool_mask': (
        'conv_c8_kernel<x3> 1179648.0 iiseg_conv_c8_slice',
        'B=2 C1=16 H=8 W=8 Cout=32 KH=3 KW=3 pad=1 dil=1 OH=8 OW=8 flags=9',
        'op:bf16[2, 4, 8, 8, 8]/[2048, 512, 64, 8, 1] 0 - - w16 ptr:f32[32]/[1]:f32 - 0 op:bf16[2, 8, 8, 8, 8]/[4096, 512, 64, 8, 1] 1 op:bf16[2, 8, 4, 4, 8]/[1024, 128, 32, 8, 1] op:u8[2, 4, 4, 4, 8]/[512, 128, 32, 8, 1]',
        'B=2 C1=16 C2=0 Cin=16 Cout=32 H=8 OH=8 OW=8 W=8 add=0 flat=(0,8,8,1) kind=1 pool=True unpool=False',
        'bf16[2, 8, 8, 8, 8]/[4096, 512, 64, 8, 1]',
    ),
    'x3_depool': (
        'conv_c8_kernel<x3> 1492992.0 iiseg_conv_c8_slice',
        'B=2 C1=16 H=9 W=9 Cout=32 KH=3 KW=3 pad=1 dil=1 OH=9 OW=9 flags=11',
        'op:bf16[2, 4, 4, 4, 8]/[512, 128, 32, 8, 1] 0 - op:u8[2, 2, 4, 4, 8]/[256, 128, 32, 8, 1] w16 ptr:f32[32]/[1]:f32 - 0 op:bf16[2, 8, 9, 9, 8]/[5184, 648, 72, 8, 1] 1 - -',
        'B=2 C1=16 C2=0 Cin=16 Cout=32 H=9 OH=9 OW=9 W=9 add=0 flat=(0,9,9,0) kind=1 pool=False unpool=True',
        'bf16[2, 8, 9, 9, 8]/[5184, 648, 72, 8, 1]',
    ),
    'x3_add_bf16_pair': (
        'conv_c8_kernel<x3> 1179648.0 iiseg_conv_c8_slice',
        'B=2 C1=16 H=8 W=8 Cout=32 KH=3 KW=3 pad=1 dil=1 OH=8 OW=8 AH=8 AW=8 flags=9',
        'op:bf16[2, 4, 8, 8, 8]/[2048, 512, 64, 8, 1] 0 - - w16 ptr:f32[32]/[1]:f32 op:bf16[2, 8, 8, 8, 8]/[4096, 512, 64, 8, 1] 1 op:bf16[2, 8, 8, 8, 8]/[4096, 512, 64, 8, 1] 1 - -',
        'B=2 C1=16 C2=0 Cin=16 Cout=32 H=8 OH=8 OW=8 W=8 add=1 flat=(0,8,8,0) kind=1 pool=False unpool=False',
        'bf16[2, 8, 8, 8, 8]/[4096, 512, 64, 8, 1]',
    ),
    'm16_c8': (
        'conv_c8_m16_kernel 589824.0 iiseg_conv_c8_m16_ws',
        'B=2 C1=16 H=8 W=8 Cout=16 KH=3 KW=3 pad=1 dil=1 OH=8 OW=8 flags=1',
        'op:bf16[2, 2, 8, 8, 8]/[1024, 512, 64, 8, 1] 16 - - - w16 ptr:f32[16]/[1]:f32 op:bf16[2, 2, 8, 8, 8]/[1024, 512, 64, 8, 1] 1 addr 512 - - 0.0 - - - - 0',
        'B=2 C1=16 C2=0 Cin=16 Cout=16 H=8 OH=8 OW=8 W=8 add=0 flat=m16 kind=1 pool=False unpool=False',
        'bf16[2, 2, 8, 8, 8]/[1024, 512, 64, 8, 1]',
    ),
    'm16_cout11_nchw': (
        'conv_c8_m16_kernel 513216.0 iiseg_conv_c8_m16_ws',
        'B=2 C1=16 H=9 W=9 Cout=11 KH=3 KW=3 pad=1 dil=1 OH=9 OW=9',
        'op:bf16[2, 2, 9, 9, 8]/[1296, 648, 72, 8, 1] 16 - - - w16 ptr:f32[11]/[1]:f32 op:f32[2, 11, 9, 9]/[891, 81, 9, 1] 3 addr 512 - - 0.0 - - - - 0',
        'B=2 C1=16 C2=0 Cin=16 Cout=11 H=9 OH=9 OW=9 W=9 add=0 flat=m16 kind=3 pool=False unpool=False',
        'f32[2, 11, 9, 9]/[891, 81, 9, 1]',
    ),
    'm16_cout16_nchw': (
        'conv_c8_m16_kernel 589824.0 iiseg_conv_c8_m16_ws',
        'B=2 C1=16 H=8 W=8 Cout=16 KH=3 KW=3 pad=1 dil=1 OH=8 OW=8 flags=1',
        'op:bf16[2, 2, 8, 8, 8]/[1024, 512, 64, 8, 1] 16 - - - w16 ptr:f32[16]/[1]:f32 op:f32[2, 16, 8, 8]/[1024, 64, 8, 1] 3 addr 512 - - 0.0 - - - - 0',
        'B=2 C1=16 C2=0 Cin=16 Cout=16 H=8 OH=8 OW=8 W=8 add=0 flat=m16 kind=3 pool=False unpool=False',
        'f32[2, 16, 8, 8]/[1024, 64, 8, 1]',
    ),
    'm16_depool_window': (
        'conv_c8_m16_kernel 184320.0 iiseg_conv_c8_m16_ws',
        'B=2 C1=16 H=9 W=9 Cout=16 KH=3 KW=3 pad=1 dil=1 oy0=1 ox0=2 OH=5 OW=4 flags=3',
        'op:bf16[2, 2, 4, 4, 8]/[256, 128, 32, 8, 1] 16 op:u8[2, 2, 4, 4, 8]/[256, 128, 32, 8, 1] - - w16 ptr:f32[16]/[1]:f32 op:bf16[2, 2, 5, 4, 8]/[320, 160, 32, 8, 1] 1 addr 512 - - 0.0 - - - - 0',
        'B=2 C1=16 C2=0 Cin=16 Cout=16 H=9 OH=5 OW=4 W=9 add=0 flat=m16 kind=1 pool=False unpool=True',
        'bf16[2, 2, 5, 4, 8]/[320, 160, 32, 8, 1]',
    ),
    'm16_place': (
        'conv_c8_m16_kernel 589824.0 iiseg_conv_c8_m16_ws',
        'B=2 C1=16 H=8 W=8 Cout=16 KH=3 KW=3 pad=1 dil=1 OH=8 OW=8 flags=1 out_H=9 out_W=10 out_y0=1 out_x0=2',
        'op:bf16[2, 2, 8, 8, 8]/[1024, 512, 64, 8, 1] 16 - - - w16 ptr:f32[16]/[1]:f32 op:bf16[2, 2, 9, 10, 8]/[1440, 720, 80, 8, 1] 1 addr 512 - - 0.0 - - - - 0',
        'B=2 C1=16 C2=0 Cin=16 Cout=16 H=8 OH=8 OW=8 W=8 add=0 flat=m16 kind=1 pool=False unpool=False',
        'bf16[2, 2, 9, 10, 8]/[1440, 720, 80, 8, 1] (the out given)',
    ),
    'm16_place_nchw': (
        'conv_c8_m16_kernel 405504.0 iiseg_conv_c8_m16_ws',
        'B=2 C1=16 H=8 W=8 Cout=11 KH=3 KW=3 pad=1 dil=1 OH=8 OW=8 flags=1 out_H=9 out_W=10 out_y0=1 out_x0=2',
        'op:bf16[2, 2, 8, 8, 8]/[1024, 512, 64, 8, 1] 16 - - - w16 ptr:f32[11]/[1]:f32 op:f32[2, 11, 9, 10]/[990, 90, 10, 1] 3 addr 512 - - 0.0 - - - - 0',
        'B=2 C1=16 C2=0 Cin=16 Cout=11 H=8 OH=8 OW=8 W=8 add=0 flat=m16 kind=3 pool=False unpool=False',
        'f32[2, 11, 9, 10]/[990, 90, 10, 1] (the out given)',
    ),
    'm16_wide_out_is_slice_0': (
        'conv_c8_m16_kernel 589824.0 iiseg_conv_c8_m16_ws',
        'B=2 C1=16 H=8 W=8 Cout=16 KH=3 KW=3 pad=1 dil=1 OH=8 OW=8 flags=1 out_ctot=32',
        'op:bf16[2, 2, 8, 8, 8]/[1024, 512, 64, 8, 1] 16 - - - w16 ptr:f32[16]/[1]:f32 op:bf16[2, 4, 8, 8, 8]/[2048, 512, 64, 8, 1] 1 addr 512 - - 0.0 - - - - 0',
        'B=2 C1=16 C2=0 Cin=16 Cout=16 H=8 OH=8 OW=8 W=8 add=0 flat=m16 kind=1 pool=False unpool=False',
        'bf16[2, 4, 8, 8, 8]/[2048, 512, 64, 8, 1] (the out given)',
    ),
    'm16_two_chunk_slice_out': (
        'conv_c8_m16_kernel 589824.0 iiseg_conv_c8_m16_ws',
        'B=2 C1=16 H=8 W=8 Cout=16 KH=3 KW=3 pad=1 dil=1 OH=8 OW=8 flags=1 out_ctot=48',
        'op:bf16[2, 2, 8, 8, 8]/[1024, 512, 64, 8, 1] 16 - - - w16 ptr:f32[16]/[1]:f32 op:bf16[2, 2, 8, 8, 8]/[3072, 512, 64, 8, 1] 1 addr 512 - - 0.0 - - - - 0',
        'B=2 C1=16 C2=0 Cin=16 Cout=16 H=8 OH=8 OW=8 W=8 add=0 flat=m16 kind=1 pool=False unpool=False',
        'bf16[2, 2, 8, 8, 8]/[3072, 512, 64, 8, 1] (the out given)',
    ),
    'm16_dense': (
        'conv_c8_m16_kernel 1474560.0 iiseg_conv_c8_m16_ws',
        'B=2 C1=48 H=8 W=8 Cout=16 KH=3 KW=3 pad=1 dil=1 OH=8 OW=8 flags=1 out_ctot=64 out_c0=48',
        'op:bf16[2, 8, 8, 8, 8]/[4096, 512, 64, 8, 1] 64 - ptr:f32[48]/[1]:f32 ptr:f32[48]/[1]:f32 w16 ptr:f32[16]/[1]:f32 op:bf16[2, 8, 8, 8, 8]/[4096, 512, 64, 8, 1] 1 addr 512 - - 0.0 - - - - 0',
        'B=2 C1=48 C2=0 Cin=40 Cout=16 H=8 OH=8 OW=8 W=8 add=0 flat=m16 kind=1 pool=False unpool=False',
        'bf16[2, 8, 8, 8, 8]/[4096, 512, 64, 8, 1] (the out given)',
    ),
    'm16_dense_stats': (
        'conv_c8_m16_kernel 1474560.0 iiseg_conv_c8_m16_ws',
        'B=2 C1=48 H=8 W=8 Cout=16 KH=3 KW=3 pad=1 dil=1 OH=8 OW=8 flags=1 out_ctot=64 out_c0=48',
        'op:bf16[2, 8, 8, 8, 8]/[4096, 512, 64, 8, 1] 64 - ptr:f32[48]/[1]:f32 ptr:f32[48]/[1]:f32 w16 ptr:f32[16]/[1]:f32 op:bf16[2, 8, 8, 8, 8]/[4096, 512, 64, 8, 1] 1 addr 512 ptr:f32[64]/[1]:f32 ptr:f32[64]/[1]:f32 0.0001 - - - - 0',
        'B=2 C1=48 C2=0 Cin=40 Cout=16 H=8 OH=8 OW=8 W=8 add=0 flat=m16 kind=1 pool=False unpool=False',
        'bf16[2, 8, 8, 8, 8]/[4096, 512, 64, 8, 1] (the out given)',
    ),
    'm16_dense_stats_fold': (
        'conv_c8_m16_kernel 1474560.0 iiseg_conv_c8_m16_ws',
        'B=2 C1=48 H=8 W=8 Cout=16 KH=3 KW=3 pad=1 dil=1 OH=8 OW=8 flags=1 out_ctot=64 out_c0=48',
        'op:bf16[2, 8, 8, 8, 8]/[4096, 512, 64, 8, 1] 64 - ptr:f32[48]/[1]:f32 ptr:f32[48]/[1]:f32 w16 ptr:f32[16]/[1]:f32 op:bf16[2, 8, 8, 8, 8]/[4096, 512, 64, 8, 1] 1 addr 512 ptr:f32[64]/[1]:f32 ptr:f32[64]/[1]:f32 0.0001 ptr:f32[64]/[1]:f32 ptr:f32[64]/[1]:f32 ptr:f32[64]/[1]:f32 ptr:f32[64]/[1]:f32 64',
        'B=2 C1=48 C2=0 Cin=40 Cout=16 H=8 OH=8 OW=8 W=8 add=0 flat=m16 kind=1 pool=False unpool=False',
        'bf16[2, 8, 8, 8, 8]/[4096, 512, 64, 8, 1] (the out given)',
    ),
    'm16_workspace': (
        'conv_c8_m16_kernel 18874368.0 iiseg_conv_c8_m16_ws',
        'B=2 C1=512 H=8 W=8 Cout=16 KH=3 KW=3 pad=1 dil=1 OH=8 OW=8 flags=1',
        'op:bf16[2, 64, 8, 8, 8]/[32768, 512, 64, 8, 1] 512 - - - w16 ptr:f32[16]/[1]:f32 op:bf16[2, 2, 8, 8, 8]/[1024, 512, 64, 8, 1] 1 addr 524800 - - 0.0 - - - - 0',
        'B=2 C1=512 C2=0 Cin=512 Cout=16 H=8 OH=8 OW=8 W=8 add=0 flat=m16 kind=1 pool=False unpool=False',
        'bf16[2, 2, 8, 8, 8]/[1024, 512, 64, 8, 1]',
    ),
    'm16_no_workspace': (
        'conv_c8_m16_kernel 589824.0 iiseg_conv_c8_m16_ws',
        'B=2 C1=16 H=8 W=8 Cout=16 KH=3 KW=3 pad=1 dil=1 oy0=4 ox0=4 OH=8 OW=8 flags=1',
        'op:bf16[2, 2, 8, 8, 8]/[1024, 512, 64, 8, 1] 16 - - - w16 ptr:f32[16]/[1]:f32 op:bf16[2, 2, 8, 8, 8]/[1024, 512, 64, 8, 1] 1 - 0 - - 0.0 - - - - 0',
        'B=2 C1=16 C2=0 Cin=16 Cout=16 H=8 OH=8 OW=8 W=8 add=0 flat=m16 kind=1 pool=False unpool=False',
        'bf16[2, 2, 8, 8, 8]/[1024, 512, 64, 8, 1]',
    ),
}

EXPECTED_1X1 = (
    'conv1x1_c8_kernel 112640.0 iiseg_conv1x1_c8', '',
    'addr:None 2 48 64 8 8 ptr:f32[48]/[1]:f32 ptr:f32[48]/[1]:f32 ptr:bf16[8]/[1]:bf16 ptr:f32[11]/[1]:f32 11 0 addr:None 0 0',
    '', 'f32[2, 11, 8, 8]/[704, 64, 8, 1]')


def fmt(x):
    return '%s%s/%s' % (NAMES[x.dtype], list(x.shape), list(x.stride()))


class Token:
    """What a recorder hands back in place of a pointer."""

    def __init__(self, text):
        self.text = text

    def data_ptr(self):
        return WS_ADDR


class Recorder:
    def __init__(self):
        self.launches, self.info, self.pointers = [], [], 0

    def ptr(self, x, dtype=F32):
        self.pointers += 1
        return None if x is None else Token('ptr:%s:%s' % (fmt(x), NAMES[dtype]))

    def operand(self, x):
        self.pointers += 1
        return None if x is None else Token('op:' + fmt(x))

    def workspace(self, kind, n, device):
        self.pointers += 1
        return Token('ws:%s:%d' % (kind, n))

    def weights(self, conv):
        self.pointers += 1
        return Token('w16')

    def arg(self, a):
        if a is None:
            return '-'
        if isinstance(a, Token):
            return a.text
        if isinstance(a, C.c_void_p):
            return 'addr' if a.value == WS_ADDR else 'addr:%s' % a.value
        assert type(a) in (int, float), a
        return repr(a)

    def launch(self, kernel, flops, fn, *args):
        d = args[0]._obj if type(args[0]).__name__ == 'CArgObject' else None
        desc = '' if d is None else \
            ' '.join('%s=%d' % (n, getattr(d, n)) for n, _ in d._fields_ if getattr(d, n))
        self.launches.append(('%s %r %s' % (kernel() if callable(kernel) else kernel, flops, fn.__name__), desc,
                              ' '.join(self.arg(a) for a in args[d is not None:])))

    def row(self, out, given):
        assert len(self.launches) == 1 and len(self.info) <= 1
        info = ' '.join('%s=%s' % (k, str(v).replace(' ', '')) for k, v in sorted(self.info[0].items())) \
            if self.info else ''
        ret = '-' if out is None else fmt(out) + (' (the out given)' if out is given else '')
        return self.launches[0] + (info, ret)


@pytest.fixture
def rec(built_lib, monkeypatch):
    from iterative_inference_segm_amd import ops
    r = Recorder()
    monkeypatch.setattr(ops, '_launch', r.launch)
    monkeypatch.setattr(ops, '_operand', r.operand)
    monkeypatch.setattr(ops, '_ptr', r.ptr)
    monkeypatch.setattr(ops, '_workspace', r.workspace)
    monkeypatch.setattr(ops.Conv, '_c8_weights', lambda conv: r.weights(conv))
    monkeypatch.setattr(ops, 'CONV_PROFILE', [])
    monkeypatch.setattr(ops, 'CONV_PROFILE_INFO', r.info)
    monkeypatch.setattr(ops, 'C8_M16', True)
    return r


def run(rec, case):
    conv, x1, kw = case()
    del rec.launches[:], rec.info[:]
    return rec.row(conv(x1, **kw), kw.get('out'))


@pytest.mark.parametrize('name', sorted(CASES))
def test_every_argument_of_the_launch(rec, name):
    assert run(rec, CASES[name]) == EXPECTED[name]


def test_the_cases_cover_both_kernels_every_flag_and_both_workspace_answers():
    assert set(EXPECTED) == set(CASES)
    heads = {k: v[0].split()[0] for k, v in EXPECTED.items()}
    assert {heads[k] for k in heads if k.startswith('main_')} == {'conv_c8_kernel'}
    assert {heads[k] for k in heads if k.startswith('x3_')} == {'conv_c8_kernel<x3>'}
    assert {heads[k] for k in heads if k.startswith('m16_')} == {'conv_c8_m16_kernel'}
    assert ' addr ' in EXPECTED['m16_workspace'][2] and ' addr ' not in EXPECTED['m16_no_workspace'][2]


@pytest.mark.parametrize('name', sorted(CHOICE))
def test_each_term_of_the_choice_between_the_two_kernels(rec, name):
    case, kernel = CHOICE[name]
    assert run(rec, case)[0].split()[0] == kernel


def test_the_switch_turns_the_16_channel_kernel_off(rec, monkeypatch):
    from iterative_inference_segm_amd import ops
    monkeypatch.setattr(ops, 'C8_M16', False)
    for name in ('eligible', 'eligible_pad0', 'eligible_concat_layer'):
        assert run(rec, CHOICE[name][0])[0].split()[0] == 'conv_c8_kernel'
    with pytest.raises(RuntimeError, match='in_c / bn on C8 input: layers with at most 16'):
        run(rec, CASES['m16_dense'])


@pytest.mark.parametrize('name', sorted(REFUSALS))
def test_refusals_come_before_any_pointer(rec, name):
    match, case = REFUSALS[name]
    conv, x1, kw = case()
    with pytest.raises(RuntimeError, match=match):
        conv(x1, **kw)
    assert rec.pointers == 0 and not rec.launches and not rec.info


def test_nchw_input_refuses_the_c8_only_arguments(rec):
    for kw in (dict(zins=True), dict(in_c=16), dict(bn=(t(16), t(16))), dict(stats=(t(16), t(16), 1e-4)),
               dict(fold=(t(16),) * 4 + (16,))):
        with pytest.raises(RuntimeError, match='C8 input only'):
            layer(16, 16)(t(2, 16, 8, 8), **kw)
    assert rec.pointers == 0


# Conv1x1C8 shares the rule "the first in_c channels of a C8 stack" with the 16-channel kernel
def conv1x1(cin, cout):
    from iterative_inference_segm_amd import ops
    conv = ops.Conv1x1C8(torch.zeros(cout, cin, 1, 1), torch.zeros(cout), device='cpu')
    for n in (16, 32, 48, 64):
        conv._wp[n] = t(8, dtype=BF)                 # (packed already: packing needs a stream)
    return conv


@pytest.mark.parametrize('cin,ch,in_c,text', [
    (16, 32, 24, '24 input channels of 32'), (16, 16, 32, '32 input channels of 16'),
    (40, 64, 32, '32 input channels of 64'), (16, 32, None, '32 input channels of 32')])
def test_conv1x1_c8_in_c_refusals(rec, cin, ch, in_c, text):
    with pytest.raises(RuntimeError, match=r'Conv1x1C8: %s \(layer: %d\)' % (text, cin)):
        conv1x1(cin, 11)(c8(2, ch, 8, 8), in_c=in_c)
    assert rec.pointers == 0 and not rec.launches


def test_conv1x1_c8_launch(rec):
    s = stack64()
    out = conv1x1(40, 11)(s, in_c=48, bn=(t(48), t(48)))
    assert rec.row(out, None) == EXPECTED_1X1
    pooled = c8(2, 64, 4, 4)
    rec.launches.clear()
    assert conv1x1(40, 16)(s, in_c=48, bn=(t(48), t(48)), pool=True, out=pooled, out_c0=32) is pooled
    args = rec.launches[0][2].split()          # (x8 and out go by their addresses: none on meta tensors)
    assert args[1:4] == ['2', '48', '64'] and args[-2:] == ['64', '32']
