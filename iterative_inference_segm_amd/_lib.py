"""ctypes binding of libiiseg_hip.so (the C ABI of include/iiseg.h).

There is NO fallback: if the shared library is missing or a symbol is absent, importing a
compute path raises.  The product never routes through the CPU oracle.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, 'libiiseg_hip.so')

ABI_VERSION = 34

CONV_RELU = 1
CONV_UNPOOL = 2
CONV_X3 = 8
CONV_TRANSPOSED2 = 4
CONV_ZINS = 16


class ConvDesc(C.Structure):
    """struct iiseg_conv_desc"""
    _fields_ = [(n, C.c_int32) for n in
                ('B', 'C1', 'C2', 'H', 'W', 'Cout', 'KH', 'KW', 'pad', 'dil',
                 'oy0', 'ox0', 'OH', 'OW', 'AH', 'AW', 'ay0', 'ax0')] + \
               [('flags', C.c_uint32), ('Kpad', C.c_int32), ('Mpad', C.c_int32),
                ('out_ctot', C.c_int32), ('out_c0', C.c_int32),
                ('out_H', C.c_int32), ('out_W', C.c_int32), ('out_y0', C.c_int32),
                ('out_x0', C.c_int32), ('tile_y0', C.c_int32), ('tile_x0', C.c_int32)]


class DeconvDesc(C.Structure):
    """struct iiseg_deconv_desc"""
    _fields_ = [(n, C.c_int32) for n in
                ('B', 'Cin', 'H', 'W', 'Cout', 'K', 'stride', 'oy0', 'ox0', 'OH', 'OW',
                 'AH', 'AW', 'ay0', 'ax0')]


CRF_BILATERAL = 1
CRF_INPUT_0_255 = 2


class CrfDesc(C.Structure):
    """struct iiseg_crf_desc"""
    _fields_ = [(n, C.c_int32) for n in ('B', 'C', 'H', 'W', 'R')] + [('flags', C.c_uint32)] + \
               [(n, C.c_double) for n in ('sxy_g', 'w_g', 'sxy_b', 'srgb', 'w_b', 'clip')]


LOSS_CROSSENTROPY = 1
LOSS_SQUARED_ERROR = 2
OPT_RMSPROP = 0
OPT_ADAM = 1


class WgradDesc(C.Structure):
    """struct iiseg_wgrad_desc"""
    _fields_ = [(n, C.c_int32) for n in ('B', 'Cin', 'Cout', 'H', 'W', 'K', 'dil', 'gz_H', 'gz_W', 'gz_y0',
                                         'gz_x0', 'reserved')] + [('so', C.c_int64), ('sc', C.c_int64)]


class DgradDesc(C.Structure):
    """struct iiseg_dgrad_desc"""
    _fields_ = [(n, C.c_int32) for n in ('B', 'Cin', 'Cout', 'K', 'dil', 'OH', 'OW', 'out_H', 'out_W', 'out_y0',
                                         'out_x0', 'wy0', 'wx0', 'WH', 'WW', 'ci0', 'nci', 'gx_C', 'gx_H', 'gx_W',
                                         'gx_c0', 'gx_y0', 'gx_x0', 'reserved')] + [('so', C.c_int64), ('sc', C.c_int64)]


class ConvWgradDesc(C.Structure):
    """struct iiseg_conv_wgrad_desc"""
    _fields_ = [(n, C.c_int32) for n in ('B', 'Cin', 'Cout', 'H', 'W', 'K', 'pad', 'ci0', 'Cin_tot')] + \
               [('reserved', C.c_int32 * 3), ('so', C.c_int64), ('sc', C.c_int64)]


class ConvDgradDesc(C.Structure):
    """struct iiseg_conv_dgrad_desc"""
    _fields_ = [(n, C.c_int32) for n in ('B', 'Cin', 'Cout', 'H', 'W', 'K', 'pad', 'ci0', 'Cin_tot', 'accumulate')] + \
               [('reserved', C.c_int32 * 2), ('so', C.c_int64), ('sc', C.c_int64)]


class ConvWgradKxKDesc(C.Structure):
    """struct iiseg_conv_wgrad_kxk_desc"""
    _fields_ = [(n, C.c_int32) for n in ('B', 'Cin', 'Cout', 'H', 'W', 'K', 'ci0', 'Cin_tot', 'x_y0', 'x_x0')] + \
               [('reserved', C.c_int32 * 2)] + \
               [(n, C.c_int64) for n in ('x_row', 'x_plane', 'x_image', 'so', 'sc')]


class ConvFwdKxKDesc(C.Structure):
    """struct iiseg_conv_fwd_kxk_desc"""
    _fields_ = [(n, C.c_int32) for n in ('B', 'Cin', 'Cout', 'H', 'W', 'K', 'relu', 'reserved')]


class BnReluConvDesc(C.Structure):
    """struct iiseg_bnrelu_conv_desc"""
    _fields_ = [(n, C.c_int32) for n in ('B', 'n', 'cap', 'Cout', 'H', 'W', 'out_cap', 'out_c0')]


L2_MAX_RANGES = 64
BN_BWD_REDUCE, BN_BWD_APPLY = 1, 2       # iiseg_bn_relu_bwd_*'s stages

C8DIL_OUT_NCHW = 0x100


class C8DilDesc(C.Structure):
    """struct iiseg_c8dil_desc"""
    _fields_ = [(n, C.c_int32) for n in ('B', 'Cin', 'Cout', 'H', 'W', 'K', 'dil', 'out_H', 'out_W', 'out_y0',
                                         'out_x0')] + [('flags', C.c_uint32)]


_vp, _i32, _i64, _f32, _f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double

# name -> (restype, argtypes); mirrors include/iiseg.h one to one
SIGNATURES = {
    'iiseg_strerror': (C.c_char_p, [C.c_int]),
    'iiseg_last_hip_error': (C.c_char_p, []),
    'iiseg_abi_version': (C.c_int, []),
    'iiseg_profile_begin': (C.c_int, [C.c_int]),
    'iiseg_profile_count': (C.c_int, []),
    'iiseg_profile_end': (C.c_int, [C.POINTER(C.c_float), C.c_int]),
    'iiseg_target_arch': (C.c_char_p, []),
    'iiseg_conv_ktab_entries': (C.c_int, [C.POINTER(ConvDesc)]),
    'iiseg_conv_plan': (C.c_int, [C.POINTER(ConvDesc)]),
    'iiseg_conv_pack_f32': (C.c_int, [_vp, C.POINTER(ConvDesc), _vp, _i64, _i64, _vp, _vp]),
    'iiseg_conv_f32': (C.c_int, [_vp, C.POINTER(ConvDesc)] + [_vp] * 9),
    'iiseg_conv_small_supported': (C.c_int, [C.POINTER(ConvDesc)]),
    'iiseg_conv_pool_supported': (C.c_int, [C.POINTER(ConvDesc)]),
    'iiseg_conv_direct_kernel': (C.c_int, [C.POINTER(ConvDesc), C.c_int, C.c_int, C.POINTER(C.c_int32)]),
    'iiseg_conv_pool_f32': (C.c_int, [_vp, C.POINTER(ConvDesc)] + [_vp] * 10),
    'iiseg_conv_halo_seam': (C.c_int, [C.c_int]),
    'iiseg_conv_halo_seam_launches': (_i64, []),
    'iiseg_conv_mask_supported': (C.c_int, [C.POINTER(ConvDesc)]),
    'iiseg_conv_mask_f32': (C.c_int, [_vp, C.POINTER(ConvDesc)] + [_vp] * 12),
    'iiseg_conv_bnrelu_supported': (C.c_int, [C.POINTER(ConvDesc)]),
    'iiseg_conv_bnrelu_f32': (C.c_int, [_vp, C.POINTER(ConvDesc), _vp, _i64] + [_vp] * 8),
    'iiseg_conv_wino_supported': (C.c_int, [C.POINTER(ConvDesc)]),
    'iiseg_conv_wino_weight_elems': (_i64, [C.POINTER(ConvDesc)]),
    'iiseg_conv_wino_workspace_elems': (_i64, [C.POINTER(ConvDesc)]),
    'iiseg_conv_wino_pack_f32': (C.c_int, [_vp, C.POINTER(ConvDesc), _vp, _i64, _i64, _vp]),
    'iiseg_conv_wino_f32': (C.c_int, [_vp, C.POINTER(ConvDesc)] + [_vp] * 9 + [C.c_uint32]),
    'iiseg_conv_wino_pool_supported': (C.c_int, [C.POINTER(ConvDesc)]),
    'iiseg_conv_wino_input_wide': (C.c_int, [C.c_int]),
    'iiseg_conv_wino_input_path': (C.c_int, [C.POINTER(ConvDesc), C.c_int]),
    'iiseg_conv_wino_m_quad': (C.c_int, [C.c_int]),
    'iiseg_conv_wino_gemm_slim': (C.c_int, [C.c_int]),
    'iiseg_conv_wino_input_narrow': (C.c_int, [C.c_int]),
    'iiseg_conv_wino_input_tiles': (C.c_int, [C.POINTER(ConvDesc), C.c_int]),
    'iiseg_conv_wino_mask_f32': (C.c_int, [_vp, C.POINTER(ConvDesc)] + [_vp] * 12 + [C.c_uint32]),
    'iiseg_conv_wino_bf16_supported': (C.c_int, [C.POINTER(ConvDesc)]),
    'iiseg_conv_wino_bf16_weight_bytes': (_i64, [C.POINTER(ConvDesc)]),
    'iiseg_conv_wino_bf16_workspace_bytes': (_i64, [C.POINTER(ConvDesc)]),
    'iiseg_conv_wino_bf16_pack': (C.c_int, [_vp, C.POINTER(ConvDesc), _vp, _i64, _i64, _vp]),
    'iiseg_conv_wino_bf16': (C.c_int, [_vp, C.POINTER(ConvDesc)] + [_vp] * 9 + [C.c_uint32]),
    'iiseg_conv_gemm_bf16_supported': (C.c_int, [C.POINTER(ConvDesc)]),
    'iiseg_conv_gemm_bf16_weight_bytes': (_i64, [C.POINTER(ConvDesc)]),
    'iiseg_conv_gemm_bf16_workspace_bytes': (_i64, [C.POINTER(ConvDesc)]),
    'iiseg_conv_gemm_bf16_pack': (C.c_int, [_vp, C.POINTER(ConvDesc), _vp, _i64, _i64, _vp]),
    'iiseg_conv_gemm_bf16': (C.c_int, [_vp, C.POINTER(ConvDesc)] + [_vp] * 5),
    'iiseg_conv_halo_bf16_supported': (C.c_int, [C.POINTER(ConvDesc)]),
    'iiseg_conv_halo_bf16_weight_bytes': (_i64, [C.POINTER(ConvDesc)]),
    'iiseg_conv_halo_bf16_pack': (C.c_int, [_vp, C.POINTER(ConvDesc), _vp, _i64, _i64, _vp]),
    'iiseg_conv_halo_bf16': (C.c_int, [_vp, C.POINTER(ConvDesc)] + [_vp] * 11),
    'iiseg_conv_halo_bf16_fwd_check': (C.c_int, [C.POINTER(ConvDesc)]),
    'iiseg_conv_halo_bf16_fwd_weight_bytes': (_i64, [C.POINTER(ConvDesc)]),
    'iiseg_conv_halo_bf16_fwd_pack': (C.c_int, [_vp, C.POINTER(ConvDesc), _vp, _i64, _i64, _vp]),
    'iiseg_conv_halo_bf16_fwd': (C.c_int, [_vp, C.POINTER(ConvDesc)] + [_vp] * 11),
    'iiseg_conv_wino_f64_supported': (C.c_int, [C.POINTER(ConvDesc)]),
    'iiseg_conv_wino_f64_weight_elems': (_i64, [C.POINTER(ConvDesc)]),
    'iiseg_conv_wino_f64_workspace_elems': (_i64, [C.POINTER(ConvDesc)]),
    'iiseg_conv_wino_pack_f64': (C.c_int, [_vp, C.POINTER(ConvDesc), _vp, _i64, _i64, _vp]),
    'iiseg_conv_wino_f64': (C.c_int, [_vp, C.POINTER(ConvDesc)] + [_vp] * 9),
    'iiseg_conv_c8_supported': (C.c_int, [C.POINTER(ConvDesc)]),
    'iiseg_conv_c8_is_flat': (C.c_int, [C.POINTER(ConvDesc)]),
    'iiseg_conv_c8_force_tiling': (C.c_int, [C.c_int, C.c_int, C.c_int]),
    'iiseg_conv_c8_tiling': (C.c_int, [C.POINTER(ConvDesc), C.c_int, C.POINTER(C.c_int32)]),
    'iiseg_conv_c8': (C.c_int, [_vp, C.POINTER(ConvDesc)] + [_vp] * 6 + [_i32, _vp, _i32, _vp, _vp]),
    'iiseg_conv_c8_slice': (C.c_int, [_vp, C.POINTER(ConvDesc), _vp, _i32] + [_vp] * 5 + [_i32, _vp, _i32, _vp, _vp]),
    'iiseg_unpool_c8': (C.c_int, [_vp] * 4 + [C.c_int] * 7),
    'iiseg_depool_bwd_c8': (C.c_int, [_vp] * 5 + [C.c_int] * 10),
    'iiseg_relu_gate_c8': (C.c_int, [_vp] * 4 + [C.c_int] * 8),
    'iiseg_conv_c8_m16_supported': (C.c_int, [C.POINTER(ConvDesc)]),
    'iiseg_conv_c8_m16': (C.c_int, [_vp, C.POINTER(ConvDesc), _vp, _i32] + [_vp] * 6 + [_i32]),
    'iiseg_conv_c8_m16_workspace_bytes': (_i64, [C.POINTER(ConvDesc)]),
    'iiseg_conv_c8_m16_ws': (C.c_int, [_vp, C.POINTER(ConvDesc), _vp, _i32] + [_vp] * 6 + [_i32, _vp, _i64, _vp, _vp, _f64] + [_vp] * 4 + [_i32]),
    'iiseg_conv1x1_c8_weight_bytes': (_i64, [C.c_int, C.c_int]),
    'iiseg_conv1x1_c8_pack': (C.c_int, [_vp, _vp, _i64, _i64, C.c_int, C.c_int, C.c_int, _vp]),
    'iiseg_conv1x1_c8': (C.c_int, [_vp, _vp] + [C.c_int] * 5 + [_vp] * 4 + [C.c_int, C.c_int, _vp, C.c_int, C.c_int]),
    'iiseg_bn_fold_f32': (C.c_int, [_vp] * 7 + [_i32]),
    'iiseg_bn_stats_c8_workspace_elems': (C.c_int64, [_i32]),
    'iiseg_bn_stats_c8': (C.c_int, [_vp, _vp] + [_i32] * 6 + [C.c_double, _vp, _vp, _vp]),
    'iiseg_nchw_to_c8_slice': (C.c_int, [_vp, _vp, _vp] + [_i32] * 6),
    'iiseg_c8_slice_to_nchw': (C.c_int, [_vp, _vp, _vp] + [_i32] * 6),
    'iiseg_nchw_to_c8': (C.c_int, [_vp, _vp, _vp] + [_i32] * 5),
    'iiseg_c8_to_nchw': (C.c_int, [_vp, _vp, _vp] + [_i32] * 5),
    'iiseg_pool_mask_c8': (C.c_int, [_vp, _vp, _i32, _vp, _vp] + [_i32] * 11),
    'iiseg_conv_c8_split_weights': (C.c_int, [_vp, _vp, _i64, _i64, _i32, _i32, _vp]),
    'iiseg_nchw_to_c8x3': (C.c_int, [_vp, _vp, _vp] + [_i32] * 5),
    'iiseg_c8x3_to_nchw': (C.c_int, [_vp, _vp, _vp] + [_i32] * 5),
    'iiseg_pool_mask_c8x3': (C.c_int, [_vp, _vp, _vp, _vp] + [_i32] * 12),
    'iiseg_conv_gemm_supported': (C.c_int, [C.POINTER(ConvDesc)]),
    'iiseg_conv_gemm_workspace_elems': (_i64, [C.POINTER(ConvDesc)]),
    'iiseg_conv_gemm_f32': (C.c_int, [_vp, C.POINTER(ConvDesc)] + [_vp] * 5 + [C.c_uint32]),
    'iiseg_maxpool2x2_f32': (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32]),
    'iiseg_unpool_eqmask_f32': (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32]),
    'iiseg_maxpool2x2_window_f32': (C.c_int, [_vp] * 3 + [_i32] * 7),
    'iiseg_maxpool2x2_window_f64': (C.c_int, [_vp] * 3 + [_i32] * 7),
    'iiseg_maxpool2x2_mask_window_f32': (C.c_int, [_vp] * 4 + [_i32] * 7),
    'iiseg_unpool_eqmask_window_f32': (C.c_int, [_vp] * 5 + [_i32] * 7),
    'iiseg_unpool_eqmask_window_f64': (C.c_int, [_vp] * 5 + [_i32] * 7),
    'iiseg_deconv_f32': (C.c_int, [_vp, C.POINTER(DeconvDesc)] + [_vp] * 5),
    'iiseg_deconv_phase_supported': (C.c_int, [C.POINTER(DeconvDesc), C.c_int, C.c_int]),
    'iiseg_deconv_phase_weight_elems': (C.c_int64, [C.POINTER(DeconvDesc)]),
    'iiseg_deconv_phase_pack_f32': (C.c_int, [_vp, C.POINTER(DeconvDesc), _vp, _vp]),
    'iiseg_deconv_phase_pack_f64': (C.c_int, [_vp, C.POINTER(DeconvDesc), _vp, _vp]),
    'iiseg_deconv_phase_f32': (C.c_int, [_vp, C.POINTER(DeconvDesc)] + [_vp] * 5),
    'iiseg_deconv_phase_f64': (C.c_int, [_vp, C.POINTER(DeconvDesc)] + [_vp] * 5),
    'iiseg_crop_softmax_f32': (C.c_int, [_vp, _vp, _vp, _vp] + [_i32] * 8),
    'iiseg_refine_partials': (C.c_int, [_i32, _i32]),
    'iiseg_refine_update_f32': (C.c_int, [_vp] * 5 + [_i32] * 8 + [_f32]),
    'iiseg_refine_update_c8_f32': (C.c_int, [_vp] * 6 + [_i32] * 9 + [_f32]),
    'iiseg_refine_finalize': (C.c_int, [_vp] * 5 + [_i32] * 3 + [_f64]),
    'iiseg_ctx_tail_partials': (C.c_int, [_i32, _i32]),
    'iiseg_ctx_tail_f32': (C.c_int, [_vp] * 3 + [_i32] + [_vp] * 2 + [_i32] + [_vp] * 5 + [_i32] * 10 + [_f32]),
    'iiseg_confusion_f32': (C.c_int, [_vp] * 5 + [_i32] * 3),
    'iiseg_confusion_masked_f32': (C.c_int, [_vp] * 6 + [_i32] * 3),
    'iiseg_confusion_masked_f64': (C.c_int, [_vp] * 6 + [_i32] * 3),
    'iiseg_bn_stats_workspace_elems': (_i64, [_i32]),
    'iiseg_bn_stats_f32': (C.c_int, [_vp, _vp, _i64, _i32, _i32, _i32, _f32, _vp, _vp, _vp]),
    'iiseg_bn_relu_f32': (C.c_int, [_vp, _vp, _i64, _i32, _i32, _i32] + [_vp] * 5),
    'iiseg_bn_stats_f64': (C.c_int, [_vp, _vp, _i64, _i32, _i32, _i32, _f64, _vp, _vp, _vp]),
    'iiseg_bn_relu_f64': (C.c_int, [_vp, _vp, _i64, _i32, _i32, _i32] + [_vp] * 5),
    'iiseg_bn_relu_bwd_workspace_elems': (_i64, [_i32, _i32]),
    'iiseg_bn_relu_bwd_f32': (C.c_int, [_vp, _vp, _i64, _vp, _vp, _i32, _i32, _i32] + [_vp] * 7 + [_i32]),
    'iiseg_bn_relu_bwd_f64': (C.c_int, [_vp, _vp, _i64, _vp, _vp, _i32, _i32, _i32] + [_vp] * 7 + [_i32]),
    'iiseg_maxpool2x2_bwd_f32': (C.c_int, [_vp] * 5 + [_i32] * 3),
    'iiseg_maxpool2x2_bwd_f64': (C.c_int, [_vp] * 5 + [_i32] * 3),
    'iiseg_sqerr_softmax_bwd_f32': (C.c_int, [_vp] * 4 + [_i32] * 8),
    'iiseg_sqerr_softmax_bwd_f64': (C.c_int, [_vp] * 4 + [_i32] * 8),
    'iiseg_depool_bwd_f32': (C.c_int, [_vp] * 5 + [_i32] * 3),
    'iiseg_depool_bwd_f64': (C.c_int, [_vp] * 5 + [_i32] * 3),
    'iiseg_pool_relu_bwd_f32': (C.c_int, [_vp] * 5 + [_i32] * 3),
    'iiseg_pool_relu_bwd_f64': (C.c_int, [_vp] * 5 + [_i32] * 3),
    'iiseg_grad_update_f32': (C.c_int, [_vp] * 6 + [_i32] * 8 + [C.c_float]),
    'iiseg_grad_update_f64': (C.c_int, [_vp] * 6 + [_i32] * 8 + [C.c_double]),
    'iiseg_add_noise_f32': (C.c_int, [_vp, _vp, _vp, C.c_float, _vp, _i64]),
    'iiseg_add_noise_f64': (C.c_int, [_vp, _vp, _vp, C.c_double, _vp, _i64]),
    'iiseg_dropout_apply_f32': (C.c_int, [_vp, _vp, _vp, C.c_float, _i64]),
    'iiseg_dropout_apply_f64': (C.c_int, [_vp, _vp, _vp, C.c_double, _i64]),
    'iiseg_bn_affine_window_f32': (C.c_int, [_vp, _vp] + [_i32] * 8 + [_vp] * 4),
    'iiseg_bn_affine_window_f64': (C.c_int, [_vp, _vp] + [_i32] * 8 + [_vp] * 4),
    # float64 (strict-parity) variants
    'iiseg_conv_plan_f64': (C.c_int, [C.POINTER(ConvDesc)]),
    'iiseg_conv_pack_f64': (C.c_int, [_vp, C.POINTER(ConvDesc), _vp, _i64, _i64, _vp]),
    'iiseg_conv_f64': (C.c_int, [_vp, C.POINTER(ConvDesc)] + [_vp] * 8),
    'iiseg_conv_halo_f64_supported': (C.c_int, [C.POINTER(ConvDesc)]),
    'iiseg_conv_pool_f64_supported': (C.c_int, [C.POINTER(ConvDesc)]),
    'iiseg_conv_pool_f64': (C.c_int, [_vp, C.POINTER(ConvDesc)] + [_vp] * 9),
    'iiseg_conv_mask_f64_supported': (C.c_int, [C.POINTER(ConvDesc)]),
    'iiseg_conv_mask_f64': (C.c_int, [_vp, C.POINTER(ConvDesc)] + [_vp] * 11),
    'iiseg_conv_gemm_f64_supported': (C.c_int, [C.POINTER(ConvDesc)]),
    'iiseg_conv_gemm_f64_workspace_elems': (_i64, [C.POINTER(ConvDesc)]),
    'iiseg_conv_gemm_f64': (C.c_int, [_vp, C.POINTER(ConvDesc)] + [_vp] * 5),
    'iiseg_im2col_f64': (C.c_int, [_vp, _vp, _vp] + [_i32] * 6),
    'iiseg_maxpool2x2_f64': (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32]),
    'iiseg_unpool_eqmask_f64': (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32]),
    'iiseg_deconv_f64': (C.c_int, [_vp, C.POINTER(DeconvDesc)] + [_vp] * 5),
    'iiseg_crop_softmax_f64': (C.c_int, [_vp, _vp, _vp, _vp] + [_i32] * 8),
    'iiseg_refine_update_f64': (C.c_int, [_vp] * 5 + [_i32] * 8 + [_f64]),
    'iiseg_confusion_f64': (C.c_int, [_vp] * 5 + [_i32] * 3),
    'iiseg_count_nonfinite_f32': (C.c_int, [_vp, _vp, _i64, _vp]),
    'iiseg_count_nonfinite_f64': (C.c_int, [_vp, _vp, _i64, _vp]),
    # dense-CRF mean field
    'iiseg_crf_supported': (C.c_int, [C.POINTER(CrfDesc)]),
    'iiseg_crf_prepare_f32': (C.c_int, [_vp, C.POINTER(CrfDesc)] + [_vp] * 7),
    'iiseg_crf_prepare_f64': (C.c_int, [_vp, C.POINTER(CrfDesc)] + [_vp] * 7),
    'iiseg_crf_step_f32': (C.c_int, [_vp, C.POINTER(CrfDesc)] + [_vp] * 6),
    'iiseg_crf_step_f64': (C.c_int, [_vp, C.POINTER(CrfDesc)] + [_vp] * 6),
    # training the context-module DAE
    'iiseg_ctx_loss_partials': (C.c_int, [_i32] * 3),
    'iiseg_ctx_loss_count_f32': (C.c_int, [_vp] * 4 + [_i32] * 4),
    'iiseg_ctx_loss_count_f64': (C.c_int, [_vp] * 4 + [_i32] * 4),
    'iiseg_ctx_loss_f32': (C.c_int, [_vp] * 7 + [_i32] * 4 + [C.c_uint32, _f64]),
    'iiseg_ctx_loss_f64': (C.c_int, [_vp] * 7 + [_i32] * 4 + [C.c_uint32, _f64]),
    'iiseg_conv_small_wgrad_partials': (C.c_int, [C.POINTER(WgradDesc), _i32]),
    'iiseg_conv_small_wgrad_f32': (C.c_int, [_vp, C.POINTER(WgradDesc)] + [_vp] * 7),
    'iiseg_conv_small_wgrad_f64': (C.c_int, [_vp, C.POINTER(WgradDesc)] + [_vp] * 7),
    'iiseg_opt_step_f32': (C.c_int, [_vp, _i32] + [_vp] * 6 + [_i64]),
    'iiseg_opt_step_f64': (C.c_int, [_vp, _i32] + [_vp] * 6 + [_i64]),
    # true-gradient refinement through the context-module DAE
    'iiseg_conv_small_dgrad_blocks': (C.c_int, [C.POINTER(DgradDesc)]),
    'iiseg_conv_small_dgrad_f32': (C.c_int, [_vp, C.POINTER(DgradDesc)] + [_vp] * 4),
    'iiseg_conv_small_dgrad_f64': (C.c_int, [_vp, C.POINTER(DgradDesc)] + [_vp] * 4),
    'iiseg_ctx_grad_head_blocks': (C.c_int, [_i32] * 5),
    'iiseg_ctx_grad_head_f32': (C.c_int, [_vp] * 5 + [_i64] * 2 + [_vp] * 2 + [_i32] * 5),
    'iiseg_ctx_grad_head_f64': (C.c_int, [_vp] * 5 + [_i64] * 2 + [_vp] * 2 + [_i32] * 5),
    # 16-bit leg of the context-module DAE
    'iiseg_conv_c8_dil_check': (C.c_int, [C.POINTER(C8DilDesc)]),
    'iiseg_conv_c8_dil_pack_bytes': (_i64, [_i32]),
    'iiseg_conv_c8_dil_pack_host': (C.c_int, [C.POINTER(C8DilDesc), _vp, _i64, _i64, _vp]),
    'iiseg_conv_c8_dil_pack': (C.c_int, [_vp, C.POINTER(C8DilDesc), _vp, _i64, _i64, _vp]),
    'iiseg_conv_c8_dil': (C.c_int, [_vp, C.POINTER(C8DilDesc)] + [_vp] * 5),
    # training the standard DAE
    'iiseg_conv_wgrad_check': (C.c_int, [C.POINTER(ConvWgradDesc)]),
    'iiseg_conv_wgrad_slabs': (C.c_int, [C.POINTER(ConvWgradDesc), _i32]),
    'iiseg_conv_wgrad_workspace_elems': (_i64, [C.POINTER(ConvWgradDesc), _i32]),
    'iiseg_conv_wgrad_f32': (C.c_int, [_vp, C.POINTER(ConvWgradDesc)] + [_vp] * 5),
    'iiseg_conv_wgrad_f64': (C.c_int, [_vp, C.POINTER(ConvWgradDesc)] + [_vp] * 5),
    'iiseg_opt_step_grid_f32': (C.c_int, [_vp, _i32] + [_vp] * 6 + [_i64]),
    'iiseg_opt_step_grid_f64': (C.c_int, [_vp, _i32] + [_vp] * 6 + [_i64]),
    # training FCN-8
    'iiseg_conv_wgrad_kxk_check': (C.c_int, [C.POINTER(ConvWgradKxKDesc)]),
    'iiseg_conv_wgrad_kxk_slabs': (C.c_int, [C.POINTER(ConvWgradKxKDesc), _i32]),
    'iiseg_conv_wgrad_kxk_workspace_elems': (_i64, [C.POINTER(ConvWgradKxKDesc), _i32]),
    'iiseg_conv_wgrad_kxk_f32': (C.c_int, [_vp, C.POINTER(ConvWgradKxKDesc)] + [_vp] * 5),
    'iiseg_conv_wgrad_kxk_f64': (C.c_int, [_vp, C.POINTER(ConvWgradKxKDesc)] + [_vp] * 5),
    'iiseg_deconv_dgrad_f32': (C.c_int, [_vp, C.POINTER(DeconvDesc)] + [_vp] * 3),
    'iiseg_deconv_dgrad_f64': (C.c_int, [_vp, C.POINTER(DeconvDesc)] + [_vp] * 3),
    'iiseg_deconv_wgrad_partials': (C.c_int, [C.POINTER(DeconvDesc)]),
    'iiseg_deconv_wgrad_f32': (C.c_int, [_vp, C.POINTER(DeconvDesc)] + [_vp] * 5),
    'iiseg_deconv_wgrad_f64': (C.c_int, [_vp, C.POINTER(DeconvDesc)] + [_vp] * 5),
    # ... of the K = 3 stride-2 layers on the 16-bit matrix pipe (deconv='bf16')
    'iiseg_deconv_grad_bf16_check': (C.c_int, [C.POINTER(DeconvDesc)]),
    'iiseg_deconv_wgrad_bf16_slabs': (C.c_int, [C.POINTER(DeconvDesc)]),
    'iiseg_deconv_wgrad_bf16_workspace_elems': (_i64, [C.POINTER(DeconvDesc)]),
    'iiseg_deconv_dgrad_bf16_workspace_elems': (_i64, [C.POINTER(DeconvDesc)]),
    'iiseg_deconv_wgrad_bf16': (C.c_int, [_vp, C.POINTER(DeconvDesc)] + [_vp] * 5),
    'iiseg_deconv_dgrad_bf16': (C.c_int, [_vp, C.POINTER(DeconvDesc)] + [_vp] * 4),
    'iiseg_relu_gate_f32': (C.c_int, [_vp] * 4 + [_i64]),
    'iiseg_relu_gate_f64': (C.c_int, [_vp] * 4 + [_i64]),
    'iiseg_l2_term_partials': (C.c_int, [_i32]),
    'iiseg_l2_term_f32': (C.c_int, [_vp] * 3 + [_i64, C.POINTER(_i64), _i32, _f64, _vp, _vp]),
    'iiseg_l2_term_f64': (C.c_int, [_vp] * 3 + [_i64, C.POINTER(_i64), _i32, _f64, _vp, _vp]),
    # weight gradients on the 16-bit matrix pipe (wgrad='bf16')
    'iiseg_conv_wgrad_bf16_slabs': (C.c_int, [C.POINTER(ConvWgradDesc)]),
    'iiseg_conv_wgrad_bf16_workspace_elems': (_i64, [C.POINTER(ConvWgradDesc)]),
    'iiseg_conv_wgrad_bf16': (C.c_int, [_vp, C.POINTER(ConvWgradDesc)] + [_vp] * 5),
    # ... in blocks of 16 output channels (co_block=16)
    'iiseg_conv_wgrad_bf16_co16_slabs': (C.c_int, [C.POINTER(ConvWgradDesc)]),
    'iiseg_conv_wgrad_bf16_co16_workspace_elems': (_i64, [C.POINTER(ConvWgradDesc)]),
    'iiseg_conv_wgrad_bf16_co16': (C.c_int, [_vp, C.POINTER(ConvWgradDesc)] + [_vp] * 5),
    # db alone, as iiseg_conv_wgrad_f32 forms it
    'iiseg_conv_wgrad_db_workspace_elems': (_i64, [C.POINTER(ConvWgradDesc)]),
    'iiseg_conv_wgrad_db_f32': (C.c_int, [_vp, C.POINTER(ConvWgradDesc)] + [_vp] * 3),
    # data gradients on the 16-bit matrix pipe (dgrad='bf16')
    'iiseg_conv_dgrad_bf16_check': (C.c_int, [C.POINTER(ConvDgradDesc)]),
    'iiseg_conv_dgrad_bf16_pack_elems': (_i64, [C.POINTER(ConvDgradDesc)]),
    'iiseg_conv_dgrad_bf16_pack': (C.c_int, [_vp, C.POINTER(ConvDgradDesc)] + [_vp] * 2),
    'iiseg_conv_dgrad_bf16': (C.c_int, [_vp, C.POINTER(ConvDgradDesc)] + [_vp] * 4),
    'iiseg_conv_wgrad_kxk_bf16_check': (C.c_int, [C.POINTER(ConvWgradKxKDesc)]),
    'iiseg_conv_wgrad_kxk_bf16_slabs': (C.c_int, [C.POINTER(ConvWgradKxKDesc)]),
    'iiseg_conv_wgrad_kxk_bf16_workspace_elems': (_i64, [C.POINTER(ConvWgradKxKDesc)]),
    'iiseg_conv_wgrad_kxk_bf16': (C.c_int, [_vp, C.POINTER(ConvWgradKxKDesc)] + [_vp] * 5),
    'iiseg_conv_dgrad_kxk_bf16_check': (C.c_int, [C.POINTER(ConvDgradDesc)]),
    'iiseg_conv_dgrad_kxk_bf16_slabs': (C.c_int, [C.POINTER(ConvDgradDesc)]),
    'iiseg_conv_dgrad_kxk_bf16_workspace_elems': (_i64, [C.POINTER(ConvDgradDesc)]),
    'iiseg_conv_dgrad_kxk_bf16_pack_elems': (_i64, [C.POINTER(ConvDgradDesc)]),
    'iiseg_conv_dgrad_kxk_bf16_pack': (C.c_int, [_vp, C.POINTER(ConvDgradDesc)] + [_vp] * 2),
    'iiseg_conv_dgrad_kxk_bf16': (C.c_int, [_vp, C.POINTER(ConvDgradDesc)] + [_vp] * 5),
    'iiseg_conv_fwd_kxk_bf16_check': (C.c_int, [C.POINTER(ConvFwdKxKDesc)]),
    'iiseg_conv_fwd_kxk_bf16_slabs': (C.c_int, [C.POINTER(ConvFwdKxKDesc)]),
    'iiseg_conv_fwd_kxk_bf16_workspace_elems': (_i64, [C.POINTER(ConvFwdKxKDesc)]),
    'iiseg_conv_fwd_kxk_bf16': (C.c_int, [_vp, C.POINTER(ConvFwdKxKDesc)] + [_vp] * 5),
    # FC-DenseNet's dense-block layer, BatchNorm + ReLU + 3x3 + bias + dropout mask in one launch (fwd='bf16')
    'iiseg_bnrelu_conv_fwd_bf16_check': (C.c_int, [C.POINTER(BnReluConvDesc)]),
    'iiseg_bnrelu_conv_fwd_bf16_slabs': (C.c_int, [C.POINTER(BnReluConvDesc)]),
    'iiseg_bnrelu_conv_fwd_bf16_workspace_elems': (_i64, [C.POINTER(BnReluConvDesc)]),
    'iiseg_bnrelu_conv_fwd_bf16': (C.c_int, [_vp, C.POINTER(BnReluConvDesc)] + [_vp] * 8 + [C.c_float] + [_vp] * 2),
}

_lib = None


def load():
    """Load the HIP library (once).  Raises RuntimeError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            'libiiseg_hip.so is missing (%s). Build it with '
            '`python -m iterative_inference_segm_amd.build`; there is no CPU fallback.' % LIB_PATH)
    # torch first: the library shares torch's HIP runtime (streams and device pointers cross the
    # boundary).  Loaded before torch it brought up a runtime of its own, whose first launch on a GPU
    # box said "no ROCm-capable device is detected" (__graft_entry__.build() followed by smoke()).
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.iiseg_abi_version() != ABI_VERSION:
        raise RuntimeError('libiiseg_hip.so ABI %d != binding ABI %d; rebuild'
                           % (lib.iiseg_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(status, what):
    if status != 0:
        msg = load().iiseg_strerror(status).decode()
        if status == -4:                       # IISEG_ERR_LAUNCH: say what the HIP runtime said
            msg += ': ' + load().iiseg_last_hip_error().decode()
        raise RuntimeError('%s failed: %s (iiseg_status %d)' % (what, msg, status))
