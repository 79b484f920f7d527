"""CPU: which kernel FORM ops.Conv chooses for a launch (describe + choose, no GPU, no launch).

The tables below were read off a profiled step of the commit BEFORE the dispatch was split into
describe / choose / run (bench workload, BASELINE configs[1]: FCN-8 + the 64-filter DAE, layer=['pool4'],
224x224, pad 100; float32 and bf16 at batch 64, float64 at batch 32): for every conv layer the first launch
of the step -- its operands' shapes and keyword arguments -- and the form whose kernels that launch ran.
Every other launch of a layer in that step ran the same form."""
import pytest
import torch

N_CLASSES = 11

# (layer, x1's shape, the call's keyword arguments with tensors given as shapes, form)
F32 = [
    ('convs.conv1_1', (64, 3, 224, 224), dict(anchor=(98, 98), window=(98, 98, 226, 226), out=(64, 64, 422, 422),
         place=(98, 98)), 'direct'),
    ('convs.conv1_2', (64, 64, 422, 422), dict(anchor=(97, 97), window=(96, 96, 230, 230), out=(64, 64, 422, 422),
         place=(96, 96), pool_out=(64, 64, 211, 211)), 'pool_f32'),
    ('convs.conv2_1', (64, 64, 211, 211), dict(anchor=(47, 47), window=(47, 47, 117, 117), out=(64, 128, 211,
         211), place=(47, 47)), 'direct'),
    ('convs.conv2_2', (64, 128, 211, 211), dict(anchor=(46, 46), window=(46, 46, 120, 120), out=(64, 128, 211,
         211), place=(46, 46), pool_out=(64, 128, 105, 105)), 'wino_f32'),
    ('convs.conv3_1', (64, 128, 105, 105), dict(anchor=(22, 22), window=(22, 22, 62, 62), out=(64, 256, 105, 105),
         place=(22, 22)), 'wino_f32'),
    ('convs.conv3_2', (64, 256, 105, 105), dict(anchor=(21, 21), window=(21, 21, 64, 64), out=(64, 256, 105, 105),
         place=(21, 21)), 'wino_f32'),
    ('convs.conv3_3', (64, 256, 105, 105), dict(anchor=(20, 20), window=(20, 20, 66, 66), out=(64, 256, 105, 105),
         place=(20, 20), pool_out=(64, 256, 52, 52)), 'wino_f32'),
    ('convs.conv4_1', (64, 256, 52, 52), dict(anchor=(9, 9), window=(9, 9, 35, 35), out=(64, 512, 52, 52),
         place=(9, 9)), 'wino_f32'),
    ('convs.conv4_2', (64, 512, 52, 52), dict(anchor=(8, 8), window=(8, 8, 37, 37), out=(64, 512, 52, 52),
         place=(8, 8)), 'wino_f32'),
    ('convs.conv4_3', (64, 512, 52, 52), dict(anchor=(7, 7), window=(7, 7, 39, 39), out=(64, 512, 52, 52),
         place=(7, 7)), 'wino_f32'),
    ('convs.conv5_1', (64, 512, 26, 26), dict(anchor=(2, 2), window=(2, 2, 22, 22), out=(64, 512, 26, 26),
         place=(2, 2)), 'wino_f32'),
    ('convs.conv5_2', (64, 512, 26, 26), dict(anchor=(1, 1), window=(1, 1, 24, 24), out=(64, 512, 26, 26),
         place=(1, 1)), 'wino_f32'),
    ('convs.conv5_3', (64, 512, 26, 26), dict(anchor=(0, 0), window=(0, 0, 26, 26), out=(64, 512, 26, 26),
         place=(0, 0), pool_out=(64, 512, 13, 13)), 'wino_f32'),
    ('convs.fc6', (64, 512, 13, 13), dict(), 'gemm_f32'),
    ('convs.fc7', (64, 4096, 7, 7), dict(), 'gemm_f32'),
    ('convs.score_fr', (64, 4096, 7, 7), dict(), 'gemm_f32'),
    ('convs.score_pool4', (64, 512, 26, 26), dict(window=(5, 5, 16, 16)), 'direct'),
    ('convs.score_pool3', (64, 256, 52, 52), dict(window=(9, 9, 34, 34)), 'direct'),
    ('enc.conv1_1', (64, 11, 224, 224), dict(anchor=(98, 98), window=(98, 98, 226, 226), out=(64, 64, 422, 422),
         place=(98, 98), pool_out=(64, 64, 211, 211), mask_out=(64, 64, 211, 211), store_out=False), 'mask_f32'),
    ('enc.conv2_1', (64, 64, 211, 211), dict(anchor=(48, 48), window=(48, 48, 116, 116), out=(64, 128, 211, 211),
         place=(48, 48), pool_out=(64, 128, 105, 105), mask_out=(64, 128, 105, 105), store_out=False),
         'mask_f32'),
    ('enc.conv3_1', (64, 128, 105, 105), dict(anchor=(23, 23), window=(23, 23, 60, 60), out=(64, 256, 105, 105),
         place=(23, 23)), 'wino_f32'),
    ('enc.conv4_1', (64, 256, 52, 52), dict(anchor=(10, 10), window=(10, 10, 34, 34), out=(64, 512, 52, 52),
         place=(10, 10), pool_out=(64, 512, 26, 26), mask_out=(64, 512, 26, 26), store_out=False), 'wino_f32'),
    ('hsplit.conv5_1[0]', (64, 512, 26, 26), dict(window=(2, 2, 22, 22), out=(64, 1024, 26, 26), place=(2, 2)),
         'wino_f32'),
    ('hsplit.conv5_1[1]', (64, 512, 26, 26), dict(anchor=(4, 4), window=(2, 2, 22, 22), out=(64, 1024, 26, 26),
         place=(2, 2), pool_out=(64, 1024, 13, 13), add=(64, 1024, 26, 26), add_off=(2, 2), mask_out=(64, 1024,
         13, 13), store_out=False), 'wino_f32'),
    ('enc.conv6_1', (64, 1024, 13, 13), dict(anchor=(1, 1), window=(0, 0, 13, 13), out=(64, 2048, 13, 13),
         place=(0, 0)), 'wino_f32'),
    ('dec.up_conv6', (64, 2048, 6, 6), dict(window=(2, 2, 10, 10), out=(64, 1024, 13, 13), place=(2, 2),
         anchor=(2, 2), mask_in=(64, 2048, 6, 6), unpool_hw=(13, 13), add=(64, 1024, 13, 13), add_off=(2, 2)),
         'wino_f32'),
    ('dec.up_conv5', (64, 1024, 13, 13), dict(window=(5, 5, 17, 17), out=(64, 512, 26, 26), place=(5, 5),
         anchor=(5, 5), mask_in=(64, 1024, 13, 13), unpool_hw=(26, 26), add=(64, 512, 26, 26), add_off=(5, 5)),
         'wino_f32'),
    ('dec.up_conv4', (64, 512, 26, 26), dict(window=(11, 11, 31, 31), out=(64, 256, 52, 52), place=(11, 11),
         anchor=(11, 11), mask_in=(64, 512, 26, 26), unpool_hw=(52, 52), add=(64, 256, 52, 52), add_off=(11, 11)),
         'wino_f32'),
    ('dec.up_conv3', (64, 256, 52, 52), dict(window=(24, 24, 58, 58), out=(64, 128, 105, 105), place=(24, 24),
         anchor=(24, 24), mask_in=(64, 256, 52, 52), unpool_hw=(105, 105), add=(64, 128, 105, 105), add_off=(24,
         24)), 'wino_f32'),
    ('dec.up_conv2', (64, 128, 105, 105), dict(window=(49, 49, 113, 113), out=(64, 64, 211, 211), place=(49, 49),
         anchor=(49, 49), mask_in=(64, 128, 105, 105), unpool_hw=(211, 211), add=(64, 64, 211, 211), add_off=(49,
         49)), 'mask_f32'),
    ('dec.up_conv1', (64, 64, 211, 211), dict(window=(99, 99, 224, 224), anchor=(99, 99), mask_in=(64, 64, 211,
         211), unpool_hw=(422, 422)), 'mask_f32'),
]
F64 = [
    ('convs.conv1_1', (32, 3, 224, 224), dict(anchor=(98, 98), window=(98, 98, 226, 226), out=(32, 64, 422, 422),
         place=(98, 98)), 'direct'),
    ('convs.conv1_2', (32, 64, 422, 422), dict(anchor=(97, 97), window=(96, 96, 230, 230), out=(32, 64, 422, 422),
         place=(96, 96), pool_out=(32, 64, 211, 211)), 'pool_f64'),
    ('convs.conv2_1', (32, 64, 211, 211), dict(anchor=(47, 47), window=(47, 47, 117, 117), out=(32, 128, 211,
         211), place=(47, 47)), 'direct'),
    ('convs.conv2_2', (32, 128, 211, 211), dict(anchor=(46, 46), window=(46, 46, 119, 119), out=(32, 128, 211,
         211), place=(46, 46)), 'wino_f64'),
    ('convs.conv3_1', (32, 128, 105, 105), dict(anchor=(22, 22), window=(22, 22, 62, 62), out=(32, 256, 105, 105),
         place=(22, 22)), 'wino_f64'),
    ('convs.conv3_2', (32, 256, 105, 105), dict(anchor=(21, 21), window=(21, 21, 64, 64), out=(32, 256, 105, 105),
         place=(21, 21)), 'wino_f64'),
    ('convs.conv3_3', (32, 256, 105, 105), dict(anchor=(20, 20), window=(20, 20, 66, 66), out=(32, 256, 105, 105),
         place=(20, 20)), 'wino_f64'),
    ('convs.conv4_1', (32, 256, 52, 52), dict(anchor=(9, 9), window=(9, 9, 35, 35), out=(32, 512, 52, 52),
         place=(9, 9)), 'wino_f64'),
    ('convs.conv4_2', (32, 512, 52, 52), dict(anchor=(8, 8), window=(8, 8, 37, 37), out=(32, 512, 52, 52),
         place=(8, 8)), 'wino_f64'),
    ('convs.conv4_3', (32, 512, 52, 52), dict(anchor=(7, 7), window=(7, 7, 39, 39), out=(32, 512, 52, 52),
         place=(7, 7)), 'wino_f64'),
    ('convs.conv5_1', (32, 512, 26, 26), dict(anchor=(2, 2), window=(2, 2, 22, 22), out=(32, 512, 26, 26),
         place=(2, 2)), 'wino_f64'),
    ('convs.conv5_2', (32, 512, 26, 26), dict(anchor=(1, 1), window=(1, 1, 24, 24), out=(32, 512, 26, 26),
         place=(1, 1)), 'wino_f64'),
    ('convs.conv5_3', (32, 512, 26, 26), dict(anchor=(0, 0), window=(0, 0, 26, 26), out=(32, 512, 26, 26),
         place=(0, 0)), 'wino_f64'),
    ('convs.fc6', (32, 512, 13, 13), dict(), 'gemm_f64'),
    ('convs.fc7', (32, 4096, 7, 7), dict(), 'gemm_f64'),
    ('convs.score_fr', (32, 4096, 7, 7), dict(), 'gemm_f64'),
    ('convs.score_pool4', (32, 512, 26, 26), dict(window=(5, 5, 16, 16)), 'direct'),
    ('convs.score_pool3', (32, 256, 52, 52), dict(window=(9, 9, 34, 34)), 'direct'),
    ('enc.conv1_1', (32, 11, 224, 224), dict(anchor=(98, 98), window=(98, 98, 226, 226), out=(32, 64, 422, 422),
         place=(98, 98), pool_out=(32, 64, 211, 211), mask_out=(32, 64, 211, 211), store_out=False), 'mask_f64'),
    ('enc.conv2_1', (32, 64, 211, 211), dict(anchor=(48, 48), window=(48, 48, 116, 116), out=(32, 128, 211, 211),
         place=(48, 48), pool_out=(32, 128, 105, 105), mask_out=(32, 128, 105, 105), store_out=False),
         'mask_f64'),
    ('enc.conv3_1', (32, 128, 105, 105), dict(anchor=(23, 23), window=(23, 23, 60, 60), out=(32, 256, 105, 105),
         place=(23, 23)), 'wino_f64'),
    ('enc.conv4_1', (32, 256, 52, 52), dict(anchor=(10, 10), window=(10, 10, 33, 33), out=(32, 512, 52, 52),
         place=(10, 10)), 'wino_f64'),
    ('enc.conv5_1', (32, 512, 26, 26), dict(x2=(32, 512, 26, 26), anchor=(4, 4), window=(2, 2, 22, 22), out=(32,
         1024, 26, 26), place=(2, 2)), 'wino_f64'),
    ('enc.conv6_1', (32, 1024, 13, 13), dict(anchor=(1, 1), window=(0, 0, 13, 13), out=(32, 2048, 13, 13),
         place=(0, 0)), 'wino_f64'),
    ('dec.up_conv6', (32, 2048, 6, 6), dict(pre=(32, 2048, 13, 13), pooled=(32, 2048, 6, 6), window=(2, 2, 10,
         10), out=(32, 1024, 13, 13), place=(2, 2), anchor=(2, 2), add=(32, 1024, 13, 13), add_off=(2, 2)),
         'wino_f64'),
    ('dec.up_conv5', (32, 1024, 13, 13), dict(pre=(32, 1024, 26, 26), pooled=(32, 1024, 13, 13), window=(5, 5, 17,
         17), out=(32, 512, 26, 26), place=(5, 5), anchor=(5, 5), add=(32, 512, 26, 26), add_off=(5, 5)),
         'wino_f64'),
    ('dec.up_conv4', (32, 512, 26, 26), dict(pre=(32, 512, 52, 52), pooled=(32, 512, 26, 26), window=(11, 11, 31,
         31), out=(32, 256, 52, 52), place=(11, 11), anchor=(11, 11), add=(32, 256, 52, 52), add_off=(11, 11)),
         'wino_f64'),
    ('dec.up_conv3', (32, 256, 52, 52), dict(pre=(32, 256, 105, 105), pooled=(32, 256, 52, 52), window=(24, 24,
         58, 58), out=(32, 128, 105, 105), place=(24, 24), anchor=(24, 24), add=(32, 128, 105, 105), add_off=(24,
         24)), 'wino_f64'),
    ('dec.up_conv2', (32, 128, 105, 105), dict(window=(49, 49, 113, 113), out=(32, 64, 211, 211), place=(49, 49),
         anchor=(49, 49), mask_in=(32, 128, 105, 105), unpool_hw=(211, 211), add=(32, 64, 211, 211), add_off=(49,
         49)), 'mask_f64'),
    ('dec.up_conv1', (32, 64, 211, 211), dict(window=(99, 99, 224, 224), anchor=(99, 99), mask_in=(32, 64, 211,
         211), unpool_hw=(422, 422)), 'mask_f64'),
]
BF16 = [
    ('convs.conv1_1', (64, 3, 224, 224), dict(anchor=(98, 98), window=(98, 98, 226, 226), out=(64, 64, 422, 422),
         place=(98, 98)), 'halo_bf16'),
    ('convs.conv1_2', (64, 64, 422, 422), dict(anchor=(97, 97), window=(96, 96, 230, 230), out=(64, 64, 422, 422),
         place=(96, 96), pool_out=(64, 64, 211, 211)), 'halo_bf16'),
    ('convs.conv2_1', (64, 64, 211, 211), dict(anchor=(47, 47), window=(47, 47, 117, 117), out=(64, 128, 211,
         211), place=(47, 47)), 'halo_bf16'),
    ('convs.conv2_2', (64, 128, 211, 211), dict(anchor=(46, 46), window=(46, 46, 120, 120), out=(64, 128, 211,
         211), place=(46, 46), pool_out=(64, 128, 105, 105)), 'halo_bf16'),
    ('convs.conv3_1', (64, 128, 105, 105), dict(anchor=(22, 22), window=(22, 22, 62, 62), out=(64, 256, 105, 105),
         place=(22, 22)), 'halo_bf16'),
    ('convs.conv3_2', (64, 256, 105, 105), dict(anchor=(21, 21), window=(21, 21, 64, 64), out=(64, 256, 105, 105),
         place=(21, 21)), 'halo_bf16'),
    ('convs.conv3_3', (64, 256, 105, 105), dict(anchor=(20, 20), window=(20, 20, 66, 66), out=(64, 256, 105, 105),
         place=(20, 20)), 'wino_bf16'),
    ('convs.conv4_1', (64, 256, 52, 52), dict(anchor=(9, 9), window=(9, 9, 35, 35), out=(64, 512, 52, 52),
         place=(9, 9)), 'wino_bf16'),
    ('convs.conv4_2', (64, 512, 52, 52), dict(anchor=(8, 8), window=(8, 8, 37, 37), out=(64, 512, 52, 52),
         place=(8, 8)), 'wino_bf16'),
    ('convs.conv4_3', (64, 512, 52, 52), dict(anchor=(7, 7), window=(7, 7, 39, 39), out=(64, 512, 52, 52),
         place=(7, 7)), 'wino_bf16'),
    ('convs.conv5_1', (64, 512, 26, 26), dict(anchor=(2, 2), window=(2, 2, 22, 22), out=(64, 512, 26, 26),
         place=(2, 2)), 'wino_bf16'),
    ('convs.conv5_2', (64, 512, 26, 26), dict(anchor=(1, 1), window=(1, 1, 24, 24), out=(64, 512, 26, 26),
         place=(1, 1)), 'halo_bf16'),
    ('convs.conv5_3', (64, 512, 26, 26), dict(anchor=(0, 0), window=(0, 0, 26, 26), out=(64, 512, 26, 26),
         place=(0, 0)), 'halo_bf16'),
    ('convs.fc6', (64, 512, 13, 13), dict(), 'gemm_bf16'),
    ('convs.fc7', (64, 4096, 7, 7), dict(), 'gemm_bf16'),
    ('convs.score_fr', (64, 4096, 7, 7), dict(), 'gemm_bf16'),
    ('convs.score_pool4', (64, 512, 26, 26), dict(window=(5, 5, 16, 16)), 'direct'),
    ('convs.score_pool3', (64, 256, 52, 52), dict(window=(9, 9, 34, 34)), 'direct'),
    ('enc.conv1_1', (64, 11, 224, 224), dict(anchor=(98, 98), window=(98, 98, 226, 226), out=(64, 64, 422, 422),
         place=(98, 98), pool_out=(64, 64, 211, 211), mask_out=(64, 64, 211, 211), store_out=False), 'halo_bf16'),
    ('enc.conv2_1', (64, 64, 211, 211), dict(anchor=(48, 48), window=(48, 48, 116, 116), out=(64, 128, 211, 211),
         place=(48, 48), pool_out=(64, 128, 105, 105), mask_out=(64, 128, 105, 105), store_out=False),
         'halo_bf16'),
    ('enc.conv3_1', (64, 128, 105, 105), dict(anchor=(23, 23), window=(22, 22, 62, 62), out=(64, 256, 105, 105),
         place=(22, 22), pool_out=(64, 256, 52, 52)), 'halo_bf16'),
    ('enc.conv4_1', (64, 256, 52, 52), dict(anchor=(10, 10), window=(10, 10, 33, 33), out=(64, 512, 52, 52),
         place=(10, 10)), 'wino_bf16'),
    ('hsplit.conv5_1[0]', (64, 512, 26, 26), dict(window=(2, 2, 22, 22), out=(64, 1024, 26, 26), place=(2, 2)),
         'wino_bf16'),
    ('hsplit.conv5_1[1]', (64, 512, 26, 26), dict(anchor=(4, 4), window=(2, 2, 22, 22), out=(64, 1024, 26, 26),
         place=(2, 2), add=(64, 1024, 26, 26), add_off=(2, 2)), 'wino_bf16'),
    ('enc.conv6_1', (64, 1024, 13, 13), dict(anchor=(1, 1), window=(0, 0, 13, 13), out=(64, 2048, 13, 13),
         place=(0, 0)), 'wino_bf16'),
    ('dec.up_conv6', (64, 2048, 6, 6), dict(pre=(64, 2048, 13, 13), pooled=(64, 2048, 6, 6), window=(2, 2, 10,
         10), out=(64, 1024, 13, 13), place=(2, 2), anchor=(2, 2), add=(64, 1024, 13, 13), add_off=(2, 2)),
         'wino_bf16'),
    ('dec.up_conv5', (64, 1024, 13, 13), dict(pre=(64, 1024, 26, 26), pooled=(64, 1024, 13, 13), window=(5, 5, 17,
         17), out=(64, 512, 26, 26), place=(5, 5), anchor=(5, 5), add=(64, 512, 26, 26), add_off=(5, 5)),
         'wino_bf16'),
    ('dec.up_conv4', (64, 512, 26, 26), dict(pre=(64, 512, 52, 52), pooled=(64, 512, 26, 26), window=(11, 11, 31,
         31), out=(64, 256, 52, 52), place=(11, 11), anchor=(11, 11), add=(64, 256, 52, 52), add_off=(11, 11)),
         'halo_bf16'),
    ('dec.up_conv3', (64, 256, 52, 52), dict(pre=(64, 256, 105, 105), pooled=(64, 256, 52, 52), window=(24, 24,
         58, 58), out=(64, 128, 105, 105), place=(24, 24), anchor=(24, 24), add=(64, 128, 105, 105), add_off=(24,
         24)), 'halo_bf16'),
    ('dec.up_conv2', (64, 128, 105, 105), dict(window=(49, 49, 113, 113), out=(64, 64, 211, 211), place=(49, 49),
         anchor=(49, 49), mask_in=(64, 128, 105, 105), unpool_hw=(211, 211), add=(64, 64, 211, 211), add_off=(49,
         49)), 'halo_bf16'),
    ('dec.up_conv1', (64, 64, 211, 211), dict(window=(99, 99, 224, 224), anchor=(99, 99), mask_in=(64, 64, 211,
         211), unpool_hw=(422, 422)), 'halo_bf16'),
]


TABLES = {'f32': (torch.float32, 'f32', F32), 'f64': (torch.float64, None, F64), 'bf16': (torch.float32, 'bf16', BF16)}
TENSORS = ('x2', 'pre', 'pooled', 'add', 'out', 'pool_out', 'mask_in', 'mask_out')


@pytest.fixture(scope='module')
def params(built_lib):
    from iterative_inference_segm_amd import synthetic as S
    return S.make_fcn8_params(seed=1234), S.make_dae_params(seed=4321)


@pytest.fixture(scope='module', params=sorted(TABLES))
def model(request, params):
    """{layer name: Conv} of the headline model in one mode, built on the host, and that mode's table."""
    from iterative_inference_segm_amd.dae import StandardDAE
    from iterative_inference_segm_amd.fcn8 import FCN8
    dtype, mma, table = TABLES[request.param]
    fcn = FCN8(params[0], N_CLASSES, layer=['pool4', 'probs_dimshuffle'], device='cpu', dtype=dtype, mma=mma)
    dae = StandardDAE(params[1], N_CLASSES, concat_h=['pool4'], padding=100, n_filters=64, additional_pool=2,
                      skip=True, unpool_type='trackind', device='cpu', dtype=dtype, mma=mma)
    layers = {}
    for attr, convs in (('convs', fcn.convs), ('enc', dae.enc), ('dec', dae.dec), ('hsplit', dae.hsplit)):
        for name, v in convs.items():
            if isinstance(v, tuple):
                layers.update(('%s.%s[%d]' % (attr, name, j), c) for j, c in enumerate(v))
            else:
                layers['%s.%s' % (attr, name)] = v
    return request.param, layers, table


def _launch(conv, x1, **kw):
    """The described launch of conv(x1, **kw), tensors given as shapes (meta tensors: no storage)."""
    meta = lambda k, shape: torch.empty(shape, device='meta',
                                        dtype=torch.uint8 if k.startswith('mask') else conv.dtype)
    kw = {k: meta(k, v) if k in TENSORS else v for k, v in kw.items()}
    return conv._describe_call(meta('x1', x1), **kw)


def _form(conv, x1, **kw):
    return conv._form(_launch(conv, x1, **kw))


def _full_map(kw):
    """The same call on the whole map: no window, no placement; a skip-add from its corner."""
    kw = {k: v for k, v in kw.items() if k not in ('window', 'place', 'out', 'add_off')}
    return kw


def test_every_layer_of_the_headline_model_takes_the_form_it_ran(model):
    mode, layers, table = model
    names = {name for name, _, _, _ in table}
    # (every conv layer of the model; float32 runs conv5_1 as its h / y halves, `hsplit`)
    assert names <= set(layers) and set(layers) - names <= {'enc.conv5_1'} and len(table) >= 30
    got = {name: _form(layers[name], x1, **kw) for name, x1, kw, _ in table}
    assert got == {name: form for name, _, _, form in table}
    if mode == 'bf16':
        return      # (the choice between the two 16-bit forms goes by the launch's own width: DESIGN 3.4)
    # float32 / float64: the form does not depend on the window -- the whole map takes it too
    full = {name: _form(layers[name], x1, **_full_map(kw)) for name, x1, kw, _ in table}
    assert full == got


def test_a_window_launch_takes_the_form_of_the_full_map(model):
    """`Conv._form_by_full_map`: a Winograd layer's interior windows run the form of its whole map, at
    either tile anchor -- also where the whole map is too large for the Winograd workspace and a window
    alone would fit."""
    mode, layers, table = model
    wino = [(name, x1) for name, x1, kw, form in table if form in ('wino_f32', 'wino_f64')]
    assert len(wino) >= 15 or mode == 'bf16'
    for name, (B, C1, H, W) in wino:
        conv = layers[name]
        if conv.Cin != C1:
            continue                 # (DePool2D / concat inputs: covered by the table test)
        for batch in (B, 64 * B):
            full = _form(conv, (batch, C1, H, W))
            fh, fw = conv.out_hw(H, W)
            for win in ((1, 1, fh - 2, fw - 2), (2, 3, fh // 2, fw // 3), (fh // 2, fw // 2, 2, 2)):
                for anchor in ((0, 0), (1, 1)):
                    out = (batch, conv.Cout, fh, fw)
                    assert _form(conv, (batch, C1, H, W), window=win, anchor=anchor, out=out,
                                 place=win[:2]) == full, (name, batch, win, anchor)
    if mode != 'bf16':
        # the size limit bites somewhere in this sweep, or the second batch size proves nothing
        big = [_form(layers[n], (64 * s[0],) + s[1:]) for n, s in wino if layers[n].Cin == s[1]]
        assert 'direct' in big


def test_planner_promises_are_kept_by_the_chooser(model):
    """pool_fusable / mask_ok true: a pooled / masked launch of the layer at a legal window gets a form
    that has the pool / the mask bytes.  False and called anyway: masks are refused (RuntimeError); a pool
    is refused or runs on a form that has it, never silently dropped."""
    from iterative_inference_segm_amd.ops import Conv
    mode, layers, table = model
    for name, (B, C1, H, W), kw, _ in table:
        conv = layers[name]
        if 'mask_in' in kw or 'pre' in kw:
            H, W = kw['unpool_hw'] if 'mask_in' in kw else kw['pre'][2:]
        if 'x2' in kw or conv.Cin != C1:
            continue
        fh, fw = conv.out_hw(H, W)
        pooled = (B, conv.Cout, fh // 2, fw // 2)
        for anchor in ((0, 0), (1, 1)):
            for region in (None, (3, 5, 4, 6)):
                win = conv.pool_window(H, W, region, c8=False, anchor=anchor)
                call = dict(anchor=anchor, pool_out=pooled)
                if region is not None:
                    w = win or (2, 4, 6, 8)
                    call.update(window=w, out=(B, conv.Cout, fh, fw), place=w[:2])
                if conv.pool_fusable(False, anchor):
                    assert win is not None and _form(conv, (B, C1, H, W), **call) in Conv.POOL_FORMS
                    if conv.mask_ok(False):
                        assert _form(conv, (B, C1, H, W), mask_out=pooled, **call) in Conv.MASK_FORMS
                else:
                    assert win is None
                    try:
                        assert _form(conv, (B, C1, H, W), **call) in Conv.POOL_FORMS
                    except RuntimeError:
                        pass
        up = dict(mask_in=(B, C1, H // 2, W // 2), unpool_hw=(H, W))
        if conv.mask_ok(False):
            assert _form(conv, (B, C1, H // 2, W // 2), **up) in Conv.MASK_FORMS
        else:
            with pytest.raises(RuntimeError):
                _form(conv, (B, C1, H // 2, W // 2), **up)
