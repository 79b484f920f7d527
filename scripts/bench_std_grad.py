#!/usr/bin/env python3
"""True-gradient refinement through the standard DAE (BASELINE configs[1]: n_filters 64, h = FCN-8 pool4, two
additional pools, trackind, skip) on one GPU: one JSON line.

    python scripts/bench_std_grad.py [--batches 10 64] [--legs f32 bf16c8] [--steps 10] [--warmup 2] [--size 224x224]

Per batch size and leg ('f32': fp32 NCHW kernels; 'bf16c8': bf16 C8 activations, 16-bit MFMA operands): ms per
gradient-mode step and per residual-mode step of the same engine (both eager, graph=False, no early stop: `steps`
iterations of one refine call, median over `--repeats` calls), their ratio, and one profiled gradient step (dispatch
times of the library's launches: ops.profile_begin / profile_end) split per kernel into forward and backward, with the
backward's launches listed in order.  The yardstick: the backward convolutions run the forward's kernels on the
forward's FLOPs, so a gradient step should cost about twice the leg's own eager residual step plus the element-wise
adjoint kernels at the streaming rate on their byte model (`--hbm_tbs`, default 6.6 TB/s: what refine_update_kernel
streams); `gradient_over_yardstick` says how far it is from that, `backward_launches` which launches
carry the difference.  Host-side gaps (zero fills and crop copies are torch launches, not the library's) are
`step_ms - kernel_ms_sum`."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from iterative_inference_segm_amd import ops, synthetic as S        # noqa: E402
from iterative_inference_segm_amd.api import IterativeInference     # noqa: E402
from iterative_inference_segm_amd.dae import StandardDAE            # noqa: E402
from iterative_inference_segm_amd.fcn8 import FCN8                  # noqa: E402

ELEMENTWISE = ('depool_bwd_c8_kernel', 'relu_gate_c8_kernel')
STEP = 0.05


def _loop_ms(ii, H, Y, mode, steps, repeats):
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ii.refine(H, Y, STEP, steps, mode=mode, graph=False, early_stop=False)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / steps)
    return float(np.median(ms)), float(np.min(ms))


def _by_kernel(entries):
    out = {}
    for kernel, _, a, b in entries:
        out[kernel] = out.get(kernel, 0.0) + a.elapsed_time(b)
    return {k: round(v, 4) for k, v in out.items()}


def one(params, B, H, W, leg, steps, warmup, repeats, hbm_tbs):
    fp, dp = params
    fcn = FCN8(fp, 11, layer=['pool4', 'probs_dimshuffle'], mma=leg)
    dae = StandardDAE(dp, 11, mma=leg)
    ii = IterativeInference(fcn, dae, 11, [11])
    X = torch.from_numpy(S.make_images(B, H, W, seed=1)).float().cuda()
    out = ii.pred_fcn_fn(X)
    Hs, Y = list(out[:-1]), out[-1]
    for mode in ('residual', 'gradient'):
        ii.refine(Hs, Y, STEP, warmup, mode=mode, graph=False, early_stop=False)
    torch.cuda.synchronize()
    res_ms, res_min = _loop_ms(ii, Hs, Y, 'residual', steps, repeats)
    grd_ms, grd_min = _loop_ms(ii, Hs, Y, 'gradient', steps, repeats)
    # one profiled gradient step of a primed session (the steady state of the loop)
    y = Y.clone()
    st = ops.RefineState(B, H, W, y.device)
    sess = dae.new_session(Hs, y, tags=[ii.provenance_of(h) for h in Hs])
    dae.keep_pre = True
    dae.scores(Hs, y, session=sess)
    ops.KERNEL_BYTES.clear()
    ops.profile_begin()
    ops.CONV_PROFILE = prof = []
    try:
        score = dae.scores(Hs, y, session=sess)
        n_fwd, l_fwd = len(prof), ops._lib.load().iiseg_profile_count()
        g = dae.backward_y(ops.sqerr_softmax_bwd(score, y, off=(0, 0)), y.shape)
        n_bwd, l_bwd = len(prof), ops._lib.load().iiseg_profile_count()
        ops.grad_update(score, g, y, st, STEP, off=(0, 0))
        ops.refine_finalize(st, -1.0)
        torch.cuda.synchronize()
    finally:
        ops.CONV_PROFILE = None
        n_all = ops.profile_end()
        dae.keep_pre = False
    ms = ops.PROFILE_MS
    fwd_ms, bwd_ms, upd_ms = float(sum(ms[:l_fwd])), float(sum(ms[l_fwd:l_bwd])), float(sum(ms[l_bwd:n_all]))
    elem_bytes = sum(ops.KERNEL_BYTES.get(k, 0.0) for k in ELEMENTWISE)
    bwd_kernels = _by_kernel(prof[n_fwd:n_bwd])
    rate = {}
    for k in ELEMENTWISE:
        if k in bwd_kernels and bwd_kernels[k] > 0:
            by = ops.KERNEL_BYTES.get(k, 0.0)
            rate[k] = {'bytes': by, 'ms': bwd_kernels[k], 'gbs': by / (bwd_kernels[k] * 1e-3) / 1e9,
                       'fraction_of_hbm': by / (bwd_kernels[k] * 1e-3) / (hbm_tbs * 1e12)}
    yard = 2.0 * res_ms + elem_bytes / (hbm_tbs * 1e12) * 1e3
    return {'size': '%dx%d' % (H, W), 'leg': leg, 'batch': B,
            'gradient_step_ms': grd_ms, 'gradient_step_ms_min': grd_min,
            'residual_step_ms': res_ms, 'residual_step_ms_min': res_min,
            'gradient_over_residual': grd_ms / res_ms,
            'yardstick_ms': yard, 'gradient_over_yardstick': grd_ms / yard,
            'kernel_ms': {'forward': round(fwd_ms, 4), 'backward': round(bwd_ms, 4), 'update': round(upd_ms, 4)},
            'kernel_ms_sum': round(fwd_ms + bwd_ms + upd_ms, 4),
            'library_launches': {'forward': l_fwd, 'backward': l_bwd - l_fwd, 'update': n_all - l_bwd},
            'forward_kernels_ms': _by_kernel(prof[:n_fwd]),
            'backward_kernels_ms': bwd_kernels,
            # (launches outside ops._launch -- layout converters, the fp32 leg's pool adjoints, the softmax backward --
            # are in `kernel_ms` but carry no name here)
            'backward_unnamed_ms': round(bwd_ms - sum(bwd_kernels.values()), 4),
            'backward_launches': [(k, round(a.elapsed_time(b), 4)) for k, _, a, b in prof[n_fwd:n_bwd]],
            'byte_model': rate}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[10, 64])
    ap.add_argument('--legs', nargs='+', default=['f32', 'bf16c8'])
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--size', default='224x224')
    ap.add_argument('--hbm_tbs', type=float, default=6.6)
    a = ap.parse_args()
    H, W = (int(v) for v in a.size.split('x'))
    params = (S.make_fcn8_params(seed=1234), S.make_dae_params(seed=4321))
    rows = []
    for B in a.batches:
        for leg in a.legs:
            rows.append(one(params, B, H, W, leg, a.steps, a.warmup, a.repeats, a.hbm_tbs))
            torch.cuda.empty_cache()
    print(json.dumps({'bench': 'std_grad', 'device': torch.cuda.get_device_name(0), 'hbm_tbs': a.hbm_tbs,
                      'results': rows}))


if __name__ == '__main__':
    main()
