#!/usr/bin/env python3
"""True-gradient refinement through the context-module DAE on one GPU: one JSON line.

    python scripts/bench_ctx_grad.py [--batch 10] [--steps 20] [--warmup 3] [--sizes 224x224 360x480]

Per size and precision (fp32, float64): ms per gradient-mode step and per residual-mode step of the same engine
(both eager, graph=False, no early stop: `steps` iterations of one refine call, median over `--repeats` calls),
their ratio, the kernel time of one profiled gradient step split into forward / head / masked data gradient /
update (sums of the dispatch times of the library's launches: ops.profile_begin / profile_end), the per-launch
times of the masked data gradient, and the new kernels' rate on their byte model (g_out and out read once, the
window of g_x written) against `--hbm_tbs` (default 6.6 TB/s: what refine_update_kernel streams).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from iterative_inference_segm_amd import ops, synthetic as S        # noqa: E402
from iterative_inference_segm_amd.api import IterativeInference     # noqa: E402
from iterative_inference_segm_amd.contextmod import ContextModDAE   # noqa: E402

GROUPS = {'conv_small_dgrad_kernel': 'data_gradient', 'ctx_grad_head_kernel': 'head'}


def _loop_ms(ii, X, Y, mode, steps, repeats):
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ii.refine([X], Y, 0.05, steps, mode=mode, graph=False, early_stop=False)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / steps)
    return float(np.median(ms)), float(np.min(ms))


def one(B, H, W, dt, steps, warmup, repeats, hbm_tbs):
    params = S.make_contextmod_params(11, 3, seed=777)
    dae = ContextModDAE(params, 11, dtype=dt)
    ii = IterativeInference(None, dae, 11, [11], dtype=dt)
    X = torch.from_numpy(S.make_images(B, H, W, seed=1)).to(dt).cuda()
    L = torch.from_numpy(S.make_labels(B, H, W, seed=2)).to(dt).cuda()
    Y = (0.8 * L[:, :11] + 0.2 / 11).contiguous()
    for mode in ('residual', 'gradient'):
        ii.refine([X], Y, 0.05, warmup, mode=mode, graph=False, early_stop=False)
    torch.cuda.synchronize()
    res_ms, res_min = _loop_ms(ii, X, Y, 'residual', steps, repeats)
    grd_ms, grd_min = _loop_ms(ii, X, Y, 'gradient', steps, repeats)
    # one profiled gradient step: kernel time per group
    y = Y.clone()
    st = ops.RefineState(B, H, W, y.device)
    sess = dae.new_session([X], y)
    dae.keep_pre = True
    ops.KERNEL_BYTES.clear()
    ops.profile_begin()
    ops.CONV_PROFILE = prof = []
    try:
        score = dae.scores([X], y, session=sess)
        n_fwd = len(prof)
        g = dae.sqerr_backward(score, y)
        n_bwd = len(prof)
        ops.grad_update(score, g, y, st, 0.05, off=(0, 0))
        ops.refine_finalize(st, -1.0)
        torch.cuda.synchronize()
    finally:
        ops.CONV_PROFILE = None
        n_all = ops.profile_end()
        dae.keep_pre = False
    split = {'forward': 0.0, 'head': 0.0, 'data_gradient': 0.0}
    dg = []
    for i, (kernel, _, a, b) in enumerate(prof):
        t = a.elapsed_time(b)
        split['forward' if i < n_fwd else GROUPS[kernel]] += t
        if kernel == 'conv_small_dgrad_kernel':
            dg.append(t)
    assert n_bwd - n_fwd == 8                                 # head + dilconv6..1 + conv1: one launch per layer
    # (the copy of y into the concat buffer is a device copy, not a launch of the library; grad_update and
    # refine_finalize are its last two launches)
    split['update'] = float(sum(ops.PROFILE_MS[n_all - 2:n_all]))
    rate = {}
    for kern, grp in GROUPS.items():
        by = ops.KERNEL_BYTES.get(kern, 0.0)
        rate[grp] = {'bytes': by, 'gbs': by / (split[grp] * 1e-3) / 1e9,
                     'fraction_of_hbm': by / (split[grp] * 1e-3) / (hbm_tbs * 1e12)}
    return {'size': '%dx%d' % (H, W), 'dtype': str(dt).replace('torch.', ''), 'batch': B,
            'gradient_step_ms': grd_ms, 'gradient_step_ms_min': grd_min,
            'residual_step_ms': res_ms, 'residual_step_ms_min': res_min,
            'gradient_over_residual': grd_ms / res_ms,
            'kernel_ms': {k: round(v, 4) for k, v in split.items()},
            'kernel_ms_sum': round(sum(split.values()), 4),
            'dgrad_launch_ms': [round(t, 4) for t in dg],           # dilconv6, 5, 4, 3, 2, 1, conv1
            'byte_model': rate}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=10)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--sizes', nargs='+', default=['224x224', '360x480'])
    ap.add_argument('--dtypes', nargs='+', default=['float32', 'float64'])
    ap.add_argument('--hbm_tbs', type=float, default=6.6)
    a = ap.parse_args()
    rows = []
    for size in a.sizes:
        H, W = (int(v) for v in size.split('x'))
        for name in a.dtypes:
            rows.append(one(a.batch, H, W, getattr(torch, name), a.steps, a.warmup, a.repeats, a.hbm_tbs))
    print(json.dumps({'bench': 'ctx_grad', 'device': torch.cuda.get_device_name(0), 'hbm_tbs': a.hbm_tbs,
                      'results': rows}))


if __name__ == '__main__':
    main()
