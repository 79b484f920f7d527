#!/usr/bin/env python3
"""Training step of the context-module DAE on one GPU: one JSON line.

    python scripts/bench_train.py [--batch 10] [--steps 20] [--warmup 5] [--sizes 224x224 360x480]

Per size and precision (fp32, float64): training images/s (median of `steps` timed steps, warm), ms per step
split into forward / loss / backward-data / weight-gradient / optimizer (sums of the dispatch times of the
library's launches in one profiled step: ops.profile_begin / profile_end), the forward alone from the same run,
and the weight-gradient kernel's fraction of `--hbm_tbs` (default 6.6 TB/s: what refine_update_kernel streams,
DESIGN 3.11) on the byte model (Cin + 2 Cout) B H_in W_in sizeof (x and g_out read, g_z written).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from iterative_inference_segm_amd import ops, synthetic as S        # noqa: E402
from iterative_inference_segm_amd.contextmod import ContextModDAE   # noqa: E402
from iterative_inference_segm_amd.train import DAETrainer           # noqa: E402

GROUPS = {'conv_small_wgrad_kernel': 'weight_gradient', 'ctx_loss_count_kernel': 'loss', 'ctx_loss_kernel': 'loss',
          'opt_step_kernel': 'optimizer'}


def one(B, H, W, dt, steps, warmup, hbm_tbs):
    params = S.make_contextmod_params(11, 3, seed=777)
    dae = ContextModDAE(params, 11, dtype=dt)
    tr = DAETrainer(None, dae, 11, [11], noise=0.1, seed=1)
    X = torch.from_numpy(S.make_images(B, H, W, seed=1)).to(dt).cuda()
    L = torch.from_numpy(S.make_labels(B, H, W, seed=2)).to(dt).cuda().contiguous()
    Y = L[:, :11].contiguous()
    for _ in range(warmup):
        tr.train_step(X, Y, L)
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tr.train_step(X, Y, L)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    fwd = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dae.forward_train([X], Y)
        e1.record()
        e1.synchronize()
        fwd.append(e0.elapsed_time(e1))
    # one profiled step: kernel time per group
    ops.KERNEL_BYTES.clear()
    ops.profile_begin()
    ops.CONV_PROFILE = prof = []
    try:
        n_fwd = None
        score = dae.forward_train([X], Y, noise=0.1, generator=tr.generator)
        n_fwd = len(prof)
        res, g, _ = ops.ctx_loss(score, L, tr.losses, tr.lmb)
        dae.backward(g)
        ops.opt_step(tr.optimizer, dae.flat, dae.gflat, tr.s1, tr.s2, tr.lr, tr.state)
        torch.cuda.synchronize()
    finally:
        ops.CONV_PROFILE = None
        ops.profile_end()
    split = {'forward': 0.0, 'loss': 0.0, 'backward_data': 0.0, 'weight_gradient': 0.0, 'optimizer': 0.0}
    wg = []
    for i, (kernel, _, a, b) in enumerate(prof):
        t = a.elapsed_time(b)
        grp = 'forward' if i < n_fwd else GROUPS.get(kernel, 'backward_data')
        split[grp] += t
        if kernel == 'conv_small_wgrad_kernel':
            wg.append(t)
    wg_bytes = ops.KERNEL_BYTES.get('conv_small_wgrad_kernel', 0.0)
    med = float(np.median(ms))
    return {'size': '%dx%d' % (H, W), 'dtype': str(dt).replace('torch.', ''), 'batch': B,
            'images_per_s': B / med * 1e3, 'step_ms': med, 'step_ms_min': float(np.min(ms)),
            'forward_ms': float(np.median(fwd)), 'step_over_forward': med / float(np.median(fwd)),
            'kernel_ms': {k: round(v, 4) for k, v in split.items()},
            'wgrad_launch_ms': [round(t, 4) for t in wg],
            'wgrad_gbs': wg_bytes / (split['weight_gradient'] * 1e-3) / 1e9 if split['weight_gradient'] else None,
            'wgrad_fraction_of_hbm': (wg_bytes / (split['weight_gradient'] * 1e-3) / (hbm_tbs * 1e12)
                                      if split['weight_gradient'] else None)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=10)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--sizes', nargs='+', default=['224x224', '360x480'])
    ap.add_argument('--dtypes', nargs='+', default=['float32', 'float64'])
    ap.add_argument('--hbm_tbs', type=float, default=6.6)
    a = ap.parse_args()
    rows = []
    for size in a.sizes:
        H, W = (int(v) for v in size.split('x'))
        for name in a.dtypes:
            rows.append(one(a.batch, H, W, getattr(torch, name), a.steps, a.warmup, a.hbm_tbs))
    print(json.dumps({'bench': 'ctx_train', 'device': torch.cuda.get_device_name(0), 'hbm_tbs': a.hbm_tbs,
                      'results': rows}))


if __name__ == '__main__':
    main()
