#!/usr/bin/env python3
"""The context-module DAE's 16-bit leg against its fp32 path on one GPU: one JSON line.

    python scripts/bench_ctx_c8.py [--batches 10 64] [--sizes 224x224 360x480] [--steps 20] [--repeats 3]

Per batch size, map size and mode ('f32', 'bf16c8'): ms per residual refinement step of one engine (no early
stop; `steps` iterations of one refine call, median over `--repeats` calls) eager and replayed from the captured
graph, and the kernel time of one profiled DAE forward per launch (dispatch times of the library's launches:
ops.profile_begin / profile_end; the 16-bit leg's strided device copy of y8 into conv1's border, which is not a
launch of the library, is timed with events and listed first).  Then images/s of configs[4](i) -- FCN-8 host,
concat_h=['input'], batch 64 at 224^2, 50 steps, one engine -- with the whole pipeline in either mode."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from iterative_inference_segm_amd import ops, synthetic as S        # noqa: E402
from iterative_inference_segm_amd.api import IterativeInference     # noqa: E402
from iterative_inference_segm_amd.contextmod import ContextModDAE   # noqa: E402
from iterative_inference_segm_amd.fcn8 import FCN8                  # noqa: E402


def _loop_ms(ii, X, Y, steps, repeats, graph):
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ii.refine([X], Y, 0.1, steps, graph=graph, early_stop=False)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / steps)
    return float(np.median(ms))


def one(B, H, W, mma, steps, repeats):
    dae = ContextModDAE(S.make_contextmod_params(11, 3, seed=777), 11, mma=mma)
    ii = IterativeInference(None, dae, 11, [11])
    X = torch.from_numpy(S.make_images(B, H, W, seed=1)).cuda()
    L = torch.from_numpy(S.make_labels(B, H, W, seed=2)).cuda()
    Y = (0.8 * L[:, :11] + 0.2 / 11).contiguous()
    for graph in (False, True):
        ii.refine([X], Y, 0.1, 4, graph=graph, early_stop=False)
    torch.cuda.synchronize()
    eager, replay = _loop_ms(ii, X, Y, steps, repeats, False), _loop_ms(ii, X, Y, steps, repeats, True)
    # one profiled forward inside a session: kernel time per launch
    sess = dae.new_session([X], Y)
    dae.scores([X], Y, session=sess)
    torch.cuda.synchronize()
    ops.profile_begin()
    ops.CONV_PROFILE = prof = []
    try:
        dae.scores([X], Y, session=sess)
        torch.cuda.synchronize()
    finally:
        ops.CONV_PROFILE = None
        ops.profile_end()
    layers = [[kernel, round(a.elapsed_time(b), 4)] for kernel, _, a, b in prof]
    if dae.c8:
        # the 16-bit leg's one launch outside the library: y8 into conv1's zero border, a strided device copy that
        # the dispatch times above do not see -- timed with events over 20 copies
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            sess['y8cat'][:, :, 1:-1, 1:-1].copy_(sess['y8'])
        e1.record()
        e1.synchronize()
        layers.insert(0, ['y8cat_copy', round(e0.elapsed_time(e1) / 20, 4)])
    return {'batch': B, 'size': '%dx%d' % (H, W), 'mma': mma, 'step_ms_eager': round(eager, 4),
            'step_ms_graph': round(replay, 4), 'layer_kernel_ms': layers,
            'layer_kernel_ms_sum': round(sum(t for _, t in layers), 4)}


def config5i(mma, B=64, H=224, W=224, steps=50, batches=3):
    fcn = FCN8(S.make_fcn8_params(seed=1234), 11, layer=['input', 'probs_dimshuffle'], mma=mma)
    dae = ContextModDAE(S.make_contextmod_params(), 11, mma=mma)
    ii = IterativeInference(fcn, dae, 11, [11])
    Xs = [torch.from_numpy(S.make_images(B, H, W, seed=4000 + i)).cuda() for i in range(2)]

    def batch(X):
        out = ii.pred_fcn_fn(X)
        return ii.refine(out[:-1], out[-1], 0.1, steps, early_stop=False)
    batch(Xs[0])
    batch(Xs[1])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(batches):
        batch(Xs[i % 2])
    torch.cuda.synchronize()
    d = (time.perf_counter() - t0) / batches
    return {'mma': mma, 'batch': B, 'size': '%dx%d' % (H, W), 'num_iter': steps, 'in_flight': 1,
            'images_per_s': round(B / d, 2), 'ms_per_batch': round(d * 1e3, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[10, 64])
    ap.add_argument('--sizes', nargs='+', default=['224x224', '360x480'])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--no_config', action='store_true', help='skip the configs[4](i) pipeline')
    a = ap.parse_args()
    rows = []
    for B in a.batches:
        for size in a.sizes:
            H, W = (int(v) for v in size.split('x'))
            for mma in ('f32', 'bf16c8'):
                rows.append(one(B, H, W, mma, a.steps, a.repeats))
                torch.cuda.empty_cache()
    cfg = [] if a.no_config else [config5i('f32'), config5i('bf16c8')]
    print(json.dumps({'bench': 'ctx_c8', 'device': torch.cuda.get_device_name(0), 'results': rows,
                      'configs4_i': cfg}))


if __name__ == '__main__':
    main()
