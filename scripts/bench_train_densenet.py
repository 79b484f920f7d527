#!/usr/bin/env python3
"""One training step of FC-DenseNet103 (11 classes, default synthetic weights) on 224x224 crops: one JSON line.

    python scripts/bench_train_densenet.py [--batches 3 10] [--size 224x224] [--reps 5] [--dtypes float32 float64]

Per (precision, batch): step ms (median of `reps` warm steps between two HIP events: forward, loss, backward, L2 term,
RMSprop, refresh) and images/s; then, from the dispatch times of ONE more step run under the library's launch
profile, the time split per kernel name (launches, ms, share of the profiled launch time; kernels that do not pass
the launch profile -- bn_stats, bn_relu, the pool, the optimizer's plumbing -- are the rest up to the step), and
  * per resolution, for the two launches of ops.bn_relu_bwd: their ms summed over the layers
    of that resolution, their byte model (reduce: 2 n planes; apply: 4 n planes) over `--stream_gbs` (6600), and --
    for the widest consumer of that resolution -- their ms next to the forward ops.bn_relu launch of the same layer
    (five back-to-back launches between two HIP events on the step's own stack).  Yardstick, not asserted: 6 n
    planes against 2 n, about 3 x if both stream;
  * for the Cout = growth weight gradients of the dense-block layers (conv_wgrad_kernel): their summed nominal
    2 Cin Cout 9 OH OW B over their summed ms as a fraction of `--peak_tflops` (157.3: the fp32 matrix-pipe peak).
Reads nothing outside the repository.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from iterative_inference_segm_amd import ops, synthetic as S               # noqa: E402
from iterative_inference_segm_amd.densenet import FCDenseNet, layer_plan    # noqa: E402
from iterative_inference_segm_amd.train import DenseNetTrainer              # noqa: E402


def timed(fn, n=5):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def one(B, H, W, dt, reps, peak, stream, weight_decay):
    params = S.make_densenet_params(layer_plan(), seed=2024)
    net = FCDenseNet(params, 11, layer=[], dtype=dt, mma='f32', trainable=True)
    tr = DenseNetTrainer(net, 11, [11], learning_rate=1e-3, weight_decay=weight_decay, seed=1)
    X = torch.from_numpy(S.make_images(B, H, W, seed=2)).to(dt).cuda().contiguous()
    T = torch.from_numpy(S.make_labels(B, H, W, n_classes=11, seed=3)).to(dt).cuda().contiguous()
    for _ in range(2):
        tr.train_step(X, T)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tr.train_step(X, T)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    step = float(np.median(ms))
    peak_mem = torch.cuda.max_memory_allocated()
    # one profiled step: every `_launch` of the library between two marks, in launch order
    prof = []
    ops.KERNEL_BYTES.clear()
    ops.profile_begin()
    ops.CONV_PROFILE = prof
    try:
        score = net.forward_train(X, generator=tr.generator)
        n_fwd = len(prof)
        _, g, _ = ops.ctx_loss(score, T, ('crossentropy',), 1.0)
        net.backward(g)
        for chunk in tr.ranges:
            ops.l2_term(net.flat, net.gflat, chunk, weight_decay)
        torch.cuda.synchronize()
    finally:
        ops.CONV_PROFILE = None
        ops.profile_end()
    rows = [(k, f, a.elapsed_time(b)) for k, f, a, b in prof]
    all_ms = float(sum(t for _, _, t in rows))
    split = {}
    for i, (k, f, t) in enumerate(rows):
        k = ('forward ' if i < n_fwd else '') + k
        e = split.setdefault(k, [0, 0.0])
        e[0] += 1
        e[1] += t
    kernels = [{'kernel': k, 'launches': c, 'ms': round(t, 3), 'share_of_profiled': round(t / all_ms, 4)}
               for k, (c, t) in sorted(split.items(), key=lambda kv: -kv[1][1])]
    # the BatchNorm backward launches, in backward's order: one (reduce, apply) pair per 'brc' / 'td' layer
    back = rows[n_fwd:]
    red = [t for k, _, t in back if k == 'bn_relu_bwd_reduce_kernel']
    app = [t for k, _, t in back if k == 'bn_relu_bwd_apply_kernel']
    consumers = [e for e in reversed(net._steps) if e['kind'] in ('brc', 'td')]
    if not len(red) == len(app) == len(consumers):
        raise RuntimeError('expected one bn_relu_bwd pair per BatchNorm layer, got %d / %d for %d'
                           % (len(red), len(app), len(consumers)))
    sv = net._tsaved
    item = X.element_size()
    by_res = {}
    for e, tr_, ta in zip(consumers, red, app):
        st = sv['stacks'][e['sid']]
        hw = tuple(st.buf.shape[2:])
        planes = float(item) * B * e['n'] * hw[0] * hw[1]
        r = by_res.setdefault(hw, dict(layers=0, reduce_ms=0.0, apply_ms=0.0, reduce_bytes=0.0, apply_bytes=0.0,
                                       widest=None))
        r['layers'] += 1
        r['reduce_ms'] += tr_
        r['apply_ms'] += ta
        r['reduce_bytes'] += 2 * planes
        r['apply_bytes'] += 4 * planes
        if r['widest'] is None or e['n'] > r['widest'][0]['n']:
            r['widest'] = (e, tr_, ta)
    bn = []
    for hw, r in sorted(by_res.items(), reverse=True):
        e, tr_, ta = r['widest']
        st, L = sv['stacks'][e['sid']], net.layers[e['li']]
        out = torch.empty((B, e['n']) + hw, dtype=dt, device='cuda')
        fwd = timed(lambda: ops.bn_relu(st.buf, e['n'], L['beta'], L['gamma'], st.mean, st.inv_std, out=out))
        del out
        bn.append({'resolution': '%dx%d' % hw, 'layers': r['layers'],
                   'reduce_ms': round(r['reduce_ms'], 4), 'apply_ms': round(r['apply_ms'], 4),
                   'reduce_fraction_of_stream': round(r['reduce_bytes'] / (r['reduce_ms'] * 1e-3) / 1e9 / stream, 4),
                   'apply_fraction_of_stream': round(r['apply_bytes'] / (r['apply_ms'] * 1e-3) / 1e9 / stream, 4),
                   'widest_n': e['n'], 'widest_reduce_ms': round(tr_, 4), 'widest_apply_ms': round(ta, 4),
                   'widest_bn_relu_forward_ms': round(fwd, 4), 'widest_bwd_over_forward': round((tr_ + ta) / fwd, 3)})
    # the dense-block layers' weight gradients (Cout = growth): every conv_wgrad_kernel launch but the first conv's,
    # the last of the walk
    wg = [(f, t) for k, f, t in back if k == 'conv_wgrad_kernel'][:-1]
    n_brc = sum(1 for e in net._steps if e['kind'] == 'brc')
    if len(wg) != n_brc:
        raise RuntimeError('expected %d dense-block weight gradients, got %d' % (n_brc, len(wg)))
    wg_ms, wg_flops = sum(t for _, t in wg), sum(f for f, _ in wg)
    return {'dtype': str(dt).replace('torch.', ''), 'batch': B, 'size': '%dx%d' % (H, W), 'step_ms': round(step, 3),
            'step_ms_min': round(float(np.min(ms)), 3), 'images_per_s': round(B / (step * 1e-3), 2),
            'parameters': int(net.flat.numel()), 'weights': 'default synthetic (synthetic.make_densenet_params)',
            'max_memory_allocated_mb': round(peak_mem / 2.0 ** 20, 1), 'profiled_launches': len(rows),
            'profiled_launch_ms': round(all_ms, 3), 'kernels': kernels, 'bn_backward': bn,
            'bn_backward_ms_total': round(sum(red) + sum(app), 3),
            'wgrad_cout16_ms_total': round(wg_ms, 3),
            'wgrad_cout16_fraction_of_peak': round(wg_flops / (wg_ms * 1e-3) / (peak * 1e12), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[3, 10])
    ap.add_argument('--size', default='224x224')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--dtypes', nargs='+', default=['float32', 'float64'])
    ap.add_argument('--peak_tflops', type=float, default=157.3)
    ap.add_argument('--stream_gbs', type=float, default=6600.0)
    ap.add_argument('--weight_decay', type=float, default=1e-4)
    a = ap.parse_args()
    H, W = (int(v) for v in a.size.split('x'))
    rows = []
    for name in a.dtypes:
        for B in a.batches:
            rows.append(one(B, H, W, getattr(torch, name), a.reps, a.peak_tflops, a.stream_gbs, a.weight_decay))
            torch.cuda.empty_cache()
    print(json.dumps({'bench': 'train_densenet', 'device': torch.cuda.get_device_name(0),
                      'peak_tflops': a.peak_tflops, 'stream_gbs': a.stream_gbs, 'reps': a.reps, 'results': rows}))


if __name__ == '__main__':
    main()
