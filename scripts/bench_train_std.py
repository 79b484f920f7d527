#!/usr/bin/env python3
"""One training step of the headline standard DAE (BASELINE configs[1]: 64 filters, concat_h=['pool4'],
additional_pool=2, pad 100, trackind, skip) at batch 10, 224x224, from_gt, noise 0.1: one JSON line.

    python scripts/bench_train_std.py [--batch 10] [--size 224x224] [--reps 15] [--dtypes float32 float64]
                                      [--wgrad f32 bf16] [--dgrad f32 bf16] [--fwd f32 bf16]

Per precision: step ms (median of `reps` warm steps between two HIP events: forward, loss, backward, RMSprop,
refresh) and images/s; then, from the dispatch times of ONE more step run under the library's launch profile, per
layer the weight-gradient launches' ms (kernel + finalize; both sources of the concat layer) next to the forward
launch's ms of that same layer in that same step, their ratio, and the weight gradient's fraction of
`--peak_tflops` (157.3: the fp32 matrix-pipe peak) on the nominal 2 Cin Cout 9 OH OW B.  A trainable StandardDAE
runs its forward layers on the direct / halo kernels (no Winograd form: DESIGN section 12).
--wgrad: the weight-gradient modes to run, one result row each in the same process (bf16: float32 only; its rows
count conv_wgrad_bf16_kernel's launches and take their fraction of `--peak_tflops_bf16`, 2500).
--dgrad: the data-gradient modes to run, one result row per (wgrad, dgrad) pair in the same process; a mode may be
named twice (`--dgrad f32 f32 bf16`: the spread of two runs next to the difference between the modes).  Every row
lists, per 3x3 layer, the data-gradient launch of its mode -- the fp32 flipped-filter layer's, or
conv_dgrad_bf16_kernel's -- with its fraction of the mode's peak; the bf16 rows add the yardstick, the existing
ops.Conv(..., mma='bf16') forward kernel on the flipped filter of that same layer on a map of g_z's shape, and the
filter images' pack launches of the step; every row has `refresh_ms`, the cost of refresh() (in the fp32 mode it
flips, copies and re-packs the data-gradient filters too).  DESIGN section 16.
--fwd: the forward modes to run (StandardDAE's `fwd`; bf16: float32 only), one result row per (wgrad, dgrad, fwd)
triple in the same process; a mode may be named twice (`--fwd f32 f32 bf16`).  Every row lists per layer the forward
launch of its mode (`forward_kernel`, `forward_ms`: conv_halo_bf16_kernel's in the bf16 rows), `refresh_ms` (the bf16
rows re-pack the twelve bf16 filter images instead of the fp32 packs) and `peak_mem_mib`, the allocator's peak over
the row.  DESIGN section 20.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from iterative_inference_segm_amd import ops, synthetic as S              # noqa: E402
from iterative_inference_segm_amd.dae import StandardDAE, param_order     # noqa: E402
from iterative_inference_segm_amd.train import DAETrainer                 # noqa: E402
from dgrad_bench import launches, layer_rows, marked, yardstick           # noqa: E402


def one(B, H, W, dt, reps, peak, wgrad='f32', dgrad='f32', peak_d=157.3, yard=None, fwd='f32'):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    params = S.make_dae_params(seed=4321)
    dae = StandardDAE(params, 11, dtype=dt, mma='f32', trainable=True, wgrad=wgrad, dgrad=dgrad, fwd=fwd)
    tr = DAETrainer(None, dae, 11, [11], noise=0.1, seed=1)
    T = torch.from_numpy(S.make_labels(B, H, W, n_classes=11, seed=3)).to(dt).cuda().contiguous()
    y = T[:, :11].contiguous()
    hh, hw = H + 198, W + 198
    for _ in range(4):
        hh, hw = hh // 2, hw // 2
    gen = torch.Generator(device='cuda').manual_seed(1)
    h = [torch.randn((B, 512, hh, hw), generator=gen, device='cuda', dtype=dt)]
    for _ in range(3):
        tr.train_step(h, y, T)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tr.train_step(h, y, T)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    step = float(np.median(ms))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        dae.refresh()
    e1.record()
    torch.cuda.synchronize()
    refresh_ms = e0.elapsed_time(e1) / 5
    # one profiled step: every launch of the library between two marks, in launch order
    prof = []
    ops.profile_begin()
    ops.CONV_PROFILE = prof
    try:
        score = dae.forward_train(h, y, noise=0.1, generator=tr.generator)
        n_fwd = len(prof)
        _, g, _ = ops.ctx_loss(score, T, ('crossentropy',), 1.0)
        with marked(dae.dgrads.layers if dgrad == 'f32' else None, prof) as log:
            dae.backward(g)
        torch.cuda.synchronize()
    finally:
        ops.CONV_PROFILE = None
        ops.profile_end()
    order = param_order()
    total = len(order) // 2
    fl = [(k, f, a.elapsed_time(b)) for k, f, a, b in prof[:n_fwd] if f > 0]
    if len(fl) != len(order):
        raise RuntimeError('expected one forward convolution launch per layer, got %s' % ([k for k, _, _ in fl],))
    fwd_ms = dict(zip(order, [t for _, _, t in fl]))
    fwd_kernel = dict(zip(order, [k for k, _, _ in fl]))
    kern = 'conv_wgrad_bf16_kernel' if wgrad == 'bf16' else 'conv_wgrad_kernel'
    wg = [(f, a.elapsed_time(b)) for k, f, a, b in prof[n_fwd:] if k == kern]
    # backward's order: up_conv1..total, then conv<total>_1..conv1_1, the concat layer (h behind pool4) twice
    names = ['up_conv%d' % p for p in range(1, total + 1)]
    for p in range(total, 0, -1):
        names += ['conv%d_1' % p] * (2 if p == 5 else 1)
    if len(wg) != len(names):
        raise RuntimeError('expected %d weight-gradient calls, got %d' % (len(names), len(wg)))
    rows = {}
    for n, (f, t) in zip(names, wg):
        r = rows.setdefault(n, {'layer': n, 'flops': 0.0, 'wgrad_ms': 0.0})
        r['flops'] += f
        r['wgrad_ms'] += t
    out = []
    for n in order:
        r = rows[n]
        out.append({'layer': n, 'cout': int(params[n][0].shape[0]), 'cin': int(params[n][0].shape[1]),
                    'forward_kernel': fwd_kernel[n], 'wgrad_ms': round(r['wgrad_ms'], 4),
                    'forward_ms': round(fwd_ms[n], 4), 'wgrad_over_forward': round(r['wgrad_ms'] / fwd_ms[n], 3),
                    'wgrad_fraction_of_peak': round(r['flops'] / (r['wgrad_ms'] * 1e-3) / (peak * 1e12), 4)})
    # the data gradients, in backward's order: up_conv1..total, then conv<total>_1..conv2_1 (conv1_1's is not formed)
    dnames = ['up_conv%d' % p for p in range(1, total + 1)] + ['conv%d_1' % p for p in range(total, 1, -1)]
    if dgrad == 'bf16':
        dg = [(a.elapsed_time(b), f, k) for k, f, a, b in prof[n_fwd:] if k == 'conv_dgrad_bf16_kernel']
    else:
        dg = [launches(prof, i, j) for _, i, j in log]
        assert [n for n, _, _ in log] == dnames, log
    if len(dg) != len(dnames):
        raise RuntimeError('expected %d data-gradient launches, got %d' % (len(dnames), len(dg)))
    pack_ms = sum(a.elapsed_time(b) for k, _, a, b in prof[n_fwd:] if k == 'conv_dgrad_bf16_pack_kernel')
    all_ms = float(sum(a.elapsed_time(b) for _, _, a, b in prof))
    tw, tf = sum(r['wgrad_ms'] for r in out), sum(r['forward_ms'] for r in out)
    # (the yardstick runs a launch profile of its own: after every figure of the step's has been read)
    if dgrad == 'bf16' and yard is not None and not yard:
        _, pre, _ = dae._saved
        shapes = {'up_conv%d' % p: (B, dae.dec['up_conv%d' % p].Cout) + tuple(pre[p].shape[2:]) for p in range(1, total + 1)}
        shapes.update({'conv%d_1' % p: tuple(pre[p].shape) for p in range(2, total + 1)})
        yard.update(yardstick(dae._flipped_filters(), shapes, dt))
    dlayers = layer_rows(dnames, {n: (t, k) for n, (t, _, k) in zip(dnames, dg)},
                         {n: f for n, (_, f, _) in zip(dnames, dg)}, peak_d, yard if dgrad == 'bf16' else None)
    return {'dtype': str(dt).replace('torch.', ''), 'wgrad': wgrad, 'dgrad': dgrad, 'fwd': fwd,
            'peak_mem_mib': round(torch.cuda.max_memory_allocated() / 2.0 ** 20, 1), 'wgrad_peak_tflops': peak,
            'dgrad_peak_tflops': peak_d, 'dgrad_ms_total': round(sum(r['dgrad_ms'] for r in dlayers), 3),
            'dgrad_pack_ms': round(pack_ms, 4), 'refresh_ms': round(refresh_ms, 4), 'dgrad_layers': dlayers, 'batch': B,
            'size': '%dx%d' % (H, W), 'step_ms': round(step, 3),
            'step_ms_min': round(float(np.min(ms)), 3), 'images_per_s': round(B / (step * 1e-3), 1),
            'parameters': int(dae.flat.numel()), 'profiled_launch_ms': round(all_ms, 3),
            'wgrad_ms_total': round(tw, 3), 'forward_conv_ms_total': round(tf, 3),
            'wgrad_over_forward': round(tw / tf, 3), 'layers': out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=10)
    ap.add_argument('--size', default='224x224')
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--dtypes', nargs='+', default=['float32', 'float64'])
    ap.add_argument('--peak_tflops', type=float, default=157.3)
    ap.add_argument('--wgrad', nargs='+', choices=['f32', 'bf16'], default=['f32'])
    ap.add_argument('--dgrad', nargs='+', choices=['f32', 'bf16'], default=['f32'])
    ap.add_argument('--fwd', nargs='+', choices=['f32', 'bf16'], default=['f32'])
    ap.add_argument('--peak_tflops_bf16', type=float, default=2500.0)
    a = ap.parse_args()
    H, W = (int(v) for v in a.size.split('x'))
    yard = {}
    rows = [one(a.batch, H, W, getattr(torch, name), a.reps, a.peak_tflops_bf16 if mode == 'bf16' else a.peak_tflops,
                mode, dmode, a.peak_tflops_bf16 if dmode == 'bf16' else a.peak_tflops, yard, fmode)
            for name in a.dtypes for mode in a.wgrad for dmode in a.dgrad for fmode in a.fwd
            if (mode == 'f32' and dmode == 'f32' and fmode == 'f32') or name == 'float32']
    print(json.dumps({'bench': 'train_std', 'device': torch.cuda.get_device_name(0), 'peak_tflops': a.peak_tflops,
                      'peak_tflops_bf16': a.peak_tflops_bf16,
                      'reps': a.reps, 'results': rows}))


if __name__ == '__main__':
    main()
