#!/usr/bin/env python3
"""One training step of FCN-8 (the real architecture, 11 classes, pad 100, default synthetic weights) at batch 10,
224x224: one JSON line.

    python scripts/bench_train_fcn8.py [--batch 10] [--size 224x224] [--reps 15] [--dtypes float32]
                                       [--wgrad f32 bf16] [--dgrad f32 bf16]

Per precision: step ms (median of `reps` warm steps between two HIP events: forward, loss, backward, L2 term, adam,
refresh) and images/s; then, from the dispatch times of ONE more step run under the library's launch profile, per
layer the weight-gradient launches' ms (kernel + finalize) next to the forward launch's ms of that same layer in
that same step, their ratio, and the weight gradient's fraction of `--peak_tflops` (157.3: the fp32 matrix-pipe
peak) on the nominal 2 Cin Cout K^2 OH OW B; and for the element-wise kernels (relu_gate, l2_term) their GB/s on
algorithmic bytes against `--stream_gbs` (6600).  The transposed convolutions' forward launches are not recorded
by the launch profile: theirs are timed between two HIP events on the step's own maps, next to their weight- and
data-gradient launches.  --width_div / --fc_channels shrink the net.
--wgrad: the weight-gradient modes to run, one result row each in the same process (bf16: float32 only; the
thirteen 3x3 layers of its rows are conv_wgrad_bf16_kernel's launches and take their fraction of
`--peak_tflops_bf16`, 2500; the other layers stay on the fp32 kernels and the fp32 peak).
--dgrad: the data-gradient modes to run, one result row per (wgrad, dgrad) pair in the same process; a mode may be
named twice (`--dgrad f32 f32 bf16`: the spread of two runs next to the difference between the modes).  Every row
lists, for the twelve 3x3 layers behind conv1_1, the data-gradient launch of its mode -- the fp32 flipped-filter
layer's, or conv_dgrad_bf16_kernel's (with the ReLU gate that follows inside a block) -- with its fraction of the
mode's peak; the bf16 rows add the yardstick, the existing ops.Conv(..., mma='bf16') forward kernel on the flipped
filter of that same layer on a map of g_z's shape, and the filter images' pack launches of the step; every row has
`refresh_ms`, the cost of refresh() (in the fp32 mode it flips, copies and re-packs those filters too).  DESIGN
section 16.
--kxk: the modes of fc6's and fc7's gradients to run (`--kxk f32 f32 bf16`), one row per (wgrad, dgrad, kxk) in the
same process.  Every row lists under `kxk_layers` the four launches -- fc7's and fc6's weight and data gradient, the
fp32 K x K kernel and flipped-filter layer or conv_wgrad_kxk_bf16_kernel and conv_dgrad_kxk_bf16_kernel (with its
finalize) -- each with its fraction of the mode's peak and next to the layer's forward launch, `kxk_pack_ms` (the
two filter images' pack launches of the step), `refresh_ms` and `max_memory_allocated_mb` (torch.cuda's peak over
the timed steps).  DESIGN section 17.
--fwd: the modes of the training forward to run (`--fwd f32 f32 bf16`), one row per (wgrad, dgrad, kxk, fwd) in the
same process.  Every row lists under `fwd_layers` the forward launch of the thirteen 3x3 layers, fc6 and fc7 in its
mode -- kernel, ms, fraction of the mode's peak -- and for fc6 / fc7 the yardstick `gemm_bf16_ms`: the existing
ops.Conv(..., mma='bf16') im2col + GEMM form (iiseg_conv_gemm_bf16) of that same layer on the step's own input map;
both rows' own layer is timed the yardstick's way too (`warm_ms`: the mean of five back-to-back calls between two
HIP events, after one warm-up call, operands warm in the last-level cache), so that `warm_ms` and `gemm_bf16_ms`
compare like for like while `forward_ms` is the single launch inside the profiled step, its operands cold;
the bf16 rows add the K x K launches' GB/s on their byte model against `--stream_gbs`.  `fwd_pack_ms`: the 3x3
layers' bf16 images packed again by one refresh() (0 in the fp32 mode).  DESIGN section 18.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from iterative_inference_segm_amd import _lib, ops, synthetic as S        # noqa: E402
from iterative_inference_segm_amd.fcn8 import FCN8, PARAM_ORDER           # noqa: E402
from iterative_inference_segm_amd.train import FCN8Trainer                # noqa: E402
from dgrad_bench import launches, layer_rows, marked, yardstick           # noqa: E402

DECONVS = ('upsample', 'score4', 'score2')
KXK = ('score_pool3', 'score_pool4', 'score_fr', 'fc7', 'fc6')
KXK16 = ('fc7', 'fc6')                                   # the layers of kxk='bf16', in backward's order
FWD_IN = {'fc6': 'in_fc6', 'fc7': 'drop6'}               # the saved input maps of the two K x K layers of fwd='bf16'


def one(B, H, W, dt, reps, peak, stream, width_div, fc_channels, weight_decay, wgrad='f32',
        peak_bf16=2500.0, dgrad='f32', yard=None, kxk='f32', fwd='f32', gyard=None):
    params = S.make_fcn8_params(3, 11, seed=1234, width_div=width_div, fc_channels=fc_channels)
    net = FCN8(params, 11, layer=['score'], dtype=dt, mma='f32', trainable=True, wgrad=wgrad, dgrad=dgrad, kxk=kxk,
               fwd=fwd)
    tr = FCN8Trainer(net, 11, [11], learning_rate=1e-4, weight_decay=weight_decay, seed=1)
    X = torch.from_numpy(S.make_images(B, H, W, seed=2)).to(dt).cuda().contiguous()
    T = torch.from_numpy(S.make_labels(B, H, W, n_classes=11, seed=3)).to(dt).cuda().contiguous()
    for _ in range(3):
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
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        net.refresh()
    e1.record()
    torch.cuda.synchronize()
    refresh_ms = e0.elapsed_time(e1) / 5
    # the bf16 images of the 3x3 layers that one refresh() packs again (fwd='bf16' only)
    prof = []
    ops.profile_begin()
    ops.CONV_PROFILE = prof
    try:
        net.refresh()
        torch.cuda.synchronize()
    finally:
        ops.CONV_PROFILE = None
        ops.profile_end()
    fwd_pack_ms = sum(a.elapsed_time(b) for k, _, a, b in prof if k == 'halo_pack_bf16_kernel')
    # one profiled step: every launch of the library between two marks, in launch order
    prof = []
    ops.KERNEL_BYTES.clear()
    ops.profile_begin()
    ops.CONV_PROFILE = prof
    try:
        score = net.forward_train(X, generator=tr.generator)
        n_fwd = len(prof)
        _, g, _ = ops.ctx_loss(score, T, ('crossentropy',), 1.0)
        with marked(net.dgrads.layers, prof) as log:
            net.backward(g)
        if weight_decay > 0:
            for chunk in tr.ranges:
                ops.l2_term(net.flat, net.gflat, chunk, weight_decay)
        torch.cuda.synchronize()
    finally:
        ops.CONV_PROFILE = None
        ops.profile_end()
    convs = [n for n in PARAM_ORDER if n in net.convs]
    # forward_train's order: the thirteen block layers, fc6, fc7, score_fr, score_pool4, score_pool3
    fwd_order = convs[:16] + ['score_pool4', 'score_pool3']
    fwl = [(k, f, a.elapsed_time(b)) for k, f, a, b in prof[:n_fwd] if f > 0]
    if len(fwl) != len(fwd_order):
        raise RuntimeError('expected one forward convolution launch per layer, got %s' % ([k for k, _, _ in fwl],))
    fwd_ms = dict(zip(fwd_order, [t for _, _, t in fwl]))
    fwd_kernel = dict(zip(fwd_order, [k for k, _, _ in fwl]))
    back = prof[n_fwd:]
    by = lambda kern: [(f, a.elapsed_time(b)) for k, f, a, b in back if k == kern]
    # backward's order of the weight gradients
    blocks = [n for n in reversed(convs[:13])]
    wg = dict(zip(DECONVS, by('deconv_wgrad_kernel')))
    if kxk == 'bf16':
        wg.update(zip(KXK[:3], by('conv_wgrad_kxk_kernel')))
        wg.update(zip(KXK16, by('conv_wgrad_kxk_bf16_kernel')))
    else:
        wg.update(zip(KXK, by('conv_wgrad_kxk_kernel')))
    wg.update(zip(blocks, by('conv_wgrad_bf16_kernel' if wgrad == 'bf16' else 'conv_wgrad_kernel')))
    if sorted(wg) != sorted(PARAM_ORDER):
        raise RuntimeError('expected one weight-gradient call per layer, got %d' % len(wg))
    # the transposed convolutions' forward launches do not pass the launch profile: five back-to-back launches
    # of each between two HIP events, on the maps the profiled step kept
    sv = net.saved_maps()

    def timed(fn, n=5):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n
    fwd_ms['upsample'] = timed(lambda: net.upsample(sv['final'], window=sv['win_upsample']))
    fwd_ms['score4'] = timed(lambda: net.score4(sv['fused'], add=sv['score_pool3'], window=sv['win_score4']))
    fwd_ms['score2'] = timed(lambda: net.score2(sv['score_fr'], add=sv['score_pool4'], window=sv['win_score2']))
    for n in DECONVS:
        fwd_kernel[n] = 'deconv (%s form; HIP events)' % getattr(net, n).last_form
    dgrad_ms = dict(zip(DECONVS, [t for _, t in by('deconv_dgrad_kernel')]))
    out = []
    for n in PARAM_ORDER:
        f, t = wg[n]
        row = {'layer': n, 'shape': list(params[n][0].shape), 'wgrad_ms': round(t, 4),
               'wgrad_fraction_of_peak': round(f / (t * 1e-3) /
                                               ((peak_bf16 if (wgrad == 'bf16' and n in blocks) or
                                                 (kxk == 'bf16' and n in KXK16) else peak) * 1e12), 4)}
        if n in fwd_ms:
            row.update(forward_kernel=fwd_kernel[n], forward_ms=round(fwd_ms[n], 4),
                       wgrad_over_forward=round(t / fwd_ms[n], 3))
        if n in dgrad_ms:
            row.update(dgrad_ms=round(dgrad_ms[n], 4), dgrad_over_forward=round(dgrad_ms[n] / fwd_ms[n], 3))
        out.append(row)
    # the twelve 3x3 data gradients, in backward's order (conv1_1's is not formed)
    dnames = blocks[:-1]
    if dgrad == 'bf16':
        dg = [(a.elapsed_time(b), f, k) for k, f, a, b in back if k == 'conv_dgrad_bf16_kernel']
    else:
        dg = [launches(prof, i, j) for n, i, j in log if n in dnames]
        assert [n for n, _, _ in log if n in dnames] == dnames, log
    if len(dg) != len(dnames):
        raise RuntimeError('expected %d data-gradient launches, got %d' % (len(dnames), len(dg)))
    pack_ms = sum(a.elapsed_time(b) for k, _, a, b in back if k == 'conv_dgrad_bf16_pack_kernel')
    # fc7 and fc6 (backward's order): the four launches of the kxk mode, each next to the layer's forward launch
    if kxk == 'bf16':
        kd = [(a.elapsed_time(b), f, k) for k, f, a, b in back if k == 'conv_dgrad_kxk_bf16_kernel']
    else:
        kd = [launches(prof, i, j) for n, i, j in log if n in KXK16]
    if len(kd) != 2:
        raise RuntimeError('expected the data-gradient launches of fc7 and fc6, got %d' % len(kd))
    kpeak = peak_bf16 if kxk == 'bf16' else peak
    kxk_pack_ms = sum(a.elapsed_time(b) for k, _, a, b in back if k == 'conv_dgrad_kxk_bf16_pack_kernel')
    klayers = []
    for n, (t, f, kern) in zip(KXK16, kd):
        fw, tw_ = wg[n]
        klayers.append({'layer': n, 'forward_ms': round(fwd_ms[n], 4),
                        'wgrad_ms': round(tw_, 4), 'wgrad_fraction_of_peak': round(fw / (tw_ * 1e-3) / (kpeak * 1e12), 4),
                        'dgrad_ms': round(t, 4), 'dgrad_kernel': kern,
                        'dgrad_fraction_of_peak': round(f / (t * 1e-3) / (kpeak * 1e12), 4)})
    # the fifteen layers of the fwd mode: the forward launch of this row's mode; fc6 / fc7 next to the existing 16-bit
    # im2col + GEMM form of the same layer on the same input (timed once per process, after the step's figures)
    fpeak = peak_bf16 if fwd == 'bf16' else peak
    if gyard is not None and not gyard:
        for n in FWD_IN:
            conv = ops.Conv(net.convs[n].W.clone(), net.convs[n].b.clone(), pad=0, relu=True, dtype=dt, mma='bf16')
            xin = sv[FWD_IN[n]]
            conv(xin)
            assert conv._W16 is not None and not conv._packs          # iiseg_conv_gemm_bf16 ran
            gyard[n] = timed(lambda: conv(xin))
            del conv
    # the fp32 split-K GEMM form runs an im2col and an output kernel around its matrix launch: their time too
    gl = [n for n in fwd_order if fwd_kernel[n] == 'wino_gemm_kernel']
    around = [[a.elapsed_time(b) for k, _, a, b in prof[:n_fwd] if k == kern]
              for kern in ('gemm_im2col_kernel', 'gemm_output_kernel')]
    staged = {}
    if all(len(v) == len(gl) for v in around):
        staged = {n: around[0][i] + around[1][i] for i, n in enumerate(gl)}
    flayers = []
    for n in convs[:15]:
        fl = net.convs[n].flops(B, *sv[n].shape[2:])
        row = {'layer': n, 'forward_kernel': fwd_kernel[n], 'forward_ms': round(fwd_ms[n], 4),
               'fraction_of_peak': round(fl / (fwd_ms[n] * 1e-3) / (fpeak * 1e12), 4)}
        if n in staged:
            row['forward_ms_with_im2col_and_output'] = round(fwd_ms[n] + staged[n], 4)
        if n in FWD_IN:
            xw = sv[FWD_IN[n]]
            row['warm_ms'] = round(timed(lambda: net.convs[n](xw)), 4)
            if gyard:
                row['gemm_bf16_ms'] = round(gyard[n], 4)
            if fwd == 'bf16':
                xin, Wn = sv[FWD_IN[n]], net.convs[n].W
                d = ops.conv_fwd_kxk_desc(tuple(xin.shape), tuple(Wn.shape))
                lib = _lib.load()
                nws = lib.iiseg_conv_fwd_kxk_bf16_workspace_elems(C.byref(d))
                nbytes = 4.0 * (xin.numel() + Wn.numel() + 2 * nws + sv[n].numel())
                row.update(slabs=lib.iiseg_conv_fwd_kxk_bf16_slabs(C.byref(d)), model_mb=round(nbytes / 1e6, 1),
                           fraction_of_stream=round(nbytes / (fwd_ms[n] * 1e-3) / 1e9 / stream, 4))
        flayers.append(row)
    elem = []
    for kern in ('relu_gate_kernel', 'l2_term_kernel', 'deconv_dgrad_kernel'):
        t = sum(t for _, t in by(kern))
        if t > 0:
            gbs = ops.KERNEL_BYTES.get(kern, 0.0) / (t * 1e-3) / 1e9
            elem.append({'kernel': kern, 'launches': len(by(kern)), 'ms': round(t, 4), 'gb_per_s': round(gbs, 1),
                         'fraction_of_stream': round(gbs / stream, 4)})
    all_ms = float(sum(a.elapsed_time(b) for _, _, a, b in prof))
    tw = sum(r['wgrad_ms'] for r in out)
    twc = sum(r['wgrad_ms'] for r in out if r['layer'] in net.convs)
    t3 = sum(r['wgrad_ms'] for r in out if r['layer'] in blocks)
    tf = sum(r['forward_ms'] for r in out if r['layer'] in net.convs)
    # (the yardstick runs a launch profile of its own: after every figure of the step's has been read)
    if dgrad == 'bf16' and yard is not None and not yard:
        yard.update(yardstick(((n, net.convs[n].W.transpose(0, 1).flip(2, 3)) for n in dnames),
                              {n: tuple(sv[n].shape) for n in dnames}, dt))
    dlayers = layer_rows(dnames, {n: (t, k) for n, (t, _, k) in zip(dnames, dg)},
                         {n: f for n, (_, f, _) in zip(dnames, dg)}, peak_bf16 if dgrad == 'bf16' else peak,
                         yard if dgrad == 'bf16' else None)
    return {'dtype': str(dt).replace('torch.', ''), 'wgrad': wgrad, 'dgrad': dgrad, 'kxk': kxk, 'fwd': fwd,
            'fwd_layers': flayers, 'fwd_3x3_ms_total': round(sum(r['forward_ms'] for r in flayers[:13]), 4),
            'fwd_kxk_ms_total': round(sum(r['forward_ms'] for r in flayers[13:]), 4),
            'fwd_pack_ms': round(fwd_pack_ms, 4),
            'kxk_layers': klayers, 'kxk_pack_ms': round(kxk_pack_ms, 4),
            'kxk_ms_total': round(sum(r['wgrad_ms'] + r['dgrad_ms'] for r in klayers) + kxk_pack_ms, 4),
            'max_memory_allocated_mb': round(peak_mem / 2.0 ** 20, 1),
            'dgrad_3x3_ms_total': round(sum(r['dgrad_ms'] for r in dlayers), 3), 'dgrad_pack_ms': round(pack_ms, 4),
            'refresh_ms': round(refresh_ms, 4), 'dgrad_layers': dlayers, 'batch': B, 'size': '%dx%d' % (H, W),
            'step_ms': round(step, 3),
            'step_ms_min': round(float(np.min(ms)), 3), 'images_per_s': round(B / (step * 1e-3), 1),
            'parameters': int(net.flat.numel()), 'weights': 'default synthetic (synthetic.make_fcn8_params)',
            'profiled_launch_ms': round(all_ms, 3), 'wgrad_ms_total': round(tw, 3), 'wgrad_3x3_ms_total': round(t3, 3),
            'forward_conv_ms_total': round(tf, 3), 'step_over_forward_convs': round(step / tf, 3),
            'wgrad_over_forward': round(twc / tf, 3), 'layers': out, 'elementwise': elem}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=10)
    ap.add_argument('--size', default='224x224')
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--dtypes', nargs='+', default=['float32'])
    ap.add_argument('--peak_tflops', type=float, default=157.3)
    ap.add_argument('--wgrad', nargs='+', choices=['f32', 'bf16'], default=['f32'])
    ap.add_argument('--dgrad', nargs='+', choices=['f32', 'bf16'], default=['f32'])
    ap.add_argument('--kxk', nargs='+', choices=['f32', 'bf16'], default=['f32'])
    ap.add_argument('--fwd', nargs='+', choices=['f32', 'bf16'], default=['f32'])
    ap.add_argument('--peak_tflops_bf16', type=float, default=2500.0)
    ap.add_argument('--stream_gbs', type=float, default=6600.0)
    ap.add_argument('--width_div', type=int, default=1)
    ap.add_argument('--fc_channels', type=int, default=4096)
    ap.add_argument('--weight_decay', type=float, default=1e-4)
    a = ap.parse_args()
    H, W = (int(v) for v in a.size.split('x'))
    yard, gyard = {}, {}
    rows = [one(a.batch, H, W, getattr(torch, name), a.reps, a.peak_tflops, a.stream_gbs, a.width_div,
                a.fc_channels, a.weight_decay, mode, a.peak_tflops_bf16, dmode, yard, kmode, fmode,
                gyard if name == 'float32' else None)
            for name in a.dtypes for mode in a.wgrad for dmode in a.dgrad for kmode in a.kxk for fmode in a.fwd
            if (mode == 'f32' and dmode == 'f32' and kmode == 'f32' and fmode == 'f32') or name == 'float32']
    print(json.dumps({'bench': 'train_fcn8', 'device': torch.cuda.get_device_name(0), 'peak_tflops': a.peak_tflops,
                      'peak_tflops_bf16': a.peak_tflops_bf16,
                      'stream_gbs': a.stream_gbs, 'reps': a.reps, 'results': rows}))


if __name__ == '__main__':
    main()
