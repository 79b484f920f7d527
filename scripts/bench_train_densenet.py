#!/usr/bin/env python3
"""One training step of FC-DenseNet103 (11 classes, default synthetic weights) on 224x224 crops: one JSON line.

    python scripts/bench_train_densenet.py [--batches 3 10] [--size 224x224] [--reps 5] [--dtypes float32 float64]
                                           [--wgrad f32 f32 bf16] [--deconv f32 f32 bf16] [--fwd f32 f32 bf16]
                                           [--out profiles/NAME.json]

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
--wgrad: the weight-gradient modes to run (FCDenseNet's `wgrad`; bf16: float32 only), one result
row each per batch in the same process; a mode may be named twice, which gives the spread of the measurement.  Every
row lists its zero-padded 3x3 weight-gradient launches per layer (`wgrad3x3_layers`, from the profiled step) and per
resolution (`wgrad3x3_by_resolution`).  A bf16 row also times, for the widest and the narrowest dense-block layer of
each resolution and on the same operands (the step's own t = bn_relu(stack[:, :n]) and a g_z of the layer's shape),
the new form (co_block=16 with db=None, plus ops.conv_wgrad_db: the module's two launches), the 64-block conv_wgrad_bf16_kernel twice and the fp32 kernel (`forms`): five back-to-back
launches between two HIP events each, the fraction of `--peak_tflops_bf16` (2500) on the nominal work.  With both modes
among the rows, `wgrad_compare` gives per batch the launches' sums and the layers whose bf16 launch took longer than
both fp32 rows' launch of that layer.
--deconv: the modes of the TransitionUp gradients to run (FCDenseNet's `deconv`; bf16: float32 only; DESIGN.md section
23), one result row per (wgrad mode, deconv mode, batch) in the same process; named more than once it is the study of
this switch and the `forms` of a bf16 weight-gradient row are left out.  Every row lists, per TransitionUp layer in
backward's order, its two launches (`deconv_layers`: weight gradient and data gradient from the profiled step, each
next to its byte model over `--stream_gbs` and its nominal 2 Cin Cout (products inside the window) over
`--peak_tflops_bf16`).  With both modes among the rows, `deconv_compare` gives per batch the launches' sums, the step
against the spread of the fp32 rows, and every bf16 launch that took longer than the faster fp32 launch it replaces.
--fwd: the modes of the dense-block layers' training forward to run (FCDenseNet's `fwd`; bf16: float32 only; DESIGN.md
section 25), one result row per (wgrad mode, deconv mode, fwd mode, batch) in the same process; named more than once it
is the study of this switch.  Every row lists the forward launch of every dense-block layer from the profiled step
(`fwd_brc_layers`: the fp32 convolution launch alone, or the fused launch) and their sums per resolution
(`fwd_brc_by_resolution`).  A bf16 row also times, for the widest and the narrowest dense-block layer of each
resolution on the step's own stack (`fwd_forms`, five back-to-back launches between two HIP events each): the fused
launch with and without a mask, the fp32 chain it replaces (bn_relu + convolution + dropout_apply + slice copy) and
the fp32 convolution launch alone, the fused launch's byte model (ops.bnrelu_conv_bytes) over `--stream_gbs` and its
nominal work over `--peak_tflops_bf16`.  With both modes among the rows, `fwd_compare` gives per batch the step against
the spread of the fp32 rows, the peak memory, the launches' sums and every fused launch that took longer than the
fp32 convolution launch of the same layer in either fp32 row.
--out: the JSON record also into that file.
Reads nothing outside the repository.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from iterative_inference_segm_amd import _lib, ops, synthetic as S         # noqa: E402
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


WGRAD_KERNELS = ('conv_wgrad_kernel', 'conv_wgrad_bf16_kernel', 'conv_wgrad_bf16_co16_kernel')


def forms(net, B, dt, peak16):
    """The weight gradient of the widest and the narrowest dense-block layer of each resolution in every form, on
    the same operands."""
    sv = net._tsaved
    by_res = {}
    for e in net._steps:
        if e['kind'] == 'brc':
            hw = tuple(sv['stacks'][e['sid']].buf.shape[2:])
            lo, hi = by_res.get(hw, (e, e))
            by_res[hw] = (e if e['n'] < lo['n'] else lo, e if e['n'] > hi['n'] else hi)
    out = []
    gen = torch.Generator(device='cuda').manual_seed(7)
    for hw, pair in sorted(by_res.items(), reverse=True):
        for which, e in zip(('narrowest', 'widest'), pair):
            st, L, n, g = sv['stacks'][e['sid']], net.layers[e['li']], e['n'], net.growth
            t = ops.bn_relu(st.buf, n, L['beta'], L['gamma'], st.mean, st.inv_std)
            gz = torch.randn((B, g) + hw, generator=gen, device='cuda', dtype=dt)
            gz = gz * (torch.rand(gz.shape, generator=gen, device='cuda') < 0.5)      # as behind a dropout mask
            dW, db = torch.empty((g, n, 3, 3), dtype=dt, device='cuda'), torch.empty(g, dtype=dt, device='cuda')
            run = lambda **kw: timed(lambda: ops.conv_wgrad(t, gz, dW, db, pad=1, **kw))
            def module_form():                                    # what `backward` launches for the layer
                ops.conv_wgrad(t, gz, dW, None, pad=1, mma='bf16', co_block=16)
                ops.conv_wgrad_db(gz, db, n, pad=1)
            co16 = timed(module_form)
            b64 = [run(mma='bf16', co_block=64) for _ in range(2)]
            f32 = run(mma='f32')
            co16_again = timed(module_form)
            alone = run(mma='bf16', co_block=16)                  # the kernel with its own db
            flops = 2.0 * n * g * 9 * B * hw[0] * hw[1]
            out.append({'resolution': '%dx%d' % hw, 'layer': which, 'li': e['li'], 'cin': n, 'cout': g,
                        'co16_ms': round(co16, 5), 'co16_again_ms': round(co16_again, 5),
                        'co16_kernel_own_db_ms': round(alone, 5),
                        'bf16_64_ms': [round(v, 5) for v in b64], 'f32_ms': round(f32, 5),
                        'co16_over_bf16_64': round(min(co16, co16_again) / min(b64), 4),
                        'co16_over_f32': round(min(co16, co16_again) / f32, 4),
                        'co16_fraction_of_peak': round(flops / (min(co16, co16_again) * 1e-3) / (peak16 * 1e12), 5),
                        'bf16_64_fraction_of_peak': round(flops / (min(b64) * 1e-3) / (peak16 * 1e12), 5)})
            del t, gz, dW, db
    return out


def brc_forward(net, fwd_rows, B):
    """The forward launch of every dense-block layer in the profiled step's forward rows, in creation order: the row
    whose nominal work is the layer's (2 n g 9 B H W: the fp32 convolution's and the fused launch's alike)."""
    sv, g = net._tsaved, net.growth
    out, i = [], 0
    for e in net._steps:
        if e['kind'] != 'brc':
            continue
        hw = tuple(sv['stacks'][e['sid']].buf.shape[2:])
        want = 2.0 * e['n'] * g * 9 * B * hw[0] * hw[1]
        while i < len(fwd_rows) and fwd_rows[i][1] != want:
            i += 1
        if i == len(fwd_rows):
            raise RuntimeError('no forward launch found for dense-block layer %d' % e['li'])
        out.append({'li': e['li'], 'resolution': '%dx%d' % hw, 'cin': e['n'], 'kernel': fwd_rows[i][0],
                    'ms': round(fwd_rows[i][2], 5)})
        i += 1
    return out


def fwd_forms(net, B, dt, stream, peak16):
    """The widest and the narrowest dense-block layer of each resolution, on the step's own stack: the fused launch
    (with and without a mask) into the stack's slice, the fp32 chain it replaces and the fp32 convolution alone."""
    sv, g, p = net._tsaved, net.growth, net.dropout
    by_res = {}
    for e in net._steps:
        if e['kind'] == 'brc':
            hw = tuple(sv['stacks'][e['sid']].buf.shape[2:])
            lo, hi = by_res.get(hw, (e, e))
            by_res[hw] = (e if e['n'] < lo['n'] else lo, e if e['n'] > hi['n'] else hi)
    out = []
    gen = torch.Generator(device='cuda').manual_seed(11)
    for hw, pair in sorted(by_res.items(), reverse=True):
        for which, e in zip(('narrowest', 'widest'), pair):
            st, L, n = sv['stacks'][e['sid']], net.layers[e['li']], e['n']
            conv = L['conv']
            bn = (L['beta'], L['gamma'], st.mean, st.inv_std)
            keep = (torch.rand((B, g) + hw, generator=gen, device='cuda') >= p).to(dt)
            fused = lambda k: ops.bnrelu_conv_fwd(st.buf, n, bn, conv.W, conv.b, out=st.buf, out_c0=n, keep=k, p=p)

            def chain():
                t = ops.bn_relu(st.buf, n, *bn)
                z = conv(t)
                ops.dropout_apply(z, keep, p)
                st.buf[:, n:n + g].copy_(z)
            t = ops.bn_relu(st.buf, n, *bn)
            z = torch.empty((B, g) + hw, dtype=dt, device='cuda')
            ms = {'fused_keep': timed(lambda: fused(keep)), 'fused_no_keep': timed(lambda: fused(None)),
                  'f32_chain': timed(chain), 'f32_conv_alone': timed(lambda: conv(t, out=z)),
                  'fused_keep_again': timed(lambda: fused(keep))}
            d = ops.bnrelu_conv_desc(tuple(st.buf.shape), n, g, st.buf.shape[1], n)
            best = min(ms['fused_keep'], ms['fused_keep_again'])
            nbytes = ops.bnrelu_conv_bytes(B, n, g, hw[0], hw[1], True)
            flops = 2.0 * n * g * 9 * B * hw[0] * hw[1]
            out.append({'resolution': '%dx%d' % hw, 'layer': which, 'li': e['li'], 'cin': n, 'cout': g,
                        'slabs': int(_lib.load().iiseg_bnrelu_conv_fwd_bf16_slabs(C.byref(d))),
                        **{k + '_ms': round(v, 5) for k, v in ms.items()},
                        'model_mb': round(nbytes / 1e6, 3),
                        'model_us_at_stream': round(nbytes / (stream * 1e9) * 1e6, 2),
                        'fused_fraction_of_stream': round(nbytes / (best * 1e-3) / 1e9 / stream, 4),
                        'fused_fraction_of_peak_bf16': round(flops / (best * 1e-3) / (peak16 * 1e12), 5),
                        'fused_over_f32_chain': round(best / ms['f32_chain'], 4),
                        'fused_over_f32_conv_alone': round(best / ms['f32_conv_alone'], 4)})
            del t, z, keep
    return out


DECONV_KERNELS = {'deconv_wgrad_kernel': 'wgrad', 'deconv_wgrad_bf16_kernel': 'wgrad',
                  'deconv_dgrad_kernel': 'dgrad', 'deconv_dgrad_bf16_kernel': 'dgrad'}


def deconv_layers(net, back, B, mode, stream, peak16):
    """Per TransitionUp layer, in backward's order: its two gradient launches of the profiled step, each against its
    byte model (ops.deconv_wgrad / ops.deconv_dgrad's: x, g, the parameter and the slabs once, gx once) at `stream`
    GB/s and its nominal work at `peak16` TFLOP/s."""
    sv, lib = net._tsaved, _lib.load()
    launches = [(DECONV_KERNELS[k], k, t) for k, _, t in back if k in DECONV_KERNELS]
    tus = [e for e in reversed(net._steps) if e['kind'] == 'tu']
    if [w for w, _, _ in launches] != ['wgrad', 'dgrad'] * len(tus):
        raise RuntimeError('expected a (wgrad, dgrad) pair of launches per TransitionUp layer, got %s'
                           % [k for _, k, _ in launches])
    out = []
    for i, e in enumerate(tus):
        cin, cout = e['n'] - e['block0'], e['keep']
        hw, win = tuple(sv['stacks'][e['sid']].buf.shape[2:]), tuple(sv['win'][e['li']])
        d = ops.deconv_desc((B, cin) + hw, cout, 3, 2, win)
        nx, ng, nw = B * cin * hw[0] * hw[1], B * cout * win[2] * win[3], cin * cout * 9
        if mode == 'bf16':
            ws = lib.iiseg_deconv_wgrad_bf16_workspace_elems(C.byref(d))
            slabs = lib.iiseg_deconv_wgrad_bf16_slabs(C.byref(d))
            wbytes, dbytes = 4.0 * (nx + ng + 2 * ws), 4.0 * (ng + nw + nx)
        else:
            slabs = lib.iiseg_deconv_wgrad_partials(C.byref(d))
            wbytes, dbytes = 4.0 * (nx + ng + 2 * slabs * (nw + cout)), 4.0 * (ng + nx)
        flops = 2.0 * cin * cout * ops._deconv3_products(d)
        row = {'li': e['li'], 'resolution': '%dx%d -> %dx%d' % (hw + win[2:]), 'cin': cin, 'cout': cout,
               'slabs': int(slabs), 'nominal_gflop': round(flops / 1e9, 4)}
        for (which, kern, t), nbytes in zip(launches[2 * i:2 * i + 2], (wbytes, dbytes)):
            row[which] = {'kernel': kern, 'ms': round(t, 5), 'model_mb': round(nbytes / 1e6, 3),
                          'fraction_of_stream': round(nbytes / (t * 1e-3) / 1e9 / stream, 4),
                          'fraction_of_peak_bf16': round(flops / (t * 1e-3) / (peak16 * 1e12), 5)}
        out.append(row)
    return out


def one(B, H, W, dt, reps, peak, stream, weight_decay, wgrad='f32', peak16=2500.0, deconv='f32', with_forms=True,
        fwd_mode='f32'):
    params = S.make_densenet_params(layer_plan(), seed=2024)
    net = FCDenseNet(params, 11, layer=[], dtype=dt, mma='f32', trainable=True, wgrad=wgrad, deconv=deconv, fwd=fwd_mode)
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
    # (a bf16 layer is two launches: its dW kernel and conv_wgrad_db_kernel, counted together)
    wg_all, db_ms = [], 0.0
    for k, f, t in back:
        if k in WGRAD_KERNELS:
            wg_all.append((k, f, t))
        elif k == 'conv_wgrad_db_kernel':
            wg_all[-1] = (wg_all[-1][0], wg_all[-1][1], wg_all[-1][2] + t)
            db_ms += t
    wg = [(f, t) for _, f, t in wg_all][:-1]
    n_brc = sum(1 for e in net._steps if e['kind'] == 'brc')
    if len(wg) != n_brc:
        raise RuntimeError('expected %d dense-block weight gradients, got %d' % (n_brc, len(wg)))
    wg_ms, wg_flops = sum(t for _, t in wg), sum(f for f, _ in wg)
    # every zero-padded 3x3 layer's launch, in backward's order, and their sums per resolution
    layers3 = [e for e in reversed(net._steps) if e['kind'] in ('brc', 'first')]
    per_layer, wres = [], {}
    for e, (k, f, t) in zip(layers3, wg_all):
        hw = tuple(sv['stacks'][e['sid']].buf.shape[2:])
        per_layer.append({'li': e['li'], 'kind': e['kind'], 'resolution': '%dx%d' % hw,
                          'cin': e['n'] if e['kind'] == 'brc' else int(X.shape[1]), 'kernel': k, 'ms': round(t, 5)})
        r = wres.setdefault(hw, dict(launches=0, ms=0.0, flops=0.0))
        r['launches'] += 1
        r['ms'] += t
        r['flops'] += f
    wgrad_by_res = [{'resolution': '%dx%d' % hw, 'launches': r['launches'], 'ms': round(r['ms'], 4),
                     'fraction_of_peak': round(r['flops'] / (r['ms'] * 1e-3) /
                                               ((peak16 if wgrad == 'bf16' else peak) * 1e12), 5)}
                    for hw, r in sorted(wres.items(), reverse=True)]
    extra = {'forms': forms(net, B, dt, peak16)} if wgrad == 'bf16' and with_forms else {}
    tu = deconv_layers(net, back, B, deconv, stream, peak16)
    extra.update(deconv_layers=tu, deconv_ms_total=round(sum(r[w]['ms'] for r in tu for w in ('wgrad', 'dgrad')), 4))
    brc = brc_forward(net, rows[:n_fwd], B)
    fres = {}
    for r in brc:
        q = fres.setdefault(r['resolution'], dict(launches=0, ms=0.0))
        q['launches'] += 1
        q['ms'] += r['ms']
    extra.update(fwd_brc_layers=brc, fwd_brc_ms_total=round(sum(r['ms'] for r in brc), 4),
                 fwd_brc_by_resolution=[{'resolution': k, 'launches': q['launches'], 'ms': round(q['ms'], 4)}
                                        for k, q in fres.items()])
    if fwd_mode == 'bf16':
        extra['fwd_forms'] = fwd_forms(net, B, dt, stream, peak16)         # (last: it writes into the saved stacks)
    return {'dtype': str(dt).replace('torch.', ''), 'wgrad': wgrad, 'deconv': deconv, 'fwd': fwd_mode, 'batch': B, 'size': '%dx%d' % (H, W), 'step_ms': round(step, 3),
            'step_ms_min': round(float(np.min(ms)), 3), 'images_per_s': round(B / (step * 1e-3), 2),
            'parameters': int(net.flat.numel()), 'weights': 'default synthetic (synthetic.make_densenet_params)',
            'max_memory_allocated_mb': round(peak_mem / 2.0 ** 20, 1), 'profiled_launches': len(rows),
            'profiled_launch_ms': round(all_ms, 3), 'kernels': kernels, 'bn_backward': bn,
            'bn_backward_ms_total': round(sum(red) + sum(app), 3),
            'wgrad_cout16_ms_total': round(wg_ms, 3),
            'wgrad_cout16_fraction_of_peak': round(wg_flops / (wg_ms * 1e-3) / (peak * 1e12), 4),
            'wgrad3x3_ms_total': round(sum(t for _, _, t in wg_all), 3), 'wgrad3x3_db_launches_ms': round(db_ms, 3), 'wgrad3x3_by_resolution': wgrad_by_res,
            'wgrad3x3_layers': per_layer, **extra}


def compare(rows):
    """Per batch with f32 and bf16 rows (float32): the 3x3 weight-gradient launches together and layer by layer."""
    out = []
    for B in sorted({r['batch'] for r in rows}):
        f32 = [r for r in rows if r['batch'] == B and r['dtype'] == 'float32' and r['wgrad'] == 'f32']
        b16 = [r for r in rows if r['batch'] == B and r['wgrad'] == 'bf16']
        if not f32 or not b16:
            continue
        tot = [r['wgrad3x3_ms_total'] for r in f32]
        slower = []
        for i, lb in enumerate(b16[0]['wgrad3x3_layers']):
            ref = [r['wgrad3x3_layers'][i]['ms'] for r in f32]
            if lb['ms'] > max(ref):
                slower.append({'li': lb['li'], 'resolution': lb['resolution'], 'cin': lb['cin'], 'bf16_ms': lb['ms'],
                               'f32_ms': ref})
        by_res = []
        for j, rb in enumerate(b16[0]['wgrad3x3_by_resolution']):
            by_res.append({'resolution': rb['resolution'], 'launches': rb['launches'], 'bf16_ms': rb['ms'],
                           'f32_ms': [r['wgrad3x3_by_resolution'][j]['ms'] for r in f32]})
        out.append({'batch': B, 'f32_wgrad3x3_ms': tot, 'f32_spread_ms': round(max(tot) - min(tot), 3),
                    'bf16_wgrad3x3_ms': b16[0]['wgrad3x3_ms_total'],
                    'gain_ms': round(min(tot) - b16[0]['wgrad3x3_ms_total'], 3),
                    'f32_step_ms': [r['step_ms'] for r in f32], 'bf16_step_ms': b16[0]['step_ms'],
                    'by_resolution': by_res, 'layers_slower_than_both_f32_launches': slower})
    return out


def compare_deconv(rows):
    """Per (batch, wgrad mode) with deconv f32 and bf16 rows (float32): the TransitionUp launches together and one
    by one -- a bf16 launch is slower when it took longer than the FASTER fp32 launch it replaces --, the step
    against the spread of the fp32 rows."""
    out = []
    for B, wg in sorted({(r['batch'], r['wgrad']) for r in rows}):
        mine = [r for r in rows if r['batch'] == B and r['wgrad'] == wg and r['dtype'] == 'float32']
        f32, b16 = [r for r in mine if r['deconv'] == 'f32'], [r for r in mine if r['deconv'] == 'bf16']
        if not f32 or not b16:
            continue
        slower, per_layer = [], []
        for i, lb in enumerate(b16[0]['deconv_layers']):
            entry = {'li': lb['li'], 'resolution': lb['resolution'], 'channels': lb['cin']}
            for which in ('wgrad', 'dgrad'):
                ref = [r['deconv_layers'][i][which]['ms'] for r in f32]
                entry[which] = {'f32_ms': ref, 'bf16_ms': lb[which]['ms'], 'speedup': round(min(ref) / lb[which]['ms'], 2)}
                if lb[which]['ms'] > min(ref):
                    slower.append({'li': lb['li'], 'launch': which, 'bf16_ms': lb[which]['ms'], 'f32_ms': ref})
            per_layer.append(entry)
        steps, tot = [r['step_ms'] for r in f32], [r['deconv_ms_total'] for r in f32]
        out.append({'batch': B, 'wgrad': wg, 'f32_deconv_ms': tot, 'bf16_deconv_ms': b16[0]['deconv_ms_total'],
                    'f32_step_ms': steps, 'f32_step_spread_ms': round(max(steps) - min(steps), 3),
                    'bf16_step_ms': b16[0]['step_ms'], 'step_gain_ms': round(min(steps) - b16[0]['step_ms'], 3),
                    'gain_exceeds_spread': bool(min(steps) - b16[0]['step_ms'] > max(steps) - min(steps)),
                    'f32_max_memory_mb': [r['max_memory_allocated_mb'] for r in f32],
                    'bf16_max_memory_mb': b16[0]['max_memory_allocated_mb'],
                    'layers': per_layer, 'launches_slower_than_the_faster_f32_launch': slower})
    return out


def compare_fwd(rows):
    """Per (batch, wgrad mode, deconv mode) with fwd f32 and bf16 rows (float32): the step against the spread of the
    fp32 rows, the peak memory, the dense-block layers' forward launches together, per resolution and one by one -- a
    fused launch is slower when it took longer than the fp32 CONVOLUTION launch alone of that layer in either row."""
    out = []
    for B, wg, dc in sorted({(r['batch'], r['wgrad'], r['deconv']) for r in rows}):
        mine = [r for r in rows if (r['batch'], r['wgrad'], r['deconv']) == (B, wg, dc) and r['dtype'] == 'float32']
        f32, b16 = [r for r in mine if r['fwd'] == 'f32'], [r for r in mine if r['fwd'] == 'bf16']
        if not f32 or not b16:
            continue
        slower = []
        for i, lb in enumerate(b16[0]['fwd_brc_layers']):
            ref = [r['fwd_brc_layers'][i]['ms'] for r in f32]
            if lb['ms'] > min(ref):
                slower.append({'li': lb['li'], 'resolution': lb['resolution'], 'cin': lb['cin'], 'bf16_ms': lb['ms'],
                               'f32_conv_ms': ref})
        by_res = [{'resolution': rb['resolution'], 'launches': rb['launches'], 'bf16_ms': rb['ms'],
                   'f32_conv_ms': [r['fwd_brc_by_resolution'][j]['ms'] for r in f32]}
                  for j, rb in enumerate(b16[0]['fwd_brc_by_resolution'])]
        steps = [r['step_ms'] for r in f32]
        out.append({'batch': B, 'wgrad': wg, 'deconv': dc, 'f32_step_ms': steps,
                    'f32_step_spread_ms': round(max(steps) - min(steps), 3), 'bf16_step_ms': b16[0]['step_ms'],
                    'step_gain_ms': round(min(steps) - b16[0]['step_ms'], 3),
                    'gain_exceeds_spread': bool(min(steps) - b16[0]['step_ms'] > max(steps) - min(steps)),
                    'f32_max_memory_mb': [r['max_memory_allocated_mb'] for r in f32],
                    'bf16_max_memory_mb': b16[0]['max_memory_allocated_mb'],
                    'f32_conv_launches_ms': [r['fwd_brc_ms_total'] for r in f32],
                    'bf16_fused_launches_ms': b16[0]['fwd_brc_ms_total'], 'by_resolution': by_res,
                    'fused_launches_slower_than_an_f32_conv_launch': slower})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[3, 10])
    ap.add_argument('--size', default='224x224')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--dtypes', nargs='+', default=['float32', 'float64'])
    ap.add_argument('--peak_tflops', type=float, default=157.3)
    ap.add_argument('--stream_gbs', type=float, default=6600.0)
    ap.add_argument('--weight_decay', type=float, default=1e-4)
    ap.add_argument('--wgrad', nargs='+', choices=['f32', 'bf16'], default=['f32'])
    ap.add_argument('--deconv', nargs='+', choices=['f32', 'bf16'], default=['f32'])
    ap.add_argument('--fwd', nargs='+', choices=['f32', 'bf16'], default=['f32'])
    ap.add_argument('--peak_tflops_bf16', type=float, default=2500.0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    H, W = (int(v) for v in a.size.split('x'))
    rows = []
    for name in a.dtypes:
        for mode in (a.wgrad if name == 'float32' else ['f32']):        # (bf16 operands: float32 only)
            for dmode in (a.deconv if name == 'float32' else ['f32']):
                for fmode in (a.fwd if name == 'float32' else ['f32']):
                    for B in a.batches:
                        rows.append(one(B, H, W, getattr(torch, name), a.reps, a.peak_tflops, a.stream_gbs,
                                        a.weight_decay, mode, a.peak_tflops_bf16, dmode,
                                        with_forms=len(a.deconv) == 1 and len(a.fwd) == 1, fwd_mode=fmode))
                        torch.cuda.empty_cache()
    record = json.dumps({'bench': 'train_densenet', 'device': torch.cuda.get_device_name(0),
                         'peak_tflops': a.peak_tflops, 'peak_tflops_bf16': a.peak_tflops_bf16,
                         'stream_gbs': a.stream_gbs, 'reps': a.reps, 'wgrad': a.wgrad, 'deconv': a.deconv, 'fwd': a.fwd,
                         'results': rows, 'wgrad_compare': compare(rows), 'deconv_compare': compare_deconv(rows),
                         'fwd_compare': compare_fwd(rows)})
    print(record)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(record + '\n')


if __name__ == '__main__':
    main()
