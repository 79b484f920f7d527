"""What scripts/bench_train_std.py and scripts/bench_train_fcn8.py share to report the data-gradient launch of every
3x3 layer: which entries of the launch profile belong to which flipped-filter layer of the
fp32 mode, and the yardstick -- the existing ops.Conv(..., mma='bf16') forward kernel on the flipped filter of that
same layer, on a map of g_z's shape."""
import contextlib

import torch

from iterative_inference_segm_amd import ops


class _Marked:
    """A flipped-filter layer that notes which entries of the launch profile its call made."""

    def __init__(self, conv, name, prof, log):
        self.conv, self.name, self.prof, self.log = conv, name, prof, log

    def __call__(self, *a, **kw):
        i = len(self.prof)
        out = self.conv(*a, **kw)
        self.log.append((self.name, i, len(self.prof)))
        return out

    def __getattr__(self, attr):
        return getattr(self.conv, attr)


@contextlib.contextmanager
def marked(bwd, prof):
    """While it is open the layers of `bwd` ({name: Conv}, or None) log (name, first, last + 1) of their launches'
    entries in `prof`; yields the log."""
    log = []
    if bwd is None:
        yield log
        return
    plain = dict(bwd)
    for name, conv in plain.items():
        bwd[name] = _Marked(conv, name, prof, log)
    try:
        yield log
    finally:
        bwd.update(plain)


def launches(prof, first, last):
    """(ms, flops, kernel names) of the profile entries [first, last) that are convolution launches"""
    rows = [(k, f, a.elapsed_time(b)) for k, f, a, b in prof[first:last] if f > 0]
    return sum(t for _, _, t in rows), sum(f for _, f, _ in rows), '+'.join(k for k, _, _ in rows)


def yardstick(filters, shapes, dt, reps=3):
    """{name: (ms, kernel)}: the bf16 forward kernel ops.Conv(..., mma='bf16') chooses for the flipped filter
    `filters[name]` on a standard-normal map of `shapes[name]`; the fastest of `reps` launches under the launch
    profile."""
    out = {}
    gen = torch.Generator(device='cuda').manual_seed(7)
    for name, Wt in filters:
        if name not in shapes:
            continue
        conv = ops.Conv(Wt.contiguous(), None, pad=1, relu=False, device=Wt.device, dtype=dt, mma='bf16')
        g = torch.randn(shapes[name], generator=gen, device='cuda', dtype=dt)
        conv(g)                                                   # packs / transforms the filter
        torch.cuda.synchronize()
        best = None
        for _ in range(reps):
            prof = []
            ops.profile_begin()
            ops.CONV_PROFILE = prof
            try:
                conv(g)
                torch.cuda.synchronize()
            finally:
                ops.CONV_PROFILE = None
                ops.profile_end()
            t = sum(a.elapsed_time(b) for _, _, a, b in prof)
            if best is None or t < best[0]:
                best = (t, '+'.join(k for k, _, _, _ in prof))
        out[name] = best
        del conv, g
    return out


def layer_rows(names, per_layer, flops, peak, yard=None):
    """One dict per 3x3 layer: its data-gradient launch, the fraction of `peak` TFLOP/s on the nominal flops and,
    with `yard`, the yardstick next to it."""
    rows = []
    for n in names:
        t, kern = per_layer[n]
        row = {'layer': n, 'dgrad_ms': round(t, 4), 'dgrad_kernel': kern,
               'dgrad_fraction_of_peak': round(flops[n] / (t * 1e-3) / (peak * 1e12), 4)}
        if yard and n in yard:
            row.update(bf16_forward_on_flipped_ms=round(yard[n][0], 4), bf16_forward_kernel=yard[n][1],
                       dgrad_over_bf16_forward=round(t / yard[n][0], 3))
        rows.append(row)
    return rows
