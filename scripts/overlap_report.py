"""How much the matrix-bound and the memory-bound kernels of a run really overlap, from the begin / end stamps of
a rocprofv3 --kernel-trace (csv).

Usage: python scripts/overlap_report.py <kernel_trace.csv> [--window-ms MS] [--min-calls N]

  rocprofv3 --kernel-trace -d DIR --output-format csv -- python bench.py --gpus 1 --steps 20 --warmup 5
  python scripts/overlap_report.py DIR/*/*_kernel_trace.csv --window-ms <steps * ms_per_step of the result line>

The window is the last MS milliseconds before the end of the last conv kernel (the timed steps are the last thing
a plain bench.py run launches); without --window-ms it is the whole trace.

(a) share of the window during which at least one kernel of each class runs;
(b) per transform launch shape (kernel, grid): mean duration by what the launch ran beside.  A launch is 'gemm' /
    'fused' / 'halo' when kernels of that group cover at least half of its duration (the largest wins), 'alone' when
    matrix-bound kernels cover under a tenth of it, 'mixed' otherwise.  Kernels that overlap in time are on different
    streams: one engine's stream is serial."""
import argparse
import csv
import re
from collections import defaultdict

import numpy as np

MATRIX = [('gemm', r'wino_gemm_kernel'), ('fused', r'wino_fused_kernel'), ('halo', r'conv_halo\w*_kernel'),
          ('other_mm', r'conv_igemm|conv_small|conv_taps|conv_kxk|conv_c8|gemm_kernel|Cijk_|conv1x1')]
TRANSFORM = r'wino_output_kernel|wino_input\w*_kernel'


def short(name):
    name = re.sub(r'\(anonymous namespace\)::', '', name)
    name = re.sub(r'^void ', '', name)
    m = re.match(r'([\w:]+)(<[^(]*>)?', name)
    return (m.group(1) + (m.group(2) or '')) if m else name[:60]


def group_of(name):
    for g, pat in MATRIX:
        if re.search(pat, name):
            return g
    return None


def union(iv):
    """sorted disjoint union of [b, e) intervals (n x 2 array)"""
    if len(iv) == 0:
        return np.zeros((0, 2))
    iv = iv[np.argsort(iv[:, 0])]
    out = [list(iv[0])]
    for b, e in iv[1:]:
        if b <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([b, e])
    return np.array(out)


def covered(u, b, e):
    """length of [b, e) inside the disjoint union u"""
    if len(u) == 0:
        return 0.0
    i0 = np.searchsorted(u[:, 1], b, 'right')
    i1 = np.searchsorted(u[:, 0], e, 'left')
    if i1 <= i0:
        return 0.0
    s = u[i0:i1]
    return float((np.minimum(s[:, 1], e) - np.maximum(s[:, 0], b)).sum())


def intersect_len(u, v):
    return sum(covered(v, b, e) for b, e in u)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('trace')
    ap.add_argument('--window-ms', type=float, default=None)
    ap.add_argument('--min-calls', type=int, default=3)
    a = ap.parse_args()
    rows = []
    for r in csv.DictReader(open(a.trace)):
        rows.append((r['Kernel_Name'], float(r['Start_Timestamp']), float(r['End_Timestamp']),
                     r.get('Grid_Size_X', r.get('Grid_Size', '')), r.get('Queue_Id', '')))
    conv_end = max(e for n, b, e, g, q in rows if group_of(n) or re.search(TRANSFORM, n))
    w1 = conv_end
    w0 = w1 - a.window_ms * 1e6 if a.window_ms else min(b for n, b, e, g, q in rows)
    rows = [(n, max(b, w0), min(e, w1), g, q) for n, b, e, g, q in rows if e > w0 and b < w1]
    wall = w1 - w0

    by_group = defaultdict(list)
    mem = []
    for n, b, e, g, q in rows:
        k = group_of(n)
        if k:
            by_group[k].append((b, e))
        else:
            mem.append((b, e))
    u = {k: union(np.array(v)) for k, v in by_group.items()}
    u_mat = union(np.array([iv for v in by_group.values() for iv in v]))
    u_mem = union(np.array(mem))
    busy = union(np.concatenate([u_mat, u_mem]))
    ln = lambda x: float((x[:, 1] - x[:, 0]).sum()) if len(x) else 0.0
    both = intersect_len(u_mat, u_mem)
    queues = sorted({q for n, b, e, g, q in rows})
    print('window %.1f ms, %d dispatches, %d queues' % (wall / 1e6, len(rows), len(queues)))
    print('(a) share of the window with at least one kernel running')
    print('    any kernel                      %6.2f %%' % (100 * ln(busy) / wall))
    print('    a matrix-bound kernel           %6.2f %%' % (100 * ln(u_mat) / wall))
    print('    a memory-bound kernel           %6.2f %%' % (100 * ln(u_mem) / wall))
    print('    one of each class at once       %6.2f %%  (%.1f %% of the memory-bound time)'
          % (100 * both / wall, 100 * both / max(ln(u_mem), 1)))
    tot_mat = sum(e - b for v in by_group.values() for b, e in v)
    tot_mem = sum(e - b for b, e in mem)
    print('    summed kernel time: matrix-bound %.1f ms, memory-bound %.1f ms' % (tot_mat / 1e6, tot_mem / 1e6))

    print('(b) transform launches: mean duration in us (launches) by what ran beside them')
    classes = ['alone', 'gemm', 'fused', 'halo', 'other_mm', 'mixed']
    stat = defaultdict(lambda: defaultdict(list))
    for n, b, e, g, q in rows:
        if not re.search(TRANSFORM, n) or e - b <= 0:
            continue
        d = e - b
        cov = {k: covered(u[k], b, e) / d for k in u}
        allc = covered(u_mat, b, e) / d
        best = max(cov, key=cov.get) if cov else None
        if allc < 0.1:
            c = 'alone'
        elif best and cov[best] >= 0.5:
            c = best
        else:
            c = 'mixed'
        stat[(short(n), g)][c].append(d / 1e3)
    print('    %-58s %9s ' % ('kernel', 'grid') + ' '.join('%16s' % c for c in classes))
    ratio = defaultdict(lambda: [0.0, 0.0])
    for key in sorted(stat, key=lambda k: -sum(sum(v) for v in stat[k].values())):
        s = stat[key]
        if sum(len(v) for v in s.values()) < a.min_calls:
            continue
        cells = ['%9.1f (%4d)' % (np.mean(s[c]), len(s[c])) if s[c] else '%16s' % '-' for c in classes]
        print('    %-58s %9s ' % (key[0][:58], key[1]) + ' '.join('%16s' % c for c in cells))
        if s['alone']:
            base = np.mean(s['alone'])
            for c in classes[1:]:
                if s[c]:
                    ratio[c][0] += sum(s[c])
                    ratio[c][1] += base * len(s[c])
    print('    time beside X over the same launches at their alone mean (shapes that have both):')
    for c in classes[1:]:
        if ratio[c][1]:
            print('      %-9s %.3f  (%.1f ms)' % (c, ratio[c][0] / ratio[c][1], ratio[c][0] / 1e3))


if __name__ == '__main__':
    main()
