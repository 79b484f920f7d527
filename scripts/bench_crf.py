#!/usr/bin/env python3
"""Dense-CRF mean-field throughput on one MI355X: images/s and ms per iteration of
iterative_inference_segm_amd.crf.DenseCRF (the reference's parameters, R = 12) for float32 / float64,
bilateral on / off, at 224x224 and 360x480, batch 10, 80 iterations.  Prints one JSON line.

Op model (bilateral on): 20 vector-ALU lane-operations per (pixel, window tap, iteration) -- colour
distance, one exp, the C = 11 label FMAs and the share of the separable smoothness sums -- against the
vector issue rate of 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz = 78.6e12 lane-operations/s (the 157.3
TFLOP/s FP32 vector peak counts an FMA as two).  The fraction is reported for the float32 bilateral
rows only; it is a model of the work, not a counter reading.

    python scripts/bench_crf.py [--iters 80] [--batch 10] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from iterative_inference_segm_amd import synthetic as S  # noqa: E402
from iterative_inference_segm_amd.crf import DenseCRF  # noqa: E402

LANE_OPS_PER_TAP = 20
VECTOR_LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9


def inputs(B, H, W, C=11, seed=0):
    rng = np.random.default_rng(seed)
    L = S.make_labels(B, H, W, n_classes=C, seed=seed + 1)
    cls = L.argmax(1)
    pal = rng.integers(16, 240, size=(C + 1, 3))
    X = ((pal[cls] + rng.integers(-4, 5, size=(B, H, W, 3)) + 0.5) / 255.0).transpose(0, 3, 1, 2)
    logit = 2.0 * np.eye(C)[np.minimum(cls, C - 1)].transpose(0, 3, 1, 2) + rng.normal(0, 1, (B, C, H, W))
    P = np.exp(logit) / np.exp(logit).sum(1, keepdims=True)
    return np.ascontiguousarray(P, dtype=np.float32), np.ascontiguousarray(X, dtype=np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=80)
    ap.add_argument('--batch', type=int, default=10)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--sizes', type=str, default='224x224,360x480')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_crf.py needs a GPU'
    crf = DenseCRF()
    taps = (2 * crf.radius + 1) ** 2
    rows = []
    for size in a.sizes.split(','):
        H, W = (int(v) for v in size.split('x'))
        P, X = inputs(a.batch, H, W)
        for dt in (torch.float32, torch.float64):
            Pd, Xd = torch.from_numpy(P).to(dt).cuda(), torch.from_numpy(X).to(dt).cuda()
            for bil in (True, False):
                out = torch.empty_like(Pd)
                crf.inference(Pd, Xd, 2, bilateral=bil, out=out)          # warm-up
                torch.cuda.synchronize()
                best = None
                for _ in range(a.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    crf.inference(Pd, Xd, a.iters, bilateral=bil, out=out)
                    e1.record()
                    e1.synchronize()
                    ms = e0.elapsed_time(e1)
                    best = ms if best is None else min(best, ms)
                ops = LANE_OPS_PER_TAP * taps * H * W * a.batch * a.iters
                row = {'size': [H, W], 'dtype': str(dt).split('.')[-1], 'bilateral': bil,
                       'batch_ms': round(best, 3), 'images_per_s': round(a.batch * 1e3 / best, 1),
                       'ms_per_iter': round(best / a.iters, 4)}
                if bil and dt == torch.float32:
                    row['model_lane_ops'] = ops
                    row['vector_peak_fraction'] = round(ops / VECTOR_LANE_OPS_PER_S / (best * 1e-3), 4)
                rows.append(row)
    print(json.dumps({'workload': 'dense-CRF mean field', 'batch': a.batch, 'iters': a.iters,
                      'radius': crf.radius, 'classes': 11, 'min_of_reps': a.reps,
                      'lane_ops_per_tap': LANE_OPS_PER_TAP, 'vector_lane_ops_per_s': VECTOR_LANE_OPS_PER_S,
                      'results': rows}))


if __name__ == '__main__':
    main()
