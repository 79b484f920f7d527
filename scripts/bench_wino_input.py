"""Input transform of the fp32 Winograd layers, one launch geometry at a time: the layers a steady step of
the bench workload (FCN-8 + standard DAE, fp32) launches are recorded, then the input stage alone
(stages = IISEG_WINO_INPUT) is timed with HIP events under both settings of ops.wino_input_wide.
Per geometry: launches per step, bytes of V, kernel (0 per-tile, 1 LDS-staged, 2 streaming), ms, TB/s.
Usage: python scripts/bench_wino_input.py [B] [reps]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from iterative_inference_segm_amd import ops, synthetic as S

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
ii, _, _ = bench.build_model('cuda', ['pool4'], dtype=torch.float32, mma=None)
Xs = [torch.from_numpy(S.make_images(B, 224, 224, seed=1234 + 1000 * i)).cuda() for i in range(2)]
Ts = [torch.from_numpy(S.make_labels(B, 224, 224, seed=99 + 1000 * i)).cuda() for i in range(2)]
ii.prepare(B, 224, 224)
for i in range(2):
    bench.one_step(ii, Xs[i], Ts[i], 10, 0.1)
torch.cuda.synchronize()

calls, keep = {}, []
staged, run = ops._launch_staged, ops.Conv._run_wino_f32


def spy_run(self, c):
    keep.append(c)                      # the operands stay alive for the replay
    return run(self, c)


def spy(fn, args, whole, stages):
    d = args[0]._obj
    lib = ops._lib.load()
    if fn in (lib.iiseg_conv_wino_f32, lib.iiseg_conv_wino_mask_f32):
        mb = fn is lib.iiseg_conv_wino_mask_f32 and args[5] is not None
        key = (d.C1, d.C2, d.H, d.W, d.oy0, d.ox0, d.OH, d.OW, d.tile_y0, d.tile_x0, int(d.flags) & 0xffff, mb)
        calls.setdefault(key, [0, fn, args, whole & 8])[0] += 1
    return staged(fn, args, whole, stages)


ops._launch_staged, ops.Conv._run_wino_f32 = spy, spy_run
with ops.workspace_tag(ops.current_workspace_tag()):
    bench.one_step(ii, Xs[0], Ts[0], 10, 0.1)
torch.cuda.synchronize()
ops._launch_staged, ops.Conv._run_wino_f32 = staged, run


def timed(fn, args, bits):
    ms = []
    for _ in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.check(fn(ops._stream(), *args, bits), 'wino input')
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return sorted(ms[2:])[len(ms[2:]) // 2]


lib = ops._lib.load()
before = ops.wino_input_wide()
print('# C1 C2 H W window(oy0,ox0,OH,OW) anchor mask_bytes | launches/step V_MB | old: kernel ms TB/s | new: kernel ms TB/s')
tot = [0.0, 0.0]
for key, (n, fn, args, fused) in sorted(calls.items(), key=lambda kv: -kv[1][0]):
    d = args[0]._obj
    ty0, tx0 = d.oy0 - ((d.oy0 - d.tile_y0) & 1), d.ox0 - ((d.ox0 - d.tile_x0) & 1)
    T = d.B * ((d.oy0 + d.OH - ty0 + 1) // 2) * ((d.ox0 + d.OW - tx0 + 1) // 2)
    vbytes = 64.0 * (d.C1 + d.C2) * T
    row = []
    for k, on in enumerate((False, True)):
        ops.wino_input_wide(on)
        path = lib.iiseg_conv_wino_input_path(args[0], int(key[-1]))
        ms = timed(fn, args, 1 | fused)
        tot[k] += n * ms
        row.append('%d %.4f %.2f' % (path, ms, vbytes / ms / 1e9))
    print('%d %d %d %d (%d,%d,%d,%d) (%d,%d) %d | %d %.1f | %s | %s'
          % (key[0], key[1], key[2], key[3], key[4], key[5], key[6], key[7], key[8], key[9], key[-1], n,
             vbytes / 1e6, row[0], row[1]), flush=True)
ops.wino_input_wide(before)
print('# sum over one step (launches x ms): old %.3f ms, new %.3f ms' % tuple(tot))
