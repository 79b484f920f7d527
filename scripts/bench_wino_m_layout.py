"""GEMM and output stages of the separate-GEMM fp32 layers, one launch geometry at a time: the layers a steady
step of the bench workload (FCN-8 + standard DAE, fp32) launches are recorded, then the GEMM stage alone
(stages = IISEG_WINO_GEMM) and the output stage alone (IISEG_WINO_OUTPUT) are timed with HIP events under both
settings of ops.wino_m_quad (old = M[slice][Mpad][Tpad], new = channel quads).  Both stages of a setting run
under that setting: the output stage reads what the GEMM stage of the same setting wrote.
Per geometry: launches per step, MB of M the output stage reads, then per setting GEMM ms, output ms and the
output stage's M read rate in TB/s.  Usage: python scripts/bench_wino_m_layout.py [B] [reps]"""
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

lib = ops._lib.load()
calls, keep = {}, []
staged, run_wino, run_gemm = ops._launch_staged, ops.Conv._run_wino_f32, ops.Conv._run_gemm_f32


def spy_wino(self, c):
    keep.append((self, c))              # the operands stay alive for the replay
    return run_wino(self, c)


def spy_gemm(self, c):
    keep.append((self, c))
    return run_gemm(self, c)


def spy(fn, args, whole, stages):
    d = args[0]._obj
    if fn in (lib.iiseg_conv_wino_f32, lib.iiseg_conv_wino_mask_f32, lib.iiseg_conv_gemm_f32) and not whole & 8:
        add = 7 if fn is lib.iiseg_conv_wino_f32 else 8 if fn is lib.iiseg_conv_wino_mask_f32 else None   # skip-add
        key = (d.C1 + d.C2, d.Cout, d.KH, d.H, d.W, d.oy0, d.ox0, d.OH, d.OW, d.tile_y0, d.tile_x0,
               int(d.flags) & 0xffff, add is not None and bool(args[add]))
        calls.setdefault(key, [0, fn, args])[0] += 1
    return staged(fn, args, whole, stages)


ops._launch_staged, ops.Conv._run_wino_f32, ops.Conv._run_gemm_f32 = spy, spy_wino, spy_gemm
with ops.workspace_tag(ops.current_workspace_tag()):
    bench.one_step(ii, Xs[0], Ts[0], 10, 0.1)
torch.cuda.synchronize()
ops._launch_staged, ops.Conv._run_wino_f32, ops.Conv._run_gemm_f32 = staged, run_wino, run_gemm


def timed(fn, args, bits):
    ms = []
    for _ in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.check(fn(ops._stream(), *args, bits), 'stage %d' % bits)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return sorted(ms[2:])[len(ms[2:]) // 2]


before = ops.wino_m_quad()
print('# Cin Cout k H W window(oy0,ox0,OH,OW) anchor skip_add | launches/step M_MB | old: gemm_ms output_ms M_TB/s | '
      'new: gemm_ms output_ms M_TB/s')
tot = [[0.0, 0.0], [0.0, 0.0]]
for key, (n, fn, args) in sorted(calls.items(), key=lambda kv: -kv[1][0]):
    d = args[0]._obj
    if fn is lib.iiseg_conv_gemm_f32:
        T = d.B * d.OH * d.OW
        Tpad = (T + 127) // 128 * 128
        slices = (lib.iiseg_conv_gemm_workspace_elems(args[0]) // Tpad - d.Kpad) // d.Mpad
    else:
        ty0, tx0 = d.oy0 - ((d.oy0 - d.tile_y0) & 1), d.ox0 - ((d.ox0 - d.tile_x0) & 1)
        T = d.B * ((d.oy0 + d.OH - ty0 + 1) // 2) * ((d.ox0 + d.OW - tx0 + 1) // 2)
        slices = 16
    mbytes = 4.0 * slices * d.Cout * T
    row = []
    for k, on in enumerate((False, True)):
        ops.wino_m_quad(on)
        ops.check(fn(ops._stream(), *args, 7), 'layer')      # V and M of this setting
        g, o = timed(fn, args, 2), timed(fn, args, 4)
        tot[k][0] += n * g
        tot[k][1] += n * o
        row.append('%.4f %.4f %.2f' % (g, o, mbytes / o / 1e9))
    print('%d %d %d %d %d (%d,%d,%d,%d) (%d,%d) %d | %d %.1f | %s | %s'
          % (key[0], key[1], key[2], key[3], key[4], key[5], key[6], key[7], key[8], key[9], key[10], key[-1], n,
             mbytes / 1e6, row[0], row[1]), flush=True)
ops.wino_m_quad(before)
print('# sum over one step (launches x ms): old GEMM %.3f output %.3f ms, new GEMM %.3f output %.3f ms'
      % (tot[0][0], tot[0][1], tot[1][0], tot[1][1]))
