"""Shared pieces of the full-size GPU parity tests (fp32 HIP path vs the float64 oracle where the
DePool2D equality masks make strict free-running parity a float64-only property)."""
import contextlib
from unittest import mock

import numpy as np
import torch

from oracle import dae as odae

TOL = 1e-4   # BASELINE.json north_star: within 1e-4 on the refined softmax map


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def to64(p):
    return {k: tuple(np.asarray(a, dtype=np.float64) for a in v) for k, v in p.items()}


def eq_masks(pre, pool):
    h2, w2 = pool.shape[2] * 2, pool.shape[3] * 2
    return pre[:, :, :h2, :w2] == np.repeat(np.repeat(pool, 2, 2), 2, 3)


def teacher_forced_mask_check(ii, H, Y, dp64, levels, dae_kw=None, max_flip_frac=1e-5):
    """One DAE forward from the SAME (GPU) h, y on both sides (fp32 HIP vs float64 oracle):
      1. every mask disagreement is a near-tie (the oracle window's top-2 gap is below twice the
         measured fp32 error of that tensor) and they are < `max_flip_frac` of all mask bits;
      2. with the oracle's masks injected r(y|h) is within 1e-4 everywhere (arithmetic parity).
    Returns (mask bits, flips, teacher-forced max-abs error)."""
    from iterative_inference_segm_amd import ops
    dae_kw = dae_kw or {}
    h64 = [host(h).astype(np.float64) for h in H]
    y64 = host(Y).astype(np.float64)
    r_ref, net = odae.dae_forward(dp64, h64, y64, return_net=True, **dae_kw)
    ii.dae.trace = {}
    ii.dae.scores(H, Y)
    tr = {k: host(v) for k, v in ii.dae.trace.items() if isinstance(v, torch.Tensor)}
    ii.dae.trace = None
    total_bits, flips, override = 0, 0, {}
    for p in range(1, levels + 1):
        mg = eq_masks(tr['pre%d' % p], tr['pool%d' % p])
        mo = eq_masks(net['pre%d' % p], net['pool%d' % p])
        total_bits += mo.size
        pre_err = np.abs(tr['pre%d' % p] - net['pre%d' % p]).max()
        assert pre_err <= 1e-4 * (1 + np.abs(net['pre%d' % p]).max())
        for (b, c, yy, xx) in np.argwhere(mg != mo):
            win = np.sort(net['pre%d' % p][b, c, yy // 2 * 2:yy // 2 * 2 + 2,
                                           xx // 2 * 2:xx // 2 * 2 + 2].ravel())
            assert win[-1] - win[-2] <= 2 * pre_err, \
                'mask disagreement that is not a near-tie at level %d: %s (fp32 err %g)' \
                % (p, win, pre_err)
            flips += 1
        full = np.zeros(net['pre%d' % p].shape, dtype=np.float32)
        full[:, :, :mo.shape[2], :mo.shape[3]] = mo
        override[p] = (torch.from_numpy(full).cuda(),
                       torch.ones(net['pool%d' % p].shape, dtype=torch.float32, device='cuda'))
    assert flips <= max_flip_frac * total_bits
    score = ii.dae.scores(H, Y, mask_override=override)
    r_forced = host(ops.crop_softmax(score, Y.shape[2], Y.shape[3], off=(0, 0)))
    err = float(np.abs(r_forced - r_ref).max())
    assert err <= TOL, 'teacher-forced-mask r(y|h) max-abs err %.3e' % err
    return total_bits, flips, err


def agreement(a, b):
    """(argmax agreement, mean |err|, max |err|, fraction of pixels within 1e-4) of two maps."""
    e = np.abs(a - b)
    return (float((a.argmax(1) == b.argmax(1)).mean()), float(e.mean()), float(e.max()),
            float((e.max(axis=1) <= TOL).mean()))


def assert_within_reference_sensitivity(ii32, ii64, o32, o64, steps, step=0.1, factor=None, label=''):
    """The fp32 path free-running through the DePool2D equality masks on the CHAOTIC default synthetic
    set -- the stress test.  (The fixed-tolerance end-to-end claims live on the damped set:
    tests/test_gpu_damped.py.)

    With the default (random, non-contractive) DAE weights the loop amplifies any perturbation: the
    float64 path fed with y0 * (1 + 1e-7 u), below float32 resolution, leaves the 1e-4 band on most
    pixels after 10 steps (profiles/r02_sensitivity.md).  So for more than one step nothing with a
    fixed ABSOLUTE number can be asserted about ANY float32 implementation; what is ASSERTED here --
      * the inputs of the loop (FCN-8 / DenseNet outputs, no masks involved): y0 within 1e-4, h within
        1e-4 relative to its range;
      * ONE free-running step: argmax agreement >= 0.999 and mean |err| <= 1e-4 against the float64 path;
      * EVERY requested step count: the deviation of the fp32 path RELATIVE to the float64 path's own
        deviation when its inputs are perturbed at the MEASURED input error of the fp32 path (max
        |y0_fp32 - y0_f64| absolute on the probability map, max |h_fp32 - h_f64| relative to h's range --
        no chosen constant): mean deviation <= 2 x, argmax agreement >= that - 0.05.
    Both are printed; `factor` is kept for signature compatibility and ignored."""
    H32, Y32, H64, Y64 = o32[:-1], o32[-1], o64[:-1], o64[-1]
    eps_y = float((Y32.double() - Y64).abs().max())
    eps_h = [float((a.double() - b).abs().max() / b.abs().max()) for a, b in zip(H32, H64)]
    assert eps_y <= TOL and max(eps_h) <= TOL, (label, eps_y, eps_h)
    rng = np.random.default_rng(0)
    u = torch.from_numpy(rng.uniform(-1, 1, size=tuple(Y64.shape))).to(Y64.device)
    H64p = [h + e * float(h.abs().max()) *
            torch.from_numpy(rng.uniform(-1, 1, size=tuple(h.shape))).to(h.device)
            for h, e in zip(H64, eps_h)]
    out = []
    for n in sorted(set([1] + list(steps))):
        base = ii64.refine(H64, Y64, step, n, early_stop=False)[0]
        pert = ii64.refine(H64p, (Y64 + eps_y * u).clamp(0, 1), step, n, early_stop=False)[0]
        got = ii32.refine(H32, Y32, step, n, early_stop=False)[0]
        a, b, c = host(base), host(pert), host(got).astype(np.float64)
        s_ref, s_got = agreement(a, b), agreement(a, c)
        print('%s %d steps: float64 vs float64(inputs perturbed at the measured fp32 input error: y0 '
              '%.1e abs, h %.1e rel) argmax %.5f mean %.2e max %.2e | float64 vs fp32 argmax %.5f mean '
              '%.2e max %.2e' % (label, n, eps_y, max(eps_h), s_ref[0], s_ref[1], s_ref[2], s_got[0],
                                 s_got[1], s_got[2]))
        if n == 1:
            assert s_got[0] >= 0.999 and s_got[1] <= TOL, (label, s_got)
        # EVERY step count, on these (the bench's) weights: the fp32 path stays within the reference
        # function's own sensitivity -- its mean deviation at most twice, and its argmax agreement at
        # most 0.05 below, what the float64 path shows against itself when only its inputs move by the
        # fp32 path's measured input error (measured ratios 0.13 .. 1.0 over all configs and step counts)
        assert s_got[1] <= 2.0 * max(s_ref[1], 1e-7) and s_got[0] >= s_ref[0] - 0.05, (label, n, s_ref, s_got)
        out.append((n, s_ref, s_got))
    return out


# ---- placement of the edge tests (test_gpu_tail_edges.py, test_gpu_bn_pool_deconv_edges.py) -------------------
GUARD = 4096
SENTINEL = -9          # no result is -9: maps lie in [-4, 4], counts, norms and iteration counts are >= 0
_INT_VIEW = {torch.float32: torch.int32, torch.float64: torch.int64, torch.bfloat16: torch.int16,
             torch.int32: torch.int32, torch.int64: torch.int64, torch.uint8: torch.uint8}


def _sentinel(dtype):
    # (a mask byte is at most 15: the sentinel's low byte, 247, serves the uint8 tensors)
    return SENTINEL & 0xFF if dtype == torch.uint8 else SENTINEL


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and \
        torch.equal(a.contiguous().view(_INT_VIEW[a.dtype]), b.contiguous().view(_INT_VIEW[b.dtype]))


class Placed:
    """Hands out device tensors that are views into the middle of sentinel-filled flat allocations, keeps copies
    of the read-only inputs, and checks both afterwards."""

    def __init__(self):
        self.flats, self.inputs, self.blank = [], [], []

    def out(self, shape, dtype, init=None):
        n = int(np.prod(shape))
        flat = torch.full((n + 2 * GUARD,), _sentinel(dtype), dtype=dtype, device='cuda')
        view = flat[GUARD:GUARD + n].view(tuple(shape))
        if init is not None:
            view.copy_(init if isinstance(init, torch.Tensor) else torch.from_numpy(np.array(init)))
        self.flats.append((flat, n))
        if init is None:
            self.blank.append(flat)
        return view

    def inp(self, a, dtype=torch.float32):
        t = a.cuda() if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a)).to(dtype).cuda()
        self.inputs.append((t, t.clone()))
        return t

    def state(self, ops, B, H, W, active=None, iters=None, last_norm=None, npartial=None):
        """A RefineState whose four tensors are placed between sentinels."""
        st = ops.RefineState(B, H, W, 'cuda')
        st.active = self.out((B,), torch.int32,
                             np.ones(B, np.int32) if active is None else np.asarray(active, np.int32))
        st.iters = self.out((B,), torch.int32,
                            np.zeros(B, np.int32) if iters is None else np.asarray(iters, np.int32))
        st.last_norm = self.out((B,), torch.float64,
                                np.zeros(B) if last_norm is None else np.asarray(last_norm, np.float64))
        st.partial = self.out((B * (st.nblk if npartial is None else npartial),), torch.float64)
        return st

    @contextlib.contextmanager
    def allocations(self):
        """Inside: torch.empty_like hands out placed tensors -- the wrappers that allocate their own result
        (sqerr_softmax_bwd, depool_bwd, pool_relu_bwd, add_noise) do it with that call."""
        with mock.patch.object(torch, 'empty_like', lambda t, **kw: self.out(t.shape, t.dtype)):
            yield

    def check(self):
        torch.cuda.synchronize()
        for flat, n in self.flats:
            assert bool((flat[:GUARD] == _sentinel(flat.dtype)).all()), 'wrote in front of a tensor'
            assert bool((flat[GUARD + n:] == _sentinel(flat.dtype)).all()), 'wrote behind a tensor'
        for t, kept in self.inputs:
            assert same_bits(t, kept), 'a read-only input changed'

    def nothing_written(self):
        """Every tensor handed out without initial contents still holds nothing but sentinels."""
        torch.cuda.synchronize()
        return all(bool((flat == _sentinel(flat.dtype)).all()) for flat in self.blank)
