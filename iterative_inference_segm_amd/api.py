"""The compiled-function level of the reference (iterative_inference.py:187-210) on MI355X:

    pred_fcn_fn(X)        -> [H_1..H_k, Y]          (:188)
    pred_dae_fn(H..., Y)  -> R                      (:190)
    de_fn(H..., Y)        -> Y - R                  (:204)
    val_fn(Y, T)          -> [acc, jacc(2,C), mse]  (:210)

plus `refine(H, Y, step, num_iter)` which replaces the per-image numpy loop of :258-284 with a
batched device loop that keeps the reference's per-image semantics (per-image early stop,
update applied before the test).  Arguments and results are device tensors
(C-contiguous NCHW float32): no host round trip per call.
"""
import contextlib
import os
import weakref

import numpy as np
import torch

from . import ops

import itertools

EPSILON = 1e-3  # iterative_inference.py:53
_ENGINE_IDS = itertools.count(1)
# Replay the steady-state refinement step from a captured HIP graph (see IterativeInference.refine).
# 'auto': when the loop is long enough to pay for the capture; IISEG_GRAPH=0 / 1 force it off / on.
GRAPH_MODE = os.environ.get('IISEG_GRAPH', 'auto')
# captured refinement steps kept per IterativeInference, one per (geometry, step, eps); LRU
GRAPH_CONTEXTS = int(os.environ.get('IISEG_GRAPH_CONTEXTS', '4'))


class Metrics:
    """Result of one val_fn call kept on the device: confusion counts (C x (C+1), prediction x
    truth with the void column last) and [sum mask*mse_px, sum mask]."""

    def __init__(self, n_classes, device, nonfinite=None):
        self.C = n_classes
        self.cm = torch.zeros(n_classes * (n_classes + 1), dtype=torch.int64, device=device)
        self.sums = torch.zeros(2, dtype=torch.float64, device=device)
        self.nonfinite = nonfinite      # the engine's device counter of non-finite input elements, or None
        # the stream the accumulators are filled on (an EnginePool lane's): `result` waits for it
        self.stream = torch.cuda.current_stream(device) if torch.device(device).type == 'cuda' and \
            torch.cuda.is_available() else None

    @staticmethod
    def reduce_host(cm, sums, n_classes):
        """(acc, jacc(2,C), mse) from raw accumulators, as metrics.py:11-65,144-156 define them."""
        C = n_classes
        cm = np.asarray(cm, dtype=np.float64).reshape(C, C + 1)
        nonvoid = cm[:, :C]
        tp = np.diag(nonvoid)
        denom = nonvoid.sum(1) + nonvoid.sum(0) - tp      # TP + FP + FN  (metrics.py:30-35)
        jacc = np.stack([tp, denom], axis=0)
        total = nonvoid.sum()
        acc = float(tp.sum() / total) if total > 0 else float('nan')   # void-masked (:52-63)
        mse = float(sums[0] / sums[1]) if sums[1] > 0 else float('nan')  # (:153-154)
        return acc, jacc, mse

    def result(self):
        if self.stream is not None:
            self.stream.synchronize()
        if self.nonfinite is not None and int(self.nonfinite.item()) != 0:
            raise FloatingPointError('%d non-finite values (NaN / Inf) were fed to pred_fcn_fn since the '
                                     'last check: results are undefined' % int(self.nonfinite.item()))
        return Metrics.reduce_host(self.cm.cpu().numpy(), self.sums.cpu().numpy(), self.C)


class EnginePool:
    """Whole batches in flight: N engines (each with its own nets, sessions, captured graphs and scratch),
    each on its own HIP stream, handed out round-robin -- batch i runs on engine i % N while batch i - 1 is
    still refining on the previous one.  The batches of iterative_inference.py:230-287 do not depend on each
    other, so this is pure scheduling: every batch goes through exactly the launches a single engine would
    issue for it (same kernels, same batch size, same results bit for bit), and the partly filled last round
    of workgroups of one engine's launches, the gaps between its dependent launches and its HBM-bound kernels
    overlap the other engine's matrix work.  Measured (MI355X, configs[1]): 2 in flight +8 % (fp32) / +10 %
    (bf16 C8) images/s at batch 64, +44 % at the reference's batch of 10 (3 in flight: +63 %).

        pool = EnginePool([make_engine() for _ in range(2)])
        pool.prepare(B, H, W)
        for X, T in batches:
            with pool.lane(X, T) as ii:              # ii: the next engine; its stream is current inside
                out = ii.pred_fcn_fn(X)
                ...                                  # refine, val_device: nothing here waits for the GPU
        pool.join()                                  # the caller's stream now sees every lane's results

    Tensors produced inside `lane` belong to that lane's stream: read them after `join()` /
    `synchronize()` (`Metrics.result` waits for its own lane).  One engine = the plain single-stream path."""

    def __init__(self, engines, device='cuda'):
        self.engines = list(engines)
        if not self.engines:
            raise ValueError('EnginePool needs at least one engine')
        self.streams = [torch.cuda.Stream(device=device) for _ in self.engines] \
            if len(self.engines) > 1 else [None]
        self._next = 0

    def __len__(self):
        return len(self.engines)

    @contextlib.contextmanager
    def lane(self, *inputs):
        """The next engine with its stream current.  The lane first waits for what the caller's stream has
        queued so far (the inputs); `inputs`: device tensors of the caller that the lane will read, kept
        from being reused by the caching allocator until the lane is done with them."""
        k = self._next
        self._next = (k + 1) % len(self.engines)
        s = self.streams[k]
        if s is None:
            yield self.engines[k]
            return
        s.wait_stream(torch.cuda.current_stream(s.device))
        for t in inputs:
            if isinstance(t, torch.Tensor) and t.is_cuda:
                t.record_stream(s)
        with torch.cuda.stream(s):
            yield self.engines[k]

    def prepare(self, batch, height, width, channels=3):
        for e, s in zip(self.engines, self.streams):
            with (torch.cuda.stream(s) if s is not None else contextlib.nullcontext()):
                e.prepare(batch, height, width, channels)
        self.join()

    def join(self):
        """The caller's current stream waits for everything queued on the lanes (no host wait)."""
        for s in self.streams:
            if s is not None:
                torch.cuda.current_stream(s.device).wait_stream(s)

    def synchronize(self):
        for s in self.streams:
            if s is not None:
                s.synchronize()


class IterativeInference:
    """Bundles a segmentation net and a DAE and exposes the reference's four functions."""

    def __init__(self, fcn, dae, n_classes, void_labels=(11,), device='cuda',
                 dtype=torch.float32):
        """dtype: torch.float32 (throughput path) or torch.float64 (strict-parity path, the
        reference's CPU numerics); must match the dtype the nets were built with."""
        self.fcn, self.dae = fcn, dae
        self.dtype = dtype
        self.n_classes = n_classes
        self.void_labels = list(void_labels)
        # the metrics kernel implements the one-hot/void-last contract of the reference's
        # datasets: void == n_classes (iterative_inference.py:125)
        if self.void_labels and self.void_labels != [n_classes]:
            raise NotImplementedError('void_labels must be [] or [n_classes]')
        self.device = device
        # provenance records of the h maps handed out by pred_fcn_fn (fcn8.FCN8.last_provenance),
        # keyed by tensor identity: id -> (weakref, torch version counter, record)
        self._prov = {}
        self._graphs = {}        # steady-state refinement steps captured as HIP graphs
        # scratch buffers (Winograd workspaces, ...) are per engine: two engines may run concurrently
        # on two streams (ops.workspace_tag)
        self._ws_tag = next(_ENGINE_IDS)
        # Non-finite inputs: the conv kernels do not promise to propagate a NaN (a ReLU may swallow it; the
        # reference's Theano graph would hand it through to the output), so they are counted where they
        # enter -- every batch given to pred_fcn_fn, one HBM-bound pass, no synchronisation -- and reported
        # when results are read (`val_fn`, `Metrics.result`, `check_finite`).  Weights: ops.Conv refuses them.
        self._nonfinite = None

    def check_finite(self):
        """Raises FloatingPointError if any batch handed to pred_fcn_fn since the last call held NaN / Inf
        (synchronises); resets the counter."""
        if self._nonfinite is None:
            return
        n = int(self._nonfinite.item())
        self._nonfinite.zero_()
        if n:
            raise FloatingPointError('%d non-finite values (NaN / Inf) in the images given to pred_fcn_fn' % n)

    def __del__(self):
        # the engine's scratch buffers go with it
        try:
            ops.drop_workspaces(self._ws_tag)
        except Exception:
            pass

    def _remember(self, outs):
        prov = getattr(self.fcn, 'last_provenance', None)
        self._prov = {}
        if prov is not None:
            for t, tag in zip(outs, prov):
                if tag is not None:
                    self._prov[id(t)] = (weakref.ref(t), t._version, tag)
        return outs

    def provenance_of(self, h):
        """The record pred_fcn_fn kept for this very tensor object, or None: a clone / slice /
        host copy is another object, and an in-place edit bumps torch's version counter -- both
        fall back (loudly visible through this method) to the full first step."""
        ent = self._prov.get(id(h))
        if ent is None or ent[0]() is not h or h._version != ent[1]:
            return None
        return ent[2]

    def prepare(self, batch, height, width, channels=3):
        """Load-time constant folding for one input geometry: with pad 100 most of every encoder
        map (of the FCN-8 and, through the h it hands over, of the DAE) is a function of the
        weights alone.  This evaluates those borders once, from an all-zero image, so that every
        later batch -- the first one included -- recomputes only the image-dependent regions.
        Purely an optimisation: results are bit-identical with or without it, and nothing an input
        batch produced is ever reused for another batch."""
        if self.fcn is None:
            return
        x0 = torch.zeros((int(batch), int(channels), int(height), int(width)), dtype=self.dtype,
                         device=self.device)
        with ops.workspace_tag(self._ws_tag):
            return self._prepare(x0)

    def _prepare(self, x0):
        out = self._remember(self.fcn(x0))
        if not isinstance(out, (list, tuple)) or len(out) < 2 or not hasattr(self.dae, 'new_session'):
            return
        H, Y = list(out[:-1]), out[-1]
        sess = self.dae.new_session(H, Y, tags=[self.provenance_of(h) for h in H])
        if sess is not None:
            self.dae.scores(H, Y, session=sess)

    # ---- reference function level -------------------------------------------------------
    def pred_fcn_fn(self, X):
        with ops.workspace_tag(self._ws_tag):
            X = self._dev(X)
            if X.is_cuda:
                if self._nonfinite is None:
                    self._nonfinite = torch.zeros(1, dtype=torch.int32, device=X.device)
                ops.count_nonfinite(X, self._nonfinite)
            return self._remember(self.fcn(X))

    def pred_dae_fn(self, *args):
        with ops.workspace_tag(self._ws_tag):
            return self.dae(*[self._dev(a) for a in args])

    def de_fn(self, *args):
        with ops.workspace_tag(self._ws_tag):
            return self.dae.residual(*[self._dev(a) for a in args])

    def val_fn(self, Y, T):
        """[acc, jacc, mse] on the host (synchronises); use `val_device` inside loops."""
        acc, jacc, mse = self.val_device(Y, T).result()
        return [acc, jacc, mse]

    def val_device(self, Y, T):
        m = Metrics(self.n_classes, self.device, nonfinite=self._nonfinite)
        ops.confusion_accumulate(self._dev(Y), self._dev(T), m.cm, m.sums)
        return m

    # ---- fused loop ---------------------------------------------------------------------
    def refine(self, *args, **kw):
        with ops.workspace_tag(self._ws_tag):
            return self._refine(*args, **kw)

    def _refine(self, H, Y, step, num_iter, eps=EPSILON, early_stop=True, inplace=False,
                per_iter_target=None, mode='residual', h_provenance=None,
                first_reconstruction=False, graph=None):
        """Batched replacement of iterative_inference.py:258-284.

        for it in range(num_iter):  score = DAE(H, y)                    # de_fn, :267
                                    y = clip(y - step*(y - softmax(score)), 0, 1)  # :270-273
                                    per image: stop once mean_px ||de||_2 < eps     # :275-277
        Returns (Y_ii, iters_used[B] int32, last_norm[B] float64), all on the device.

        mode='gradient' (extension; the reference only has the residual form,
        F1): descends the true gradient of E(y) = sum (r(y|h) - y)^2,
            y = clip(y - step * (J_r^T 2(r - y) - 2(r - y)), 0, 1),
        with a hand-written backward pass through the DAE (`StandardDAE.backward_y`, or
        `ContextModDAE.sqerr_backward` -- the kind the driver defaults to); the stop test
        uses mean_px ||grad||_2.  A DAE without `backward_y` (kind 'fcn8') is refused with
        NotImplementedError before any launch.  The gradient loop is eager.

        `graph` (None = api.GRAPH_MODE): replay the steady-state step (everything after the first
        step has static shapes and static buffers: the session's encoder maps, y, h, the loop
        state) from ONE captured HIP graph instead of launching its ~36 kernels from Python again
        every iteration.  Same kernels in the same order on the same stream, so results are bit for
        bit those of the eager loop.  The per-image stop test stays on the device (frozen images
        flow through unchanged, `iters` / `last_norm` are read once by the caller): no host
        synchronisation inside the loop.  Used for mode='residual' without `per_iter_target`.

        `first_reconstruction`: also return r(y_0 | h) = softmax of the first step's score map, i.e.
        the `pred_dae_fn(H, Y)` of iterative_inference.py:250 without a second DAE forward (it is
        the same forward as the loop's first `de_fn` call); appended to the returned tuple.

        `h_provenance`: explicit provenance records for H (one per h, `provenance_of(h)` of the
        tensors pred_fcn_fn returned) when the caller hands in copies of them; default: looked up
        by tensor identity.

        `per_iter_target` (one-hot T): also returns a (num_iter, C*(C+1)) int64 tensor of
        per-iteration confusion counts over the images still iterating after that iteration --
        the `valid_mat[:, :, it] += jacc_iter` of iterative_inference_valid.py:231,280-288 (the
        reference calls val_fn only when the loop did not break).
        """
        if mode not in ('residual', 'gradient'):
            raise ValueError('mode must be "residual" or "gradient"')
        if mode == 'gradient' and not hasattr(self.dae, 'backward_y'):
            # refused before any launch of the loop
            raise NotImplementedError(
                "mode='gradient' needs the DAE's backward pass (backward_y), which the DAE kind %r (%s) does "
                "not have: it is built for the kinds 'standard' and 'contextmod'"
                % (getattr(self.dae, 'kind', '?'), type(self.dae).__name__))
        if mode == 'gradient' and getattr(self.dae, 'kind', None) == 'contextmod':
            if getattr(self.dae, 'c8', False):
                self.dae._refuse_c8("mode='gradient'")  # (no backward pass on the 16-bit leg: before any launch)
            self.dae._refuse_wide("mode='gradient'")    # (nor with more than 16 channels into conv1)
        H_in = list(H) if isinstance(H, (list, tuple)) else [H]
        want_graph = GRAPH_MODE if graph is None else ('1' if graph else '0')
        if inplace:
            want_graph = '0'    # the graph path works on its own static copy of y
        if want_graph != '0' and mode == 'residual' and per_iter_target is None and \
                hasattr(self.dae, 'new_session') and int(num_iter) >= 3 and torch.cuda.is_available():
            # 'auto': a capture costs about as much as the launches it saves in one short loop, so
            # it must be reusable -- the DAE session (whose buffers the graph points into) has to be
            # the persistent one that the next batch gets again (every h with a provenance record;
            # StandardDAE.new_session) -- or the loop long enough to amortise it
            tags = list(h_provenance) if h_provenance is not None else \
                [self.provenance_of(a) if isinstance(a, torch.Tensor) else None for a in H_in]
            persistent = bool(tags) and all(t is not None for t in tags) and \
                getattr(self.dae, 'licm', False) and getattr(self.dae, 'fold_border', False)
            # ... or one whose buffers stay the same from batch to batch without any record (the C8 DAE hands
            # out buffer-stable sessions: StandardDAE.new_session)
            persistent = persistent or (getattr(self.dae, 'stable_sessions', False) and
                                        getattr(self.dae, 'licm', False))
            if want_graph == '1' or persistent or int(num_iter) >= 16:
                return self._refine_graph(H_in, Y, step, int(num_iter), eps if early_stop else -1.0,
                                          tags, first_reconstruction)
        H = [self._dev(h) for h in H_in]
        # where each h came from: explicit records, else what pred_fcn_fn remembered for these
        # very tensor objects (None -> no cross-batch reuse for this call)
        tags = list(h_provenance) if h_provenance is not None else \
            [self.provenance_of(a) if isinstance(a, torch.Tensor) else None for a in H_in]
        y = self._dev(Y)
        if not inplace:
            y = y.clone()
        B, _, Hh, Ww = y.shape
        st = ops.RefineState(B, Hh, Ww, y.device)
        eps_eff = eps if early_stop else -1.0
        per_iter, r0 = None, None
        if per_iter_target is not None:
            T = self._dev(per_iter_target)
            nb = self.n_classes * (self.n_classes + 1)
            per_iter = torch.zeros((int(num_iter), nb), dtype=torch.int64, device=y.device)
            scratch = torch.zeros(2, dtype=torch.float64, device=y.device)
        # h is fixed and only y evolves: the DAE may keep loop-invariant parts of its maps
        sess = self.dae.new_session(H, y, tags=tags) if hasattr(self.dae, 'new_session') else None
        if hasattr(self.dae, 'keep_pre'):
            self.dae.keep_pre = mode == 'gradient'     # backward_y reads the pre-pool maps
        fused = getattr(self.dae, 'fused_step', None) if mode == 'residual' else None
        for it in range(int(num_iter)):
            if fused is not None and sess is not None and not (it == 0 and first_reconstruction):
                # scores + update as the DAE's own fused step (context module: its last layers and the update
                # are one launch)
                nblk = fused(H, y, st, step, sess)
                if nblk is not None:
                    ops.refine_finalize(st, eps_eff, nblk=nblk)
                    if per_iter is not None:
                        ops.confusion_accumulate(y, T, per_iter[it], scratch, active=st.active)
                    if early_stop and it + 1 < int(num_iter) and not bool(st.active.any()):
                        break
                    continue
            score = self.dae.scores(H, y, session=sess) if sess is not None \
                else self.dae.scores(H, y)
            if it == 0 and first_reconstruction:
                r0 = ops.crop_softmax(score, Hh, Ww, off=(0, 0))
            if mode == 'gradient':
                if hasattr(self.dae, 'sqerr_backward'):
                    # (context module: the softmax backward, the last layer's adjoint and a mask are one launch)
                    g_through = self.dae.sqerr_backward(score, y)
                else:
                    # (a C8 standard DAE walks on bf16 C8 maps in there, fp32 NCHW in and out; grad_update does not
                    # feed the session's y8 -- `c8_feed` -- so the next `scores` converts y itself)
                    g_through = self.dae.backward_y(ops.sqerr_softmax_bwd(score, y, off=(0, 0)), y.shape)
                ops.grad_update(score, g_through, y, st, step, off=(0, 0))
            elif mode == 'residual':
                self._update(score, y, st, step, sess)
            else:
                raise ValueError('mode must be "residual" or "gradient"')
            ops.refine_finalize(st, eps_eff)
            if per_iter is not None:
                ops.confusion_accumulate(y, T, per_iter[it], scratch, active=st.active)
            # every image has met the stop test: the remaining iterations would not change anything
            # (the reference breaks out of its per-image loop, iterative_inference.py:276-277).
            # One small device->host read per iteration, only when early stopping is on.
            if early_stop and it + 1 < int(num_iter) and not bool(st.active.any()):
                break
        res = (y, st.iters, st.last_norm)
        if per_iter is not None:
            res = res + (per_iter,)
        if first_reconstruction:
            res = res + (r0,)
        return res

    def _refine_graph(self, H_in, Y, step, num_iter, eps_eff, h_provenance, first_reconstruction):
        """The loop of `refine` with its steady-state step replayed from a HIP graph.

        Static buffers (owned by a per-geometry context): y, the h maps, the loop state; the DAE
        session's encoder maps are static by construction.  Per call: copy Y / H in, step 0 eagerly
        (it recomputes the larger region a new batch touches), then steps 1.. as graph replays.  The
        graph is captured once per (geometry, step, eps, session): the first call runs step 1
        eagerly too (weight packing, launch plans and workspaces come into being there) and
        captures step 2."""
        from . import ops as _ops
        tags = list(h_provenance) if h_provenance is not None else \
            [self.provenance_of(a) if isinstance(a, torch.Tensor) else None for a in H_in]
        H_src = [self._dev(h) for h in H_in]
        y_src = self._dev(Y)
        key = (tuple(tuple(h.shape) for h in H_src), tuple(y_src.shape), y_src.dtype, float(step),
               float(eps_eff))
        ctx = self._graphs.get(key)
        if ctx is None:
            B, _, Hh, Ww = y_src.shape
            ctx = {'y': torch.empty_like(y_src), 'H': [torch.empty_like(h) for h in H_src],
                   'st': _ops.RefineState(B, Hh, Ww, y_src.device), 'graph': None, 'sess': None}
            # a few geometries side by side (alternating batch shapes do not re-capture every call);
            # the least recently used context goes first
            while len(self._graphs) >= GRAPH_CONTEXTS:
                self._graphs.pop(next(iter(self._graphs)))
            self._graphs[key] = ctx
        else:
            self._graphs[key] = self._graphs.pop(key)      # most recently used last
        y, H, st = ctx['y'], ctx['H'], ctx['st']
        y.copy_(y_src)
        for dst, src in zip(H, H_src):
            dst.copy_(src)
        st.reset()
        if hasattr(self.dae, 'keep_pre'):
            self.dae.keep_pre = False        # (a gradient-mode call before this one leaves it set)
        sess = self.dae.new_session(H, y, tags=tags)
        dae_scores = (lambda: self.dae.scores(H, y, session=sess)) if sess is not None else \
            (lambda: self.dae.scores(H, y))

        fused = getattr(self.dae, 'fused_step', None)

        def one_step():
            if fused is not None and sess is not None:
                nblk = fused(H, y, st, step, sess)
                if nblk is not None:
                    _ops.refine_finalize(st, eps_eff, nblk=nblk)
                    return None
            score = dae_scores()
            self._update(score, y, st, step, sess)
            _ops.refine_finalize(st, eps_eff)
            return score

        score = dae_scores()                                     # step 0, eager
        # The captured step is valid only for the launch structure and the buffers it was captured
        # on.  Step 0 has just run on the CURRENT ones (it re-primes the session when the masked-level
        # set, trace / keep_pre, ... changed since the last call), so the fingerprint is taken here.
        fp = (id(sess), self._launch_fingerprint(sess))
        # ... and for the scratch (Winograd / BN workspaces of this engine's tag) the captured
        # launches point into: a larger launch elsewhere may have regrown one since the capture,
        # which hands the old allocation back to the caching allocator
        if ctx.get('fingerprint') != fp or \
                (ctx['graph'] is not None and ctx.get('ws_ptrs') != _ops.workspace_ptrs(y.device)):
            ctx['graph'], ctx['fingerprint'] = None, fp
            ctx.pop('keep', None)            # nothing pins the old session / scratch any longer
        r0 = _ops.crop_softmax(score, y.shape[2], y.shape[3], off=(0, 0)) if first_reconstruction \
            else None
        self._update(score, y, st, step, sess)
        _ops.refine_finalize(st, eps_eff)
        it = 1
        if ctx['graph'] is None and it < num_iter:
            one_step()                                           # step 1, eager: lazy state settles
            it += 1
            if it < num_iter:
                prof, _ops.CONV_PROFILE = _ops.CONV_PROFILE, None
                g = torch.cuda.CUDAGraph()
                torch.cuda.synchronize()
                with torch.cuda.graph(g):
                    one_step()
                _ops.CONV_PROFILE = prof
                ctx['graph'] = g
                # scratch the captured launches point at must outlive the graph
                ctx['keep'] = (_ops.workspace_refs(y.device), sess)
                ctx['ws_ptrs'] = _ops.workspace_ptrs(y.device)
        g = ctx['graph']
        while it < num_iter:
            g.replay()
            it += 1
            # per-image early stop (iterative_inference.py:275-277): once every image is frozen the
            # remaining replays would change nothing.  One 4-byte read every 4th replay, only when
            # the stop test is on.
            if eps_eff >= 0 and it < num_iter and (it & 3) == 0 and not bool(st.active.any()):
                break
        res = (y.clone(), st.iters.clone(), st.last_norm.clone())
        if first_reconstruction:
            res = res + (r0,)
        return res

    def _update(self, score, y, st, step, sess):
        """The fused update of iterative_inference.py:270-273; under mma='bf16c8' it also writes the
        new y in the DAE's input format (bf16 C8) into the session's buffer."""
        y8 = self.dae.c8_feed(sess) if hasattr(self.dae, 'c8_feed') else None
        if y8 is not None and y8.shape[0] == y.shape[0] and tuple(y8.shape[2:4]) == tuple(y.shape[2:]):
            ops.refine_update(score, y, st, step, off=(0, 0), y8=y8)
            self.dae.c8_fed(sess)
        else:
            ops.refine_update(score, y, st, step, off=(0, 0))
        if sess is not None and hasattr(self.dae, 'y_updated'):
            self.dae.y_updated(sess, y)     # (context module: the concat buffer's y channels follow y)

    def _launch_fingerprint(self, sess):
        """What a captured refinement step depends on besides shapes: the DAE's launch-structure
        switches and the identity of the session buffers the launches point into."""
        dae = self.dae
        knobs = tuple(getattr(dae, k, None) for k in
                      ('dce', 'licm', 'fold_border', 'fuse_unpool', 'use_masks', 'keep_pre',
                       'emulate_noise', 'mma')) + (getattr(dae, 'trace', None) is not None,)
        if not isinstance(sess, dict):
            return knobs
        bufs = tuple(sorted((k, v.data_ptr()) for k, v in sess.items()
                            if isinstance(v, torch.Tensor) and v.device.type != 'meta'))
        return knobs + (sess.get('masked'), sess.get('gen'), bufs)

    def _dev(self, a):
        if isinstance(a, torch.Tensor):
            t = a
        else:
            t = torch.from_numpy(np.ascontiguousarray(a))
        if t.dtype != self.dtype:
            t = t.to(self.dtype)
        if not t.is_cuda:
            t = t.to(self.device, non_blocking=True)
        return t.contiguous()
