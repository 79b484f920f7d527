"""Standard conditional DAE  r(y | h)  on the HIP kernels (mirror of reference
models/DAE_h.py:12-63, models/fcn_down.py:9-138, models/fcn_up.py:11-172).

The layer plan is static per (B, H, W): every launch is a fused kernel --
  encoder level p :  conv3x3 (+bias +ReLU; two-source gather where h is concatenated) , maxpool
  decoder level p :  conv3x3 whose input gather IS the DePool2D equality-mask unpool, with the
                     skip sum (ElemwiseSumLayer) and the final center crop fused in the epilogue
so the unpooled tensors, the concatenated tensor and the cropped score are never materialised.
"""
import os

import numpy as np

import torch

from . import ops, regions
from .datagrads import DataGrads, Layer, Views, _embed, flipped
from .params import Trainable, check_mode
from .regions import center
from .weights import load_param_list

# float64 decoder layers on the halo-tile kernel apply DePool2D while staging their patches
# (conv_halo_f64.hip); 0: materialise the unpooled window first (pool_unpool.hip) and run the plain conv
F64_FUSE_UNPOOL = os.environ.get('IISEG_F64_FUSE_UNPOOL', '1') != '0'


def _n_pool(concat_h, additional_pool):
    n = int(concat_h[-1][-1]) if 'pool' in concat_h[-1] else 0   # DAE_h.py:37-40
    return n, n + additional_pool


def param_order(concat_h=('pool4',), conv_before_pool=1, additional_pool=2,
                unpool_type='trackind', bn=0):
    """get_all_param_values order of dae_model_best.npz; with bn=1 every conv is
    followed by its BatchNormLayer entry `<name>_bn` (fcn_down.py:112-114, fcn_up.py:91-93)."""
    _, total = _n_pool(list(concat_h), additional_pool)
    names = []
    for p in range(total):
        for i in range(1, conv_before_pool + 1):
            names.append('conv%d_%d' % (p + 1, i))
            if bn:
                names.append('conv%d_%d_bn' % (p + 1, i))
    for p in range(total, 0, -1):
        names.append(('up%d' if unpool_type == 'standard' else 'up_conv%d') % p)
        if bn and unpool_type != 'standard':
            names.append('up_conv%d_bn' % p)
    return names


# mma='bf16c8': decoder levels with at least this many input channels materialise DePool2D (ops.unpool_c8) and run
# their conv as a plain layer (0: every level unpools in its conv's patch staging)
C8_UNPOOL_MIN_CIN = int(os.environ.get('IISEG_C8_UNPOOL_MIN_CIN', '1024'))


class _NCHWAdjoint:
    """What `StandardDAE._adjoint_walk` does at a level on fp32 / float64 NCHW maps: the layers' data gradients
    (`StandardDAE.dgrads`), ops.depool_bwd / ops.pool_relu_bwd under the forward's (pre, pooled) tensors and, with
    `gv`, ops.conv_wgrad on the g_z the chain forms and the layer input that `forward_train` saved (DePool2D's
    output is materialised for the up_conv layers, a concat layer is two calls into one dW, h first)."""

    def __init__(self, dae, override, gv):
        # (without `gv` -- backward_y -- every data gradient takes the fp32 flipped-filter form, whatever `dgrad` says)
        self.dae, self.flipped = dae, gv is None
        dae.dgrads.prepare(self.flipped)
        _, self.pre, self.pool = dae._saved
        if any(t.device.type == 'meta' for t in self.pre.values()):
            raise RuntimeError('backward_y needs the pre-pool maps of the forward pass: set '
                               'dae.keep_pre = True before calling scores()')
        self.override, self.gv = override, gv
        if gv is not None:
            self.h_list, _, self.fused = dae._tsaved
            self.feeds = regions.concat_feeds(dae.concat_h, dae.total, dae.n_pool)

    def enter(self, g_score):
        return g_score

    def pre_hw(self, p):
        return self.pre[p].shape[2], self.pre[p].shape[3]

    def pool_hw(self, p):
        return self.pool[p].shape[2], self.pool[p].shape[3]

    def decoder(self, p, g_c):
        """g_c (the gradient w.r.t. up_conv_p's output) -> the gradient w.r.t. the level's pooled-size input."""
        mpre, mpool = self.override[p] if self.override and p in self.override else (self.pre[p], self.pool[p])
        if self.gv is not None:
            t_in = self.pool[self.dae.total] if p == self.dae.total else self.fused['fused_up%d' % (p + 1)]
            ops.conv_wgrad(ops.unpool_eqmask(t_in, mpre, mpool), g_c, *self.gv['up_conv%d' % p], pad=1,
                           mma=self.dae.wgrad)
        g_u = self.dae.dgrads('up_conv%d' % p, g_c, flipped=self.flipped)
        return ops.depool_bwd(g_u, mpre, mpool)

    def encoder(self, p, gp, acc, window, want_data):
        """gp (the gradient w.r.t. pool_p) through max-pool + ReLU and conv_p: + acc (the skip's share, summed in
        place); `window` of the result; nothing is formed without `want_data` (the weight gradients only)."""
        g_z = ops.pool_relu_bwd(gp, self.pre[p], self.pool[p])
        name = 'conv%d_1' % p
        if self.gv is not None:
            fwd, (dW, db) = self.dae.enc[name], self.gv[name]
            ch = 0
            if (p - 1) in self.feeds:                    # h first (P13), then the features
                h = self.h_list[self.feeds[p - 1]]
                ch = h.shape[1]
                ops.conv_wgrad(h, g_z, dW, None, pad=fwd.pad, ci0=0, mma=self.dae.wgrad)
            ops.conv_wgrad(self.pool[p - 1], g_z, dW, db, pad=fwd.pad, ci0=ch, mma=self.dae.wgrad)
        if not want_data:
            return None
        return self.dae.dgrads(name, g_z, acc=acc, window=window, flipped=self.flipped)


class _C8Adjoint:
    """The same two steps on bf16 C8 maps (mma='bf16c8'), from what the C8 forward wrote anyway: per level the
    pooled map and the DePool2D mask bytes (`StandardDAE._saved_c8`).  Every map between two launches is bf16
    (rounded once, at its store, from an fp32 sum); gates and mask selects are exact.
      decoder level : flipped-filter conv, ops.depool_bwd_c8 -- at the deepest level with the ReLU gate of the
                      encoder stage that follows in the same launch;
      encoder level : ops.relu_gate_c8 at pooled resolution (relu'(0) = 0; every position equal to the window
                      maximum receives the gradient: the mask bytes), then the flipped-filter conv whose input
                      staging IS DePool2D of the gated map under the level's own bytes -- or, from
                      C8_UNPOOL_MIN_CIN input channels on, ops.unpool_c8 and a plain conv: the choice the decoder
                      forward makes.  The skip's share enters as the conv's `add` (one fp32 sum, one rounding),
                      into a buffer of its own; the first layer writes fp32 NCHW."""

    def __init__(self, dae):
        if dae._saved_c8 is None:
            raise RuntimeError("backward_y needs the pooled maps and mask bytes of the forward pass: set "
                               "dae.keep_pre = True before calling scores() (mma='bf16c8')")
        self.dae, self.bwd = dae, dae._bwd_convs()
        self.pool8, self.masks, self.hw = dae._saved_c8

    def enter(self, g_score):
        return ops.nchw_to_c8(g_score)

    def pre_hw(self, p):
        return self.hw[p]

    def pool_hw(self, p):
        return self.pool8[p].shape[2], self.pool8[p].shape[3]

    def decoder(self, p, g_c):
        g_u = self.dae.dgrads('up_conv%d' % p, g_c)
        return ops.depool_bwd_c8(g_u, self.masks[p], gate=self.pool8[p] if p == self.dae.total else None)

    def encoder(self, p, gp, acc, window, want_data):
        if not want_data:
            return None
        if p != self.dae.total:                          # (the deepest level arrives gated: `decoder`)
            gp = ops.relu_gate_c8(gp, self.pool8[p], out=gp)
        name = 'conv%d_1' % p
        conv = self.bwd[name]
        kw = dict(window=window)
        if acc is not None:
            kw['add'] = acc
        if p == 1:
            kw['out_format'] = 'nchw'
        ph, pw = self.hw[p]
        if 0 < C8_UNPOOL_MIN_CIN <= conv.Cin and conv.Cout > 16:
            u = torch.zeros(tuple(gp.shape[:2]) + (ph, pw, 8), dtype=torch.bfloat16, device=gp.device)
            return self.dae.dgrads(name, ops.unpool_c8(gp, self.masks[p], u), **kw)
        return self.dae.dgrads(name, gp, mask_in=self.masks[p], unpool_hw=(ph, pw), **kw)


class StandardDAE(Trainable, Views):
    """Callable with (h_1..h_k, y) like the compiled pred_dae_fn (iterative_inference.py:189-190)."""

    kind = 'standard'
    _BUILT = 'a StandardDAE'

    def __init__(self, params, n_classes, concat_h=('pool4',), padding=100, n_filters=64,
                 conv_before_pool=1, additional_pool=2, skip=True, unpool_type='trackind', bn=0,
                 device='cuda', dtype=torch.float32, pad_multi_concat=False, noise=0.0,
                 dropout=0.0, emulate_noise=False, seed=0, mma=None, trainable=False, wgrad='f32',
                 dgrad='f32', fwd='f32'):
        """mma: matrix-pipe operand precision of the float32 path's convolutions ('f32' default,
        'bf16' = 16-bit MFMA operands with fp32 accumulation; ops.Conv).
        trainable=True: the parameters live in ONE flat buffer in `param_order` (W then b per layer), every
        layer holds views of it and runs on the direct / halo kernels only, so that `refresh()` can pack
        them again in place after an optimizer step.
        wgrad: operand precision of `backward`'s 3x3 weight gradients ('f32' default; 'bf16' = operands rounded
        to bf16 for v_mfma_f32_32x32x16_bf16, fp32 accumulation -- float32 trainable modules only; the forward,
        the data gradients, the parameters and db stay float32: DESIGN.md section 15).
        dgrad: operand precision of `backward`'s 3x3 data gradients ('f32' default: the fp32 flipped-filter layers;
        'bf16' = ops.conv_dgrad on the parameters themselves, W and g_z rounded once to bf16, fp32 accumulation --
        float32 trainable modules only; the forward, `backward_y`, the parameters and the masks stay float32:
        DESIGN.md section 16).
        fwd: operand precision of every forward of the module -- `forward_train`, `scores` with and without a
        session, `__call__` / `residual` ('f32' default: every bit, launch and buffer as without the keyword; 'bf16'
        = every encoder and decoder layer an ops.Conv(fwd16=True): z = sum bf16(W) bf16(x) + b (+ the skip addend) on
        conv_halo_bf16_kernel with the pool, DePool2D, the addend's crop, windows and placement in the launch as
        before, fp32 accumulation, fp32 NCHW maps -- float32 trainable modules only; the parameters, the saved maps,
        the pool / ReLU / DePool2D decisions, the loss, `backward`, `backward_y` and the optimizer stay float32:
        DESIGN.md section 20)."""
        concat_h = list(concat_h)
        mma = mma or ops.DEFAULT_MMA
        self.trainable = bool(trainable)
        for switch, mode in (('wgrad', wgrad), ('dgrad', dgrad), ('fwd', fwd)):
            setattr(self, switch, check_mode(switch, mode, dtype, bool(trainable)))
        self._tsaved = None
        if trainable:
            if conv_before_pool != 1 or bn or dropout > 0 or unpool_type not in ('trackind', 'inverse'):
                raise NotImplementedError('training the standard DAE: conv_before_pool=1, bn=0, dropout=0, '
                                          'unpool_type in {trackind, inverse}')
            if dtype not in (torch.float32, torch.float64) or (dtype == torch.float32 and mma != 'f32'):
                raise NotImplementedError("training the standard DAE: float32 (mma='f32') or float64; the "
                                          '16-bit legs are not trained')
            if emulate_noise:
                raise NotImplementedError('training the standard DAE: emulate_noise (DePool2D masks of a hidden '
                                          'noisy re-forward) is not built: the weight gradients take the masks of '
                                          'the training forward itself')
            params = self._store_params(params, param_order(concat_h, conv_before_pool, additional_pool, unpool_type,
                                                            bn), dtype, device)
        self.mma = mma
        # bf16 C8 activations between the layers (ops.Conv mma='bf16c8', `_scores_c8`)
        # ('bf16x3': the same plan on hi / lo pairs, the fp32-class mode of that kernel)
        self.c8 = mma in ('bf16c8', 'bf16x3') and dtype == torch.float32
        self.x3 = self.c8 and mma == 'bf16x3'
        assert all(el in ['pool1', 'pool2', 'pool3', 'pool4', 'input', 'pool5']
                   for el in concat_h)                                   # fcn_down.py:39-41
        if concat_h[-1] == 'input' and additional_pool == 0:
            raise ValueError('It seems your DAE will have no conv/pooling layers!')  # :71-72
        if unpool_type not in ('standard', 'trackind', 'inverse'):
            raise ValueError('Unkown unpool type')                       # fcn_up.py:114-115
        if unpool_type == 'standard' and dtype != torch.float32:
            raise NotImplementedError("unpool_type='standard' (4x4/2 transposed conv) is float32 "
                                      "only")
        self.bn = bool(bn)
        self.enc_bn = {}
        # stochastic-mask emulation (optional): DePool2D's masks from a hidden down-path
        # re-forward with GaussianNoiseLayer / DropoutLayer active, one fresh sample per level
        # (whenever noise > 0 OR dropout > 0: layers/mylayers.py:91-93 drops `deterministic` for
        # every stochastic layer).  Off by default: the deterministic masks are the build's
        # reference semantics -- a documented deviation from the reference whenever noise or
        # dropout is non-zero.
        self.noise, self.dropout = float(noise), float(dropout)
        self.emulate_noise = bool(emulate_noise)
        self.random_source = None     # callable(kind, level, name, shape) -> tensor, or None: torch RNG
        self._seed, self._gen = int(seed), None
        self.dtype = dtype
        self._saved, self._saved_c8 = None, None
        self.unpool_type = unpool_type
        self.concat_h, self.padding, self.skip = concat_h, padding, skip
        self.conv_before_pool = conv_before_pool
        self.n_classes = n_classes
        self.n_pool, self.total = _n_pool(concat_h, additional_pool)
        self.device = device
        self.enc, self.dec = {}, {}
        # (fwd='bf16': the layers say so themselves; a layer built the old way is what it was)
        fwd16 = dict(fwd16=True) if self.fwd == 'bf16' else {}
        for p in range(self.total):
            for i in range(1, conv_before_pool + 1):
                # pad-100 rule of fcn_down.py:90-94
                # pad_multi_concat: build-defined generalisation for several concat points
                # (SURVEY A9', config 5); the reference applies pad-100 only with ONE concat point
                first_pad = (p == 0 and i == 1 and (len(concat_h) == 1 or pad_multi_concat)
                             and concat_h[-1] != 'input' and padding > 0)
                name = 'conv%d_%d' % (p + 1, i)
                self.enc[name] = ops.Conv(params[name][0], params[name][1],
                                          pad=padding if first_pad else 1, relu=True,
                                          device=device, dtype=dtype, mma=mma, **fwd16)        # :102-104
                if bn:   # BatchNormLayer on the rectified conv, stored averages (:112-114)
                    self.enc_bn[name] = tuple(
                        torch.as_tensor(np.asarray(a)).to(dtype).contiguous().to(device)
                        for a in params[name + '_bn'])
        # The conv that follows a concat point computes W_h*h + W_y*features.  h does not change
        # during a refinement loop, so the h half (a per-pixel bias map) is loop-invariant
        # (SURVEY section 7): it is kept as its own linear conv whose output the y half adds in its
        # epilogue.  Same association with or without a session, float32 only (float64 keeps the
        # single-sum form of the oracle).
        self.hsplit = {}
        # (a trainable DAE keeps the two-source form: one parameter view per layer)
        if dtype == torch.float32 and os.environ.get('IISEG_H_SPLIT', '1') != '0' and not trainable:
            prev = n_classes
            for p in range(self.total):
                name = 'conv%d_1' % (p + 1)
                W, b = params[name]
                ch = W.shape[1] - prev
                at = 'input' if p == 0 else 'pool%d' % p
                if ch > 0 and at in concat_h:
                    Wt = torch.as_tensor(W)
                    conv_h = ops.Conv(Wt[:, :ch].contiguous(), b, pad=self.enc[name].pad,
                                      relu=False, device=device, dtype=dtype, mma=mma)
                    conv_y = ops.Conv(Wt[:, ch:].contiguous(), None, pad=self.enc[name].pad,
                                      relu=True, device=device, dtype=dtype, mma=mma)
                    self.hsplit[name] = (conv_h, conv_y)
                prev = params['conv%d_%d' % (p + 1, conv_before_pool)][0].shape[0]
        for p in range(self.total, 0, -1):
            if unpool_type == 'standard':                                # fcn_up.py:41-45
                name = 'up%d' % p
                self.dec[name] = ops.Conv(params[name][0], params[name][1], pad=0, relu=False,
                                          layout='iohw', transposed=True, device=device,
                                          dtype=dtype, mma=mma)
                continue
            name = 'up_conv%d' % p
            W, b = params[name]
            if bn:
                # fcn_up.py:91-93: BatchNormLayer (stored averages) on the LINEAR up_conv, before
                # the skip sum -- an affine per output channel, folded into W and b in float64
                beta, gamma, mean, inv_std = (np.asarray(a, np.float64) for a in params[name + '_bn'])
                sc = gamma * inv_std
                W = np.asarray(W, np.float64) * sc[:, None, None, None]
                b = (np.asarray(b, np.float64) - mean) * sc + beta
            self.dec[name] = ops.Conv(W, b, pad=1, relu=False, device=device,
                                      dtype=dtype, mma=mma, **fwd16)                  # fcn_up.py:83-86
        self.conv_log = None
        # DePool2D fused into the conv's input load (halo kernel: 3 loads per PATCH element;
        # Winograd: applied by the input transform) or materialised first.  None (auto): fused in
        # float32, materialised in float64; True / False force either form.
        env = os.environ.get('IISEG_FUSE_UNPOOL', 'auto')
        self.fuse_unpool = None if env == 'auto' else env != '0'
        # compute each decoder level only on the window that reaches the final crop
        self.dce = os.environ.get('IISEG_DECODER_DCE', '1') != '0'
        # inside a refinement loop recompute only the y-dependent part of the encoder maps
        self.licm = os.environ.get('IISEG_ENCODER_LICM', '1') != '0'
        # keep the weights-only border of the encoder maps across batches (see new_session)
        self.fold_border = os.environ.get('IISEG_DAE_BORDER_FOLD', '1') != '0'
        self._store = None
        self._scratch_sessions = {}   # C8, no provenance records: buffer-stable sessions per geometry (new_session)
        self.trace = None   # set to a dict to keep intermediates (debug / parity tests)
        # DePool2D masks as bytes: where the encoder conv that pools and the decoder conv that
        # unpools both run on halo kernels, the pre-pool map is never stored -- the encoder writes
        # pool + one mask byte per pooled element, the decoder reads up + that byte (`_mask_levels`)
        self.use_masks = os.environ.get('IISEG_DEPOOL_MASKS', '1') != '0'
        self.keep_pre = False   # True: the pre-pool maps are needed afterwards (backward_y)
        if trainable:
            self._hold_views(self.conv_layers().values(), plain=True)
        self.dgrads = DataGrads(self._dgrad_table(), self._refuse_gradient_mode)

    def _mask_levels(self, overridden):
        """Levels (1-based) whose DePool2D mask travels as bytes in this call."""
        if not self.use_masks or overridden or self.keep_pre or self.bn or self.trace is not None or \
                self.unpool_type == 'standard' or self.dtype not in (torch.float32, torch.float64) or \
                self.fuse_unpool is False:
            return frozenset()
        levels = set()
        for L in range(1, self.total + 1):
            name = 'conv%d_%d' % (L, self.conv_before_pool)
            enc = self.enc[name]
            fed_by_h = self.conv_before_pool == 1 and \
                ('input' if L == 1 else 'pool%d' % (L - 1)) in self.concat_h
            if fed_by_h and name in self.hsplit and self._wino_f32(self.hsplit[name][1]):
                # h split off the concat: the y-half conv adds the cached h-half in its epilogue and
                # pools after that add -- the same values the pool kernel would see (the Winograd
                # output transform only: the halo kernels' pooling epilogue takes no add)
                enc, fed_by_h = self.hsplit[name][1], False
            # (the levels of the fp32-NCHW form of `scores`: a Conv built for C8 input answers for the
            # form that runs on NCHW input)
            if fed_by_h or not enc.mask_ok(False) or not self.dec['up_conv%d' % L].mask_ok(False):
                continue
            # halo kernels pool (and write the bytes) in their epilogue; fp32 Winograd layers do at an
            # even tile anchor, else the pool kernel writes the bytes (`scores`)
            if enc.pool_fusable(False) or self._wino_f32(enc):
                levels.add(L)
        return frozenset(levels)

    @staticmethod
    def _wino_f32(conv):
        """The layer runs the fp32 Winograd form (pool + mask bytes in its output transform)."""
        return conv.wino and conv.mma == 'f32' and conv.dtype == torch.float32

    def _conv_pool(self, conv, p, i, t, kw, dep, primed, session, masked, masks, hb=None):
        """Encoder conv i of level p + 1 (hb: the cached h-half of a split concat, added in the
        epilogue).  The last conv of a level on a kernel with a pooling epilogue (halo kernels, fp32
        Winograd at an even tile anchor) also writes pool_p: the window is widened to whole pooling
        windows, the extra row / column recomputed to the values it already has.  Byte-mask levels
        (`_mask_levels`) then write the mask bytes instead of the pre-pool map; where the pool is
        not fused the pool kernel writes them.  Returns (t, fused pooled map or None, mask bytes
        for the pool kernel or None); t is a shape-only stand-in when the map was not stored."""
        pw_ = None
        fh, fw = conv.out_hw(t.shape[2], t.shape[3])
        if i == self.conv_before_pool and not self.bn and (hb is None or self._wino_f32(conv)):
            pw_ = conv.pool_window(t.shape[2], t.shape[3], dep if primed else None, c8=False,
                                   anchor=kw['anchor'])
        fused_pool = None
        if pw_ is not None:
            if primed:
                fused_pool = session['pool%d' % (p + 1)]
                kw.update(window=pw_, place=(pw_[0], pw_[1]))
            else:
                fused_pool = torch.empty((t.shape[0], conv.Cout, fh // 2, fw // 2),
                                         dtype=t.dtype, device=t.device)
            kw['pool_out'] = fused_pool
        if hb is not None:
            kw.update(add=hb, add_off=kw['place'] if 'place' in kw else (0, 0))
        if (p + 1) not in masked or i != self.conv_before_pool:
            return conv(t, **kw), fused_pool, None
        m = session['mask%d' % (p + 1)] if primed else \
            torch.empty((t.shape[0], conv.Cout, fh // 2, fw // 2), dtype=torch.uint8, device=t.device)
        masks[p + 1] = m
        if pw_ is None:                  # (fp32 Winograd at an odd anchor) the pool kernel writes them
            return conv(t, **kw), None, m
        kw.update(mask_out=m, store_out=False)
        conv(t, **kw)
        # the pre-pool map is not stored: a shape-only stand-in from here on
        return torch.empty((t.shape[0], conv.Cout, fh, fw), dtype=t.dtype, device='meta'), fused_pool, None

    def new_session(self, h_list=None, y=None, tags=None):
        """State of one refinement loop (h fixed, y evolving): see `scores`.

        `tags`: one provenance record per h (FCN8.last_provenance: ((store id, geometry),
        image-dependent region)) or None.  When EVERY h comes with the record of a border-folding
        FCN-8 (outside the recorded region the map depends on that net's weights and the geometry
        only), the encoder maps of this DAE have a batch-independent border too: the session of
        the previous batch of the same geometry is handed out again and the first step recomputes
        only the region that y or the image-dependent part of h can reach.  No records (the
        default): a fresh session, every map computed in full on the first step."""
        tags = list(tags) if tags is not None else [None] * len(h_list or [])
        if self.licm and self.fold_border and y is not None and tags and \
                all(t is not None for t in tags):
            key = (tuple(t[0] for t in tags), tuple(y.shape), y.dtype)
            st = self._store
            if st is not None and st.get('key') == key and st.get('primed'):
                st['y8_fresh'] = False       # (a C8 copy of the PREVIOUS loop's last y may be there)
                st['h_fresh'] = True
                st['h_dep'] = [t[1] for t in tags]
                return st
            self._store = {'primed': False, 'key': key}
            return self._store
        if self.c8 and y is not None and h_list is not None and \
                all(isinstance(h, torch.Tensor) for h in h_list):
            # No records, C8 path: nothing of the previous batch may be REUSED, but its buffers can be written
            # again -- the session of this geometry is handed out unprimed (the first step computes every map in
            # full, into the same tensors), so a refinement step captured as a HIP graph on it stays valid for
            # the next batch (api._refine_graph; e.g. the FC-DenseNet host, whose h carries no record).
            key = (tuple(tuple(h.shape) for h in h_list), tuple(y.shape), y.dtype)
            st = self._scratch_sessions.get(key)
            if st is None:
                while len(self._scratch_sessions) >= 2:
                    self._scratch_sessions.pop(next(iter(self._scratch_sessions)))
                st = self._scratch_sessions[key] = {'stable': True}
            else:
                self._scratch_sessions[key] = self._scratch_sessions.pop(key)
            st.update(primed=False, h_stale=True, y8_fresh=False, h_fresh=False)
            return st
        return {'primed': False}

    @property
    def stable_sessions(self):
        """Sessions without provenance records keep their buffers from batch to batch (C8 path): a captured
        refinement step stays valid, so api.refine replays it for short loops too."""
        return bool(self.c8)

    def conv_layers(self):
        d = dict(self.enc)
        d.update(self.dec)
        return d

    def _plan(self, y_shape, primed=False, h_dep=None):
        """regions.dae_plan for this net's layers: the windows of one `scores` call on a y of that
        shape, for both activation layouts.  What depends on a Conv's chosen form (pool_window,
        `_mask_levels`) is decided by the layout's walk, fed from the plan."""
        convs = [(c.pad, c.KH, c.KW, c.dil) for c in
                 (self.enc['conv%d_%d' % (p + 1, i)] for p in range(self.total)
                  for i in range(1, self.conv_before_pool + 1))]
        plan = regions.dae_plan(convs, self.conv_before_pool, self.total, self.n_pool, self.concat_h,
                                (y_shape[2], y_shape[3]), primed, h_dep, self.dce)
        if self.total in plan.feeds:
            raise NotImplementedError('h concatenated at the last pool feeds DePool2D directly '
                                      '(additional_pool=0); not shape-consistent in the reference')
        return plan

    def _h_half(self, name, h, step, session, convert=lambda h: h, **fmt):
        """The h-half of the split conv behind a concat point (a per-pixel bias map the y-half adds in
        its epilogue), kept in the session: computed once per refine(); again in full for the new
        batch of a buffer-stable session (`h_stale`); on the window a fresh h changes when a
        border-folded session is reused (`h_fresh`).  convert / fmt: the layout's form of h and of
        the map.  Returns (map, whether it was allocated by this call)."""
        conv_h = self.hsplit[name][0]
        keep = session is not None and self.licm
        hb = session.get('hb_' + name) if keep else None
        if hb is None:
            hb = conv_h(convert(h), **fmt)
            if keep:
                session['hb_' + name] = hb
            return hb, True
        assert tuple(hb.shape[2:4]) == step.out_hw
        window = (0, 0) + step.out_hw if session.get('stable') and session.get('h_stale') else step.h_window
        if window is not None:
            conv_h(convert(h), window=window, out=hb, place=window[:2], **fmt)
        return hb, False

    def scores(self, h_list, y, mask_override=None, session=None):
        """Runs the DAE up to the pre-softmax score map already cropped to y's size
        (fused_up1 of fcn_up.py:104-113).  Returns score (B, n_classes, H, W).
        `mask_override` {level: (pre, pooled)} substitutes the tensors whose equality defines
        the DePool2D mask of that level (parity tests use it to inject reference masks).
        `session` (a dict from `new_session()`) makes consecutive calls with the SAME h recompute
        only what depends on y (used by the refinement loop)."""
        h_list = list(h_list)
        if len(h_list) != len(self.concat_h):
            raise ValueError('expected %d h tensors, got %d' % (len(self.concat_h), len(h_list)))
        if self.c8:
            if mask_override is not None:
                raise NotImplementedError("mask injection needs fp32 activations (mma='bf16' / 'f32')")
            return self._scores_c8(h_list, y, session)
        t = y
        pre, pool = {}, {0: y}
        # Loop-invariant code motion for the refinement loop: between two steps only y changes, so
        # only the part of every encoder map that y can reach has to be recomputed (the pad-100
        # border and everything fed by h alone keep the values of the first step).  `session`
        # carries the full-size buffers; the plan's `dep` is the y-dependent region of each map.
        primed = session is not None and session.get('primed', False) and self.licm
        will_override = mask_override is not None or (
            self.emulate_noise and (self.noise > 0 or self.dropout > 0) and
            self.unpool_type == 'trackind')
        masked = self._mask_levels(will_override)
        if session is not None:
            if primed and session.get('masked', frozenset()) != masked:
                primed = False               # buffers of the other form: compute everything again
            session['masked'] = masked
            if not primed:
                # the session's buffers are (re)allocated by this call: anything that captured
                # pointers into the previous ones (api._refine_graph) must notice
                session['gen'] = session.get('gen', 0) + 1
        plan = self._plan(y.shape, primed, session['h_dep'] if session is not None and
                          session.get('h_fresh', False) else None)
        masks = {}
        for step in plan.enc:                            # fcn_down.py:77-136
            p, i, dep = step.level, step.i, step.dep
            name = 'conv%d_%d' % (p + 1, i)
            conv = self.enc[name]
            if i == 1:
                fused_pool = pool_mask = None
            kw = dict(anchor=step.ydep[:2])
            if primed:
                assert tuple(session[name].shape[2:]) == step.out_hw
                kw.update(window=dep, out=session[name], place=dep[:2])
            if step.h is not None and name in self.hsplit:
                hb, _ = self._h_half(name, h_list[step.h], step, session)
                t, fused_pool, pool_mask = self._conv_pool(self.hsplit[name][1], p, i, t, kw, dep, primed,
                                                           session, masked, masks, hb=hb)
            elif step.h is not None:                     # h first, then features (P13)
                t = conv(h_list[step.h], x2=t, **kw)
            else:
                t, fused_pool, pool_mask = self._conv_pool(conv, p, i, t, kw, dep, primed, session,
                                                           masked, masks)
            if self.bn:
                ops.bn_affine(t, self.enc_bn[name], window=dep)
            if session is not None and not primed:
                session[name] = t
                if (p + 1) in masks and i == self.conv_before_pool:
                    session['mask%d' % (p + 1)] = masks[p + 1]
            self._count(name, conv, t, computed=dep[2:] if primed else None)
            if i < self.conv_before_pool:
                continue
            pre[p + 1] = t
            if primed:
                buf = session['pool%d' % (p + 1)]
                assert tuple(buf.shape[2:]) == (step.out_hw[0] // 2, step.out_hw[1] // 2)
                t = buf if fused_pool is not None else \
                    ops.maxpool2x2(t, out=buf, window=step.pooled, mask=pool_mask)
            else:
                t = fused_pool if fused_pool is not None else ops.maxpool2x2(t, mask=pool_mask)   # :122
                if session is not None:
                    session['pool%d' % (p + 1)] = t
            pool[p + 1] = t
        if session is not None:
            session['primed'] = True
            session['h_fresh'] = False
        # the hidden re-forward is stochastic whenever ANY stochastic layer is live: Gaussian noise
        # (noise > 0) or the DropoutLayers (dropout > 0, even at noise == 0 -- the configuration of
        # the reference's golden experiment name, plots.ipynb:84: dropout 0.5, z0)
        if self.emulate_noise and (self.noise > 0 or self.dropout > 0) and \
                self.unpool_type == 'trackind' and mask_override is None:
            mask_override = self.hidden_masks(h_list, y)
        if self.unpool_type == 'standard':
            # fcn_up.py:37-63: up_p = Deconv2DLayer(prev, n_cl, 4, stride=2, crop='valid', linear),
            # then ElemwiseSumLayer with pool_{p-1} (center crop) or CroppingLayer.  The 4x4/2
            # transposed conv runs on the static-tap conv kernel; crop + sum are its window + add.
            for p in range(self.total, 0, -1):
                name = 'up%d' % p
                conv = self.dec[name]
                other = pool[p - 1]
                uh, uw = conv.out_hw(t.shape[2], t.shape[3])
                oh, ow = min(uh, other.shape[2]), min(uw, other.shape[3])
                kw = dict(window=(center(uh, oh), center(uw, ow), oh, ow))
                if self.skip and p > 1:
                    kw.update(add=other, add_off=(center(other.shape[2], oh),
                                                  center(other.shape[3], ow)))
                t = conv(t, **kw)
                self._count(name, conv, t, full=(uh, uw))
            return t
        # ---- decoder, fcn_up.py:143-151 / UnpoolNet ------------------------------------------
        # Only the final center crop (fused_up1) is an output, so each level is computed just on
        # the window that reaches it (dead-code elimination, bit-identical results;
        # regions.decoder_windows).  Tensors keep their full-size addressing; windows are written
        # in place (`place`), the rest is never read.
        for p in range(self.total, 0, -1):
            name = 'up_conv%d' % p
            conv = self.dec[name]
            ph, pw, oh, ow, cy, cx = plan.geom[p]
            other = pool[p - 1]                          # pre-concat pool (or the input for p=1)
            y0, x0, nh, nw = plan.need[p]
            mpre, mpool = pre[p], pool[p]
            if mask_override and p in mask_override:
                mpre, mpool = mask_override[p]
            fuse = self.fuse_unpool
            if fuse is None:
                # fused in float32; in float64 where the layer runs in Winograd form (its input
                # transform applies the mask) or on the halo-tile kernel (its patch staging does);
                # materialised for the static-tap float64 kernel
                fuse = conv.dtype == torch.float32 or getattr(conv, 'wino_f64', False) or \
                    (F64_FUSE_UNPOOL and (conv.KH, conv.KW, conv.dil) == (3, 3, 1) and not conv.transposed)
            if not fuse:
                # materialise DePool2D with the HBM-bound kernel and run the plain conv
                u = torch.empty_like(mpre)
                t = ops.unpool_eqmask(t, mpre, mpool, out=u,
                                      window=regions.unpool_reads(plan.geom[p], plan.need[p]))
                mpre = mpool = None
            full = (nh, nw) == (oh, ow)
            out = None if full else torch.empty((y.shape[0], conv.Cout, oh, ow), dtype=y.dtype,
                                                device=y.device)
            kw = dict(pre=mpre, pooled=mpool, window=(cy + y0, cx + x0, nh, nw), out=out,
                      place=None if full else (y0, x0),
                      anchor=(cy + plan.win[p][0], cx + plan.win[p][1]))
            if p in masks:
                kw.update(pre=None, pooled=None, mask_in=masks[p], unpool_hw=(ph, pw))
            if self.skip and p > 1:                      # :96-102 ElemwiseSumLayer, center crop
                kw.update(add=other, add_off=(center(other.shape[2], oh) + y0,
                                              center(other.shape[3], ow) + x0))
            t = conv(t, **kw)                            # else :104-113 CroppingLayer
            self._count(name, conv, t, full=(ph, pw), computed=(nh, nw))
            if self.trace is not None:
                self.trace['fused_up%d' % p] = t
                self.trace['need%d' % p] = plan.need[p]
        if self.trace is not None:
            self.trace.update({'pre%d' % k: v for k, v in pre.items()})
            self.trace.update({'pool%d' % k: v for k, v in pool.items() if k > 0})
        self._saved = (mask_override, pre, pool)      # what backward_y needs (masks only)
        return t

    def c8_feed(self, session):
        """The C8 buffer a fused refinement update may write the new y into for the NEXT `scores`
        call of this session (ops.refine_update(..., y8=)), or None; `c8_fed(session)` afterwards."""
        if not self.c8 or self.x3 or not isinstance(session, dict):
            return None                  # (x3: y is converted to its pair per call, 0.05 ms)
        return session.get('y8')

    def c8_fed(self, session):
        session['y8_fresh'] = True

    def _scores_c8(self, h_list, y, session):
        """`scores` with bf16 C8 activations between the layers (csrc/conv_c8_bf16.hip): the same
        plan (decoder dead-code elimination, loop-invariant encoder maps, border stores) and
        fusions, in the form every level takes here --
          encoder level p : conv3x3 + ReLU whose epilogue writes pool_p (C8) and the DePool2D mask
                            bytes of its windows, taken from the fp32 results; the pre-pool map is
                            never stored (fcn_down.py:102-122);
          decoder level p : conv3x3 whose input staging IS DePool2D (fused_up_{p+1} chunk + mask
                            bytes, layers/mylayers.py:88-115), skip sum with pool_{p-1} and the crop
                            in the epilogue (fcn_up.py:64-113); the last one writes fp32 NCHW scores.
        y arrives fp32 NCHW and is converted once per call; the h half of the conv behind a concat
        point is a cached fp32 C8 addend (loop-invariant, `hsplit`)."""
        # (keep_pre on 'bf16c8': nothing more is stored -- the pooled maps and mask bytes every level writes anyway
        # are what `backward_y` walks on, `_saved_c8` below; the hi / lo pair mode has no backward walk)
        if self.conv_before_pool != 1 or self.bn or self.unpool_type == 'standard' or \
                self.trace is not None or (self.keep_pre and self.x3) or \
                (self.emulate_noise and (self.noise > 0 or self.dropout > 0)):
            raise NotImplementedError("mma='bf16c8' runs the plain trackind / inverse DAE "
                                      "(conv_before_pool=1, bn=0, no trace / gradient mode / noise "
                                      "emulation): use mma='bf16' for those")
        B, dev = y.shape[0], y.device
        primed = session is not None and session.get('primed', False) and self.licm
        if session is not None:
            if primed and session.get('masked') != 'c8':
                primed = False
            session['masked'] = 'c8'
        # (`gen` tells a captured graph that buffers were allocated anew; a buffer-stable session -- new_session
        # without records -- writes the tensors it already has)
        stable = session is not None and session.get('stable', False)
        realloc = session is not None and not primed and not stable
        plan = self._plan(y.shape, primed, session['h_dep'] if session is not None and
                          session.get('h_fresh', False) else None)
        # y as a C8 tensor: converted here, unless the refinement step that produced y has already
        # written it (`c8_feed`: api passes the session's buffer to ops.refine_update)
        y8 = session.get('y8') if session is not None else None
        if y8 is not None and tuple(y8.shape[2:4]) != tuple(y.shape[2:4]):
            y8 = None
        if y8 is not None and session.get('y8_fresh'):
            t = y8
        else:
            t = ops.nchw_to_c8(y, out=y8 if y8 is not None and y8.shape[0] == B else None, x3=self.x3)
            if session is not None:
                session['y8'] = t
        if session is not None:
            session['y8_fresh'] = False
        to_c8 = lambda h: ops.nchw_to_c8(h, x3=self.x3)
        pool8, masks = {}, {}
        for step in plan.enc:                            # fcn_down.py:77-136
            p, (fh, fw) = step.level, step.out_hw
            name = 'conv%d_1' % (p + 1)
            conv = self.enc[name]
            kw = {}
            if primed:
                kw['window'] = conv.pool_window(t.shape[2], t.shape[3], step.dep)
                pooled_t, m = session['pool%d' % (p + 1)], session['mask%d' % (p + 1)]
            else:
                pooled_t = m = None
                if stable:
                    pooled_t, m = session.get('pool%d' % (p + 1)), session.get('mask%d' % (p + 1))
                    nch = ops.c8_chunks(conv.Cout)
                    if pooled_t is None or m is None or \
                            tuple(pooled_t.shape) != (B, nch * (2 if self.x3 else 1), fh // 2, fw // 2, 8) or \
                            tuple(m.shape) != (B, nch, fh // 2, fw // 2, 8):
                        pooled_t = m = None
                if pooled_t is None:
                    pooled_t = ops.empty_c8(B, conv.Cout, fh // 2, fw // 2, dev, x3=self.x3)
                    m = ops.empty_c8(B, conv.Cout, fh // 2, fw // 2, dev, dtype=torch.uint8)
                    realloc = realloc or stable
            kw.update(pool_out=pooled_t, mask_out=m, store_out=False)
            if step.h is not None and name in self.hsplit:
                hb, fresh = self._h_half(name, h_list[step.h], step, session, to_c8, out_format='c8f32')
                realloc = realloc or (fresh and stable)
                off = (kw['window'][0], kw['window'][1]) if 'window' in kw else (0, 0)
                self.hsplit[name][1](t, add=hb, add_off=off, **kw)
            elif step.h is not None:                     # h first, then features (P13)
                if self.x3:
                    raise NotImplementedError("mma='bf16x3' needs the h-split form of a concat "
                                              "point (hsplit=True)")
                conv(ops.nchw_to_c8(h_list[step.h]), x2=t, **kw)
            else:
                conv(t, **kw)
            if session is not None and not primed:
                session['pool%d' % (p + 1)], session['mask%d' % (p + 1)] = pooled_t, m
            if self.conv_log is not None:
                cw_ = kw['window'] if 'window' in kw else (0, 0, fh, fw)
                self.conv_log.append((name, conv.flops(B, fh, fw), conv.flops(B, cw_[2], cw_[3])))
            t = pool8[p + 1] = pooled_t
            masks[p + 1] = m
        if session is not None:
            session['primed'] = True
            session['h_fresh'] = False
            session['h_stale'] = False
            if realloc:
                session['gen'] = session.get('gen', 0) + 1
        # ---- decoder, fcn_up.py:143-151 (windows as in `scores`) -------------------------------
        for p in range(self.total, 0, -1):
            name = 'up_conv%d' % p
            conv = self.dec[name]
            ph, pw, oh, ow, cy, cx = plan.geom[p]
            y0, x0, nh, nw = plan.need[p]
            full = (nh, nw) == (oh, ow)
            out = None
            if not full:
                out = torch.empty((B, conv.Cout, oh, ow), dtype=torch.float32, device=dev) if p == 1 \
                    else ops.empty_c8(B, conv.Cout, oh, ow, dev, x3=self.x3)
            kw = dict(mask_in=masks[p], unpool_hw=(ph, pw), window=(cy + y0, cx + x0, nh, nw),
                      out=out, place=None if full else (y0, x0),
                      out_format='nchw' if p == 1 else 'c8')
            if self.skip and p > 1:                      # :96-102 ElemwiseSumLayer, center crop
                oth = pool8[p - 1].shape[2:4]
                kw.update(add=pool8[p - 1], add_off=(center(oth[0], oh) + y0, center(oth[1], ow) + x0))
            if 0 < C8_UNPOOL_MIN_CIN <= conv.Cin and not self.x3 and conv.Cout > 16:
                # Deep levels: DePool2D materialised first (a few tens of MB at these sizes), the conv then runs
                # as a PLAIN layer -- LDS-DMA patch staging instead of up chunk + mask bytes selected through
                # registers by every output-channel tile of every pixel tile (same values: bit-identical).  The
                # map is kept per session (rows / columns past the last pooling window stay zero).
                skey = 'unp%d' % p
                u = session.get(skey) if session is not None else None
                if u is None or tuple(u.shape) != (B, t.shape[1], ph, pw, 8):
                    u = torch.zeros((B, t.shape[1], ph, pw, 8), dtype=torch.bfloat16, device=dev)
                    if session is not None:
                        session[skey] = u
                ops.unpool_c8(t, masks[p], u, window=regions.unpool_reads_pooled(plan.geom[p], plan.need[p]))
                kw.pop('mask_in'); kw.pop('unpool_hw')
                t = conv(u, **kw)
            else:
                t = conv(t, **kw)                        # else :104-113 CroppingLayer
            if self.conv_log is not None:
                self.conv_log.append((name, conv.flops(B, ph, pw), conv.flops(B, nh, nw)))
        self._saved = None
        # what backward_y needs of this call: {level: pooled C8 map}, {level: mask bytes} (with a session: the
        # session's buffers, valid until its next `scores`) and the pre-pool sizes
        self._saved_c8 = (pool8, masks, {step.level + 1: step.out_hw for step in plan.enc}) if self.keep_pre \
            else None
        return t

    def saved_c8(self):
        """{'pool%d': bf16 C8 map, 'mask%d': DePool2D mask bytes (B, C/8, h, w, 8)} per level, as the latest
        `scores` call of a C8 module with `keep_pre` left them (the tensors themselves, not copies); for tests."""
        if self._saved_c8 is None:
            raise RuntimeError("no C8 maps kept: mma='bf16c8' and dae.keep_pre = True before scores()")
        pool8, masks, _ = self._saved_c8
        out = {'pool%d' % k: v for k, v in pool8.items()}
        out.update({'mask%d' % k: v for k, v in masks.items()})
        return out

    # ---- true-gradient mode (not in the reference, F1) -----------------------
    def _dgrad_table(self):
        """[(name, how the layer's data gradient is formed)] (datagrads.Layer), encoder then decoder.  Backward-data
        of a 3x3 stride-1 conv = the forward conv of the gradient with the flipped filter ('same' for pad 1; for the
        pad-100 first layer the window at offset pad-1 of that 'same' result).  After a concat only the filters of
        the non-h channels are kept: h is a constant of the loop.  dgrad='bf16': ops.conv_dgrad on the layer's own
        parameter -- after a concat the feature channels only -- in `backward`; `backward_y` forces the flipped form.
        (A C8 module's layers are built for C8 input explicitly -- mma='bf16c8', whatever ops.DEFAULT_MMA says: the
        flipped weights are rounded to bf16 when they are packed; no bias.)"""
        kw = dict(pad=1, dtype=self.dtype, **(dict(mma='bf16c8') if self.c8 else {}))
        op = 'conv_dgrad' if self.dgrad == 'bf16' else None
        table, prev = [], self.n_classes
        for p in range(self.total):
            conv = self.enc['conv%d_1' % (p + 1)]        # W (Cout, ch + prev, 3, 3), on the device
            table.append(('conv%d_1' % (p + 1), Layer(lambda conv=conv, prev=prev: flipped(conv.W[:, conv.Cin - prev:]),
                                                      kw, self.trainable, 0, op, conv, conv.Cin - prev, prev)))
            prev = conv.Cout
        for p in range(self.total, 0, -1):
            conv = self.dec.get('up_conv%d' % p)         # (unpool_type='standard' has none: `_refuse_gradient_mode`)
            table.append(('up_conv%d' % p, Layer(lambda conv=conv: flipped(conv.W), kw, self.trainable, 0, op, conv, 0,
                                                 conv and conv.Cin)))
        return table

    def _refuse_gradient_mode(self):
        if self.conv_before_pool != 1 or self.bn or self.unpool_type == 'standard':
            raise NotImplementedError('gradient mode: conv_before_pool=1, bn=0, unpool_type in '
                                      '{trackind, inverse}')

    def _adjoint_walk(self, g_score, y_shape, override=None, gv=None, first_layer=True):
        """The adjoint of the latest `scores()` call, level by level (oracle/dae_grad.py), on full maps (the
        decoder / encoder windows of the forward are not exploited here): `backward_y` and `backward` are its two
        callers.  The level structure, the crop / skip geometry and the order of the sums are written here, once;
        what a level does to its maps is the layout's business: `_NCHWAdjoint` (fp32 / float64 NCHW maps, the
        forward's pre-pool and pooled maps as masks, optionally the weight gradients) or `_C8Adjoint` (bf16 C8
        maps, the forward's pooled maps and mask bytes).  override: the forward's {level: (pre, pooled)} DePool2D
        mask tensors.  gv: {name: (dW, db)} to take the weight gradients into.  first_layer: form (and return) the
        first layer's data gradient."""
        lv = _C8Adjoint(self) if self.c8 else _NCHWAdjoint(self, override, gv)
        g_pool = {}
        g_f = lv.enter(g_score)
        for p in range(1, self.total + 1):               # decoder, output to input
            ph, pw = lv.pre_hw(p)
            other_hw = lv.pool_hw(p - 1) if p > 1 else (y_shape[2], y_shape[3])
            oh, ow = min(ph, other_hw[0]), min(pw, other_hw[1])
            g_c = _embed(g_f, (ph, pw), (center(ph, oh), center(pw, ow)))          # adjoint of the center crop
            if self.skip and p > 1:                                                 # adjoint of the skip sum
                g_pool[p - 1] = _embed(g_f, other_hw, (center(other_hw[0], oh), center(other_hw[1], ow)))
            g_f = lv.decoder(p, g_c)
        g_pool[self.total] = g_f
        g_in = None
        for p in range(self.total, 0, -1):               # encoder, deep to shallow
            pad = self.enc['conv%d_1' % p].pad
            if p > 1:
                g_pool[p - 1] = lv.encoder(p, g_pool[p], g_pool.get(p - 1), None, True)
            else:                 # pad-100 first layer: the window at offset pad - 1 of the 'same' result
                g_in = lv.encoder(p, g_pool[p], None, None if pad == 1 else
                                  (pad - 1, pad - 1, y_shape[2], y_shape[3]), first_layer)
        return g_in

    def backward_y(self, g_score, y_shape):
        """dE/dy THROUGH the DAE for an upstream gradient g_score w.r.t. the (cropped) score map
        of the latest `scores()` call (`_adjoint_walk` under the mask override of that call).  fp32 NCHW in and
        out on every leg; a C8 module (mma='bf16c8') walks on bf16 C8 gradient maps in between: g_score is rounded
        to bf16 on its way in, every map between two layers is, the first layer's data gradient leaves as fp32."""
        return self._adjoint_walk(g_score, y_shape, override=None if self.c8 else self._saved[0])

    # ---- training (reference train_dae.py with dae kind 'standard') ----------
    def forward_train(self, h_list, y, noise=0.0, generator=None, eps=None):
        """The training-mode forward: GaussianNoiseLayer on y (y + noise * N(0, 1) formed ONCE, `eps` = the
        caller's standard-normal sample, else drawn from `generator`), then `scores` on full maps with the
        pre-pool maps kept; the DePool2D masks are those of this same noisy forward (one sample per step:
        DESIGN.md section 4).  Returns the score map before the softmax."""
        self._need_trainable('forward_train')
        h_list = list(h_list)
        y = ops.gaussian_noise(y, noise, generator, eps)
        keep, dce, trace = self.keep_pre, self.dce, self.trace
        # full decoder maps: the weight gradient reads every layer input whole
        self.keep_pre, self.dce, self.trace = True, False, {}
        try:
            score = self.scores(h_list, y)
            fused = self.trace
        finally:
            self.keep_pre, self.dce, self.trace = keep, dce, trace
        self._tsaved = (h_list, tuple(y.shape), fused)
        return score

    def saved_maps(self):
        """What the last `forward_train` kept, under the names of oracle/dae.py's net: 'input' (the noisy y),
        'pre%d', 'pool%d', 'fused_up%d'; for tests."""
        _, pre, pool = self._saved
        out = {'input': pool[0]}
        out.update({'pre%d' % k: v for k, v in pre.items()})
        out.update({'pool%d' % k: v for k, v in pool.items() if k > 0})
        out.update({k: v for k, v in self._tsaved[2].items() if k.startswith('fused_up')})
        return out

    def backward(self, g_score):
        """{name: (dW, db)} (views of one flat gradient buffer laid out as `self.flat`) for dL/dscore =
        g_score, after `forward_train`: `_adjoint_walk` with ops.conv_wgrad at every layer.  The data gradient
        of the first layer is not formed.  dgrad='bf16': the data gradients by ops.conv_dgrad (`_dgrad_table`)."""
        self._need_trainable('backward')
        if self._tsaved is None or self._saved is None:
            raise RuntimeError('backward() needs forward_train() first')
        gv = self._params.grad_views()
        self._adjoint_walk(g_score, self._tsaved[1], gv=gv, first_layer=False)
        return gv

    def refresh(self):
        """The parameters (`self.flat`) have been changed in place: every layer packs its weights again into
        the buffers it already has, the data-gradient layers take the flipped filters again, and sessions
        that cached maps of the old weights are dropped.  No host wait."""
        self._need_trainable('refresh')
        for conv in self.conv_layers().values():
            conv.refresh()
        self.dgrads.refresh()
        self._store = None
        self._scratch_sessions.clear()

    def _rand(self, kind, level, name, shape, like):
        if self.random_source is not None:
            t = self.random_source(kind, level, name, tuple(shape))
            return torch.as_tensor(t).to(like.dtype).contiguous().to(like.device)
        if self._gen is None:
            self._gen = torch.Generator(device=like.device)
            self._gen.manual_seed(self._seed)
        if kind == 'noise':
            return torch.randn(shape, generator=self._gen, device=like.device, dtype=like.dtype)
        u = torch.rand(shape, generator=self._gen, device=like.device, dtype=like.dtype)
        return (u >= self.dropout).to(like.dtype)     # keep mask

    def hidden_masks(self, h_list, y):
        """{level: (pre, pooled)} as DePool2D sees them when dae_dict['noise'] > 0 or
        dae_dict['dropout'] > 0: every DePool2D
        calls lasagne.layers.get_output([pool_in, pool]) WITHOUT deterministic=True
        (layers/mylayers.py:91-93), i.e. a fresh forward of the down path up to its level with
        GaussianNoiseLayer (fcn_down.py:60-63) and the DropoutLayers (:108-111) active.  The
        main path (the values that are unpooled) stays deterministic."""
        if self.bn:
            raise NotImplementedError('noise emulation with bn=1 (batch statistics in the hidden '
                                      'forward) is not supported')
        masks = {}
        feeds = regions.concat_feeds(self.concat_h, self.total, self.n_pool)
        for p in range(self.total, 0, -1):
            # GaussianNoiseLayer(sigma=0) adds nothing (and draws nothing worth emulating)
            t = ops.add_noise(y, self._rand('noise', p, None, y.shape, y), self.noise) \
                if self.noise > 0 else y
            for q in range(p):
                for i in range(1, self.conv_before_pool + 1):
                    name = 'conv%d_%d' % (q + 1, i)
                    conv = self.enc[name]
                    h = feeds.get(q) if i == 1 else None
                    t = conv(h_list[h], x2=t) if h is not None else conv(t)
                    if self.dropout > 0:
                        ops.dropout_apply(t, self._rand('dropout', p, name, t.shape, t), self.dropout)
                pre_q = t
                t = ops.maxpool2x2(t)
            masks[p] = (pre_q, t)
        return masks

    def _count(self, name, conv, out, full=None, computed=None):
        # (name, nominal FLOPs of the FULL layer output, FLOPs of the computed window)
        if self.conv_log is not None:
            oh, ow = full if full is not None else (out.shape[2], out.shape[3])
            ch, cw = computed if computed is not None else (out.shape[2], out.shape[3])
            self.conv_log.append((name, conv.flops(out.shape[0], oh, ow),
                                  conv.flops(out.shape[0], ch, cw)))

    def __call__(self, *args):
        """pred_dae_fn(h..., y) -> r  (softmax output, models/fcn_up.py:154-169)."""
        h_list, y = args[:-1], args[-1]
        score = self.scores(h_list, y)
        return ops.crop_softmax(score, score.shape[2], score.shape[3], off=(0, 0))

    def residual(self, *args):
        """de_fn(h..., y) = -(r - y) = y - r  (iterative_inference.py:203-204)."""
        h_list, y = args[:-1], args[-1]
        score = self.scores(h_list, y)
        return ops.crop_softmax(score, score.shape[2], score.shape[3], off=(0, 0), minuend=y)


def buildDAE(input_concat_h_vars=None, input_mask_var=None, n_classes=11,
             nb_features_to_concat=None, padding=100, ae_h=False, void_labels=(),
             path_weights=None, model_name='dae_model.npz', trainable=False, load_weights=False,
             out_nonlin='softmax', concat_h=('input',), noise=0.1, n_filters=64,
             conv_before_pool=1, additional_pool=0, dropout=0., skip=False,
             unpool_type='standard', bn=0, params=None, device='cuda', dtype=torch.float32,
             emulate_noise=False):
    """Mirror of models/DAE_h.py:12-20.  Inference only: `noise`, `dropout` are identities at
    deterministic=True (P8, P9); the DePool2D masks are the deterministic ones unless
    `emulate_noise` asks for the reference's noisy hidden re-forward; the symbolic
    `input_*_var`, `trainable`, `ae_h`, `void_labels` are accepted and ignored."""
    if params is None:
        if not (load_weights and path_weights):
            raise ValueError('buildDAE needs `params` or `path_weights`')
        order = param_order(concat_h, conv_before_pool, additional_pool, unpool_type, bn)
        params = load_param_list(os.path.join(path_weights, model_name), order)  # DAE_h.py:52-57
    if out_nonlin not in ('softmax',):
        raise NotImplementedError('inference uses out_nonlin=softmax (iterative_inference.py:158)')
    return StandardDAE(params, n_classes, concat_h=concat_h, padding=padding, n_filters=n_filters,
                       conv_before_pool=conv_before_pool, additional_pool=additional_pool,
                       skip=skip, unpool_type=unpool_type, bn=bn, device=device, dtype=dtype,
                       noise=noise, dropout=dropout, emulate_noise=emulate_noise)
