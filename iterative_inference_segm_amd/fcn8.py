"""FCN-8s segmentation network on the HIP kernels (mirror of reference models/fcn8.py).

`buildFCN8(...)` keeps the reference's argument names (models/fcn8.py:16-23) where they make
sense without Theano: there is no symbolic `input_var`; the returned object is called with
the image batch and returns `[net[el] for el in layer]` (models/fcn8.py:200), i.e. it plays
the role of the compiled `pred_fcn_fn` (iterative_inference.py:187-188).
"""
import itertools
import os

import numpy as np
import torch

from . import ops
from .datagrads import DataGrads, Layer, Views, flipped
from .params import Trainable, check_mode
from .regions import center, conv_region, pool_region
from .weights import load_param_list

PARAM_ORDER = ['conv1_1', 'conv1_2', 'conv2_1', 'conv2_2', 'conv3_1', 'conv3_2', 'conv3_3',
               'conv4_1', 'conv4_2', 'conv4_3', 'conv5_1', 'conv5_2', 'conv5_3',
               'fc6', 'fc7', 'score_fr', 'score2', 'score_pool4', 'score4', 'score_pool3',
               'upsample']  # lasagne get_all_param_values order

_BLOCKS = [('conv1_1', 'conv1_2'), ('conv2_1', 'conv2_2'), ('conv3_1', 'conv3_2', 'conv3_3'),
           ('conv4_1', 'conv4_2', 'conv4_3'), ('conv5_1', 'conv5_2', 'conv5_3')]
_NAMES_3X3 = frozenset(n for names in _BLOCKS for n in names)
_NAMES_KXK16 = ('fc6', 'fc7')                            # the layers of kxk='bf16'
_NAMES_FWD16 = tuple(sorted(_NAMES_3X3)) + _NAMES_KXK16  # the fifteen layers of fwd='bf16'


_UID = itertools.count(1)   # identity of a net in the provenance tags (never reused, unlike id())


class FCN8(Trainable, Views):
    _BUILT = 'an FCN8'

    def __init__(self, params, n_classes, layer=('probs_dimshuffle',), pad=100, temperature=1.0,
                 device='cuda', dtype=torch.float32, mma=None, trainable=False, dropout=0.5, wgrad='f32',
                 dgrad='f32', kxk='f32', fwd='f32'):
        """mma: matrix-pipe operand precision of the float32 path's convolutions ('f32' default,
        'bf16' = 16-bit MFMA operands with fp32 accumulation; 'bf16c8' = additionally bf16 C8
        activations between the 3x3 layers, the h maps handed out stay fp32 NCHW; ops.Conv).
        trainable=True (float32 with mma='f32', or float64; temperature 1): the parameters live in ONE flat
        buffer in PARAM_ORDER (W then b per layer), every layer holds views of it and runs on the direct / halo /
        tap kernels only, so that `refresh()` can pack them again in place after an optimizer step; every map is
        computed whole (no border fold, no session).  `dropout`: p of the DropoutLayers behind fc6 and fc7 in
        `forward_train`.
        wgrad: operand precision of `backward`'s thirteen 3x3 weight gradients ('f32' default; 'bf16' = operands
        rounded to bf16 for v_mfma_f32_32x32x16_bf16, fp32 accumulation -- float32 trainable modules only; fc6,
        fc7, the score and transposed layers, the forward and the data gradients stay float32: DESIGN.md
        section 15).
        dgrad: operand precision of `backward`'s twelve 3x3 data gradients ('f32' default: the fp32 flipped-filter
        layers; 'bf16' = ops.conv_dgrad on the parameters themselves, W and g_z rounded once to bf16, fp32
        accumulation, the ReLU gate that follows inside a block in the same launch -- float32 trainable modules
        only; fc6, fc7, the score and transposed layers and the forward stay float32: DESIGN.md section 16).
        kxk: operand precision of `backward`'s weight and data gradients of the two wide 'valid' layers fc6 (7x7)
        and fc7 (1x1) ('f32' default; 'bf16' = ops.conv_wgrad_kxk(mma='bf16') and ops.conv_dgrad_kxk on the
        parameters themselves, every operand rounded once to bf16, fp32 accumulation, no flipped fp32 copy of
        either filter -- float32 trainable modules only; the 11-channel score layers, the transposed layers and
        the forward stay float32: DESIGN.md section 17).  Independent of wgrad and dgrad.
        fwd: operand precision of `forward_train`'s thirteen 3x3 layers, fc6 and fc7, with and without
        deterministic=True ('f32' default; 'bf16' = z = relu(sum bf16(W) bf16(x) + b), every operand rounded once
        to bf16 as it is staged, fp32 accumulation in a fixed order, the bias added in fp32, the map stored as fp32
        NCHW: the 3x3 layers on conv_halo_bf16_kernel at every size, fc6 / fc7 by ops.conv_fwd_kxk on the
        parameters themselves -- float32 trainable modules only; parameters, saved maps, the ReLU / pool / dropout
        decisions (taken on the fp32 values this forward stores), the score and transposed layers, maxpool2x2 and
        `backward` stay float32 and the same code: DESIGN.md section 18).  Independent of wgrad, dgrad and kxk."""
        self.trainable = bool(trainable)
        self.dropout = float(dropout)
        for switch, mode in (('wgrad', wgrad), ('dgrad', dgrad), ('kxk', kxk), ('fwd', fwd)):
            setattr(self, switch, check_mode(switch, mode, dtype, bool(trainable)))
        self._tsaved = None
        if trainable:
            # refused here, before any device work
            if dtype not in (torch.float32, torch.float64) or \
                    (dtype == torch.float32 and (mma or ops.DEFAULT_MMA) != 'f32'):
                raise NotImplementedError("training FCN-8: float32 (mma='f32') or float64; the 16-bit legs "
                                          '(mma=%r) are not trained' % (mma or ops.DEFAULT_MMA,))
            if float(temperature) != 1.0:
                raise NotImplementedError('training FCN-8: temperature must be 1 (it divides upsample.W and '
                                          'upsample.b, which are parameters here)')
            if not 0.0 <= self.dropout < 1.0:
                raise ValueError('dropout must be in [0, 1)')
            params = self._store_params(params, PARAM_ORDER, dtype, device)
        if mma is None:
            # IISEG_MMA=bf16x3 means "the DAE loop on hi / lo pairs"; this net takes the pair form
            # only when asked by name (tests/test_gpu_x3.py: the FCN-8 in fp32 keeps the mode's parity)
            mma = 'f32' if ops.DEFAULT_MMA == 'bf16x3' else ops.DEFAULT_MMA
        # ('bf16x3': the same C8 plan on hi / lo pairs -- the 3x3 layers' fp32-class mode; fc6 / fc7 and
        # the 1x1 score layers then run their fp32 kernels)
        self.c8 = mma in ('bf16c8', 'bf16x3') and dtype == torch.float32
        self.x3 = self.c8 and mma == 'bf16x3'
        self.layer = list(layer)
        self.n_classes = n_classes
        self.pad = pad
        self.device = device
        self.dtype = dtype
        p = params
        # (fwd='bf16': the fifteen layers say so themselves; a layer built the old way is what it was)
        c = lambda name, pad_, relu=True: ops.Conv(p[name][0], p[name][1], pad=pad_, relu=relu,
                                                   device=device, dtype=dtype, mma=mma,
                                                   fwd16=(fwd == 'bf16' and name in _NAMES_FWD16))
        self.convs = {}
        for bi, names in enumerate(_BLOCKS):
            for ni, name in enumerate(names):
                # models/fcn8.py:34-35: pad=100 on conv1_1, 'same' elsewhere
                self.convs[name] = c(name, pad if (bi == 0 and ni == 0) else 1)
        self.convs['fc6'] = c('fc6', 0)            # :75-76 7x7 valid, default ReLU
        self.convs['fc7'] = c('fc7', 0)            # :80-81
        self.convs['score_fr'] = c('score_fr', 0)  # :84-85 default nonlinearity = ReLU (P2)
        self.convs['score_pool4'] = c('score_pool4', 0)  # :92-93 1x1, ReLU (P2)
        self.convs['score_pool3'] = c('score_pool3', 0)  # :102-103
        self.score2 = ops.Deconv(p['score2'][0], p['score2'][1], 2, device=device, dtype=dtype)    # :90-91
        self.score4 = ops.Deconv(p['score4'][0], p['score4'][1], 2, device=device, dtype=dtype)    # :100-101
        Wu, bu = p['upsample']
        if trainable:
            self.upsample = ops.Deconv(Wu, bu, 8, device=device, dtype=dtype)
        else:
            # temperature divides upsample.W and upsample.b (:194-198)
            self.upsample = ops.Deconv(np.asarray(Wu) / temperature, np.asarray(bu) / temperature, 8,
                                       device=device, dtype=dtype)                                  # :109-110
        self.conv_log = None  # optional list collecting (name, flops) per conv launch
        # fold the weights-only pad-100 border of the encoder maps once per input geometry
        self.fold_border = os.environ.get('IISEG_FCN_BORDER_FOLD', '1') != '0' and not trainable
        self._border = {}
        if trainable:
            self._hold_views(self.convs.values(), plain=True)
            self._hold_views([self.score2, self.score4, self.upsample])
        self.dgrads = DataGrads(self._dgrad_table())
        # kxk='bf16': the operand precision of fc6's / fc7's weight gradients (the other 'valid' layers' stay fp32)
        self._wgrad_kxk = {name: kxk if name in _NAMES_KXK16 else 'f32' for name in self.convs}
        self._uid = next(_UID)
        self.last_provenance = None   # per output of the latest forward: (store id, region) or None

    def conv_layers(self):
        return self.convs

    def __call__(self, x):
        return self.forward(x)

    def forward(self, x, hs=None, session=None):
        """hs: optional {concat point: h tensor} -- the buildFCN8_DAE wiring
        (models/fcn8_dae.py:52-54,63-65,...): h is concatenated FIRST in front of the conv that
        follows the concat point; fused as a two-source gather, never materialised.

        `session` (a dict, see `new_session`) keeps the full-size encoder maps between calls whose
        only difference is `x` (same hs, same weights): a primed call recomputes just the region
        of every map that x can reach; the pad-100 border, a function of the weights (and hs)
        alone, keeps its values.  Bit-identical to the full computation."""
        hs = hs or {}
        own = False
        if session is None and self.fold_border and not hs:
            # plain FCN-8: the border depends on the weights only, so it is folded once per
            # input geometry (like weight packing) and reused for every later batch
            key = (tuple(x.shape), x.dtype)
            if self._border.get('key') != key:
                self._border = {'key': key, 'primed': False}
            session, own = self._border, True
        primed = session is not None and session.get('primed', False)
        net = {'input': x}
        t = x
        c8 = self.c8 and not hs
        if c8:
            t = ops.nchw_to_c8(x, x3=self.x3)      # bf16 C8 from here to pool5 (conv_c8_bf16.hip)
        dep = (0, 0, x.shape[2], x.shape[3])       # region of `t` that depends on x
        deps = {}
        pending = hs.get('input')
        for bi, names in enumerate(_BLOCKS):
            fused_pool = None
            for name in names:
                conv = self.convs[name]
                fh, fw = conv.out_hw(t.shape[2], t.shape[3])
                dep = conv_region(dep, conv, fh, fw)
                # Winograd tiles anchored at the parity of the region recomputed per batch
                kw = dict(anchor=(dep[0], dep[1]))
                if primed:
                    kw.update(window=dep, out=session[name], place=(dep[0], dep[1]))
                if name == names[-1] and pending is None:
                    # last conv of the block on the halo kernel (or an fp32 Winograd layer at an even
                    # tile anchor): the pool rides in its epilogue
                    pw_ = conv.pool_window(t.shape[2], t.shape[3], dep if primed else None, c8=c8,
                                           anchor=kw['anchor'])
                    if pw_ is not None:
                        if primed:
                            fused_pool = session['pool%d' % (bi + 1)]
                            kw.update(window=pw_, place=(pw_[0], pw_[1]))
                        elif c8:
                            fused_pool = ops.empty_c8(t.shape[0], conv.Cout, fh // 2, fw // 2, t.device,
                                                      x3=self.x3)
                        else:
                            fused_pool = torch.empty((t.shape[0], conv.Cout, fh // 2, fw // 2),
                                                     dtype=t.dtype, device=t.device)
                        kw['pool_out'] = fused_pool
                        if c8:
                            # C8: nothing reads the pre-pool map of a block's last conv
                            kw = dict(pool_out=fused_pool, store_out=False)
                            if primed:
                                kw['window'] = pw_
                if pending is not None:
                    t = self._conv(name, pending, x2=t, **kw)
                    pending = None
                else:
                    t = self._conv(name, t, **kw)
                if session is not None and not primed:
                    session[name] = t
            pname = 'pool%d' % (bi + 1)
            dep = pool_region(dep, fh // 2, fw // 2)
            if fused_pool is not None:
                t = fused_pool
                if session is not None and not primed:
                    session[pname] = t
            elif primed:
                t = ops.maxpool2x2(t, out=session[pname], window=dep)   # :38,45,54,63,72
            else:
                t = ops.maxpool2x2(t)
                if session is not None:
                    session[pname] = t
            net[pname] = t
            deps[pname] = dep
            pending = hs.get(pname)
        if session is not None:
            session['primed'] = True
        if c8:
            # the h maps of the API, the 1x1 score layers and fc6 take fp32 NCHW
            f32 = {k: ops.c8_to_nchw(v, self.convs[_BLOCKS[int(k[-1]) - 1][-1]].Cout, x3=self.x3)
                   for k, v in net.items() if k.startswith('pool') and
                   (k in self.layer or k in ('pool3', 'pool4'))}
            net.update(f32)
            t = ops.c8_to_nchw(t, self.convs['conv5_3'].Cout, x3=self.x3)
        if pending is not None:          # concat after pool5 feeds fc6 (7x7: table kernel)
            t = self._conv('fc6', pending, x2=t)
        else:
            t = self._conv('fc6', t)   # dropout = identity at deterministic=True (P8)
        t = self._conv('fc7', t)
        t = self._conv('score_fr', t)
        # score_fused = score2 + score_pool4, both center-cropped to the common size (:94-97)
        t = self._deconv_sum(self.score2, t, 'score_pool4', net['pool4'])
        # score_final = score4 + score_pool3 (:104-107)
        t = self._deconv_sum(self.score4, t, 'score_pool3', net['pool3'])
        # upsample, cropped to the input (:109-119); only the needed window is computed
        H, W = x.shape[2], x.shape[3]
        uh, uw = self.upsample.out_hw(t.shape[2], t.shape[3])
        oh, ow = min(uh, H), min(uw, W)
        score = self.upsample(t, window=(center(uh, oh), center(uw, ow), oh, ow))
        net['score'] = score
        net['probs_dimshuffle'] = ops.crop_softmax(score, oh, ow, off=(0, 0))  # :122-130,187-191
        # maps owned by the internal border store are overwritten by the next call: hand out
        # copies.  Their PROVENANCE is reported next to the result, never stuck onto the tensor:
        # `last_provenance[i]` describes output i -- outside `region` such a map is a function of
        # this net's weights and the geometry alone, which lets a consumer (the DAE's encoder)
        # keep ITS weights-only border across batches as well.  api.IterativeInference carries
        # the records from pred_fcn_fn to refine (validated by object identity + torch's in-place
        # version counter), or a caller passes them explicitly (`refine(..., h_provenance=)`).
        res, prov = [], []
        for el in self.layer:
            t = net[el]
            tag = None
            if own and el.startswith('pool'):
                if not c8:                   # (C8: already a fresh fp32 copy of the stored map)
                    t = t.clone()
                tag = ((self._uid, session['key']), deps[el])
            res.append(t)
            prov.append(tag)
        self.last_provenance = prov
        return res

    def new_session(self):
        """State for consecutive forwards that differ only in x (see `forward`)."""
        return {'primed': False}

    def _conv(self, name, t, **kw):
        conv = self.convs[name]
        out = conv(t, **kw)
        if self.conv_log is not None:
            # (name, nominal FLOPs of the full layer, FLOPs of the computed window)
            fh, fw = conv.out_hw(t.shape[2], t.shape[3])
            if kw.get('window') is not None:
                ch, cw = kw['window'][2], kw['window'][3]
            elif out is not None:
                ch, cw = out.shape[2], out.shape[3]
            else:
                ch, cw = fh, fw
            self.conv_log.append((name, conv.flops(t.shape[0], fh, fw),
                                  conv.flops(t.shape[0], ch, cw)))
        return out

    def _deconv_sum(self, deconv, t, score_name, pool):
        dh, dw = deconv.out_hw(t.shape[2], t.shape[3])
        sh, sw = pool.shape[2], pool.shape[3]          # 1x1 'valid'/'same' conv keeps the size
        oh, ow = min(dh, sh), min(dw, sw)
        side = self._conv(score_name, pool, window=(center(sh, oh), center(sw, ow), oh, ow))
        return deconv(t, add=side, window=(center(dh, oh), center(dw, ow), oh, ow))

    # ---- training (reference train_fcn8.py) ----------------------------------
    def _drop(self, t, keep, generator, deterministic):
        """DropoutLayer(p, rescale=True) on a copy of t: (dropped map, the 0/1 mask used or None)."""
        if deterministic or self.dropout == 0.0:
            return t, None
        if keep is None:
            keep = (torch.rand(t.shape, generator=generator, device=t.device, dtype=torch.float32) >=
                    self.dropout).to(t.dtype)
        elif tuple(keep.shape) != tuple(t.shape) or keep.dtype != t.dtype:
            raise RuntimeError('dropout mask %s %s for a map %s %s' % (tuple(keep.shape), keep.dtype,
                                                                      tuple(t.shape), t.dtype))
        return ops.dropout_apply(t.clone(), keep, self.dropout), keep

    def _side_sum(self, s, deconv, dname, t, sname, pname):
        """`_deconv_sum` with what `backward` reads kept: the windows and the side layer's rectified output."""
        pool = s[pname]
        dh, dw = deconv.out_hw(t.shape[2], t.shape[3])
        sh, sw = pool.shape[2], pool.shape[3]
        oh, ow = min(dh, sh), min(dw, sw)
        s['win_' + sname] = (center(sh, oh), center(sw, ow), oh, ow)
        s['win_' + dname] = (center(dh, oh), center(dw, ow), oh, ow)
        s[sname] = self._conv(sname, pool, window=s['win_' + sname])
        return deconv(t, add=s[sname], window=s['win_' + dname])

    def forward_train(self, x, keep6=None, keep7=None, generator=None, deterministic=False):
        """The training-mode forward on whole maps: returns the score map (before the softmax), cropped to the
        input, and keeps what `backward` reads -- every convolution's input and rectified output, the pooled maps,
        the centre windows of pool4 / pool3, the inputs of the three transposed convolutions and the two dropout
        masks.  keep6 / keep7: the caller's 0/1 masks (the maps' shape and dtype) for the DropoutLayers behind fc6
        and fc7, else drawn from `generator`.  deterministic=True: no dropout (val_fn's forward)."""
        self._need_trainable('forward_train')
        s = {'input': x}
        t = x
        for bi, names in enumerate(_BLOCKS):
            for name in names:
                s['in_' + name] = t
                t = s[name] = self._conv(name, t)
            t = s['pool%d' % (bi + 1)] = ops.maxpool2x2(t)
        s['in_fc6'] = t
        s['fc6'] = t = self._conv('fc6', t)
        s['drop6'], s['keep6'] = self._drop(t, keep6, generator, deterministic)
        s['fc7'] = t = self._conv('fc7', s['drop6'])
        s['drop7'], s['keep7'] = self._drop(t, keep7, generator, deterministic)
        s['score_fr'] = t = self._conv('score_fr', s['drop7'])
        s['fused'] = t = self._side_sum(s, self.score2, 'score2', t, 'score_pool4', 'pool4')
        s['final'] = t = self._side_sum(s, self.score4, 'score4', t, 'score_pool3', 'pool3')
        H, W = x.shape[2], x.shape[3]
        uh, uw = self.upsample.out_hw(t.shape[2], t.shape[3])
        oh, ow = min(uh, H), min(uw, W)
        s['win_upsample'] = (center(uh, oh), center(uw, ow), oh, ow)
        s['score'] = self.upsample(t, window=s['win_upsample'])
        self._tsaved = s
        return s['score']

    def saved_maps(self):
        """What the last `forward_train` kept, under the names of tests/fcn8_train_ref.py; for tests."""
        return dict(self._tsaved)

    def _dgrad_table(self):
        """[(name, how the layer's data gradient is formed)] (datagrads.Layer) of every conv but conv1_1, which has
        none.  Backward-data of a stride-1 conv = the forward conv of the gradient with the flipped filter: 'same'
        for the 3x3 pad-1 layers, as it is for the 1x1 layers, and for the 'valid' 7x7 fc6 the 'valid' conv of g_z
        inside a zero border of 6.  dgrad='bf16': the 3x3 layers by ops.conv_dgrad, kxk='bf16': fc6 / fc7 by
        ops.conv_dgrad_kxk on g_z itself (no zero-bordered copy), on the layer's own parameter; no fp32 flipped
        copy of a filter the bf16 form replaces is built."""
        table = []
        for name in PARAM_ORDER[1:]:
            if name not in self.convs:
                continue
            conv = self.convs[name]
            op = 'conv_dgrad' if self.dgrad == 'bf16' and name in _NAMES_3X3 else \
                'conv_dgrad_kxk' if self.kxk == 'bf16' and name in _NAMES_KXK16 else None
            table.append((name, Layer(None if op else (lambda conv=conv: flipped(conv.W)),
                                      dict(pad=1 if conv.KH == 3 else 0, dtype=self.dtype, mma='f32'), True,
                                      0 if conv.KH == 3 else conv.KH - 1, op, conv)))
        return table

    def backward(self, g_score):
        """{name: (dW, db)} (views of one flat gradient buffer laid out as `self.flat`) for dL/dscore = g_score,
        after `forward_train`.  Last to first: the crop's adjoint and `upsample`, then twice (score_pool3 / score4,
        score_pool4 / score2) the fan-out of the sum into the side 1x1 layer on the pool's centre window and the
        transposed convolution, then score_fr, fc7, fc6 (gate, dropout's adjoint, K x K weight gradient, data
        gradient) and the five blocks (ops.pool_relu_bwd at a block's last convolution, ops.relu_gate at the
        others, ops.conv_wgrad and the flipped-filter convolution).  pool4 and pool3 receive two gradients: the
        main path's (conv5_1's / conv4_1's data gradient) comes first, the side branch's is added to it, placed at
        the centre window's offset.  conv1_1's data gradient is not formed.  Every data gradient is `self.dgrads`'
        (`_dgrad_table`): with dgrad='bf16' the twelve 3x3 ones by ops.conv_dgrad, the ReLU gate that follows one
        inside a block in the same launch instead of the ops.relu_gate launch behind the fp32 layer.  kxk='bf16':
        fc6's and fc7's weight gradients by ops.conv_wgrad_kxk(mma='bf16'), their data gradients by
        ops.conv_dgrad_kxk on g_z itself (no zero-bordered copy); the dropout adjoint and the ops.relu_gate behind
        fc7's data gradient stay the launches they are."""
        self._need_trainable('backward')
        s = self._tsaved
        if s is None:
            raise RuntimeError('backward() needs forward_train() first')
        gv, dgrads = self._params.grad_views(), self.dgrads
        dgrads.prepare()
        win = s['win_upsample']
        ops.deconv_wgrad(s['final'], g_score, *gv['upsample'], stride=8, window=win)
        g = ops.deconv_dgrad(g_score, self.upsample.W, 8, s['final'].shape[2:], window=win)
        side = {}
        for deconv, dname, sname, pname, src in ((self.score4, 'score4', 'score_pool3', 'pool3', 'fused'),
                                                 (self.score2, 'score2', 'score_pool4', 'pool4', 'score_fr')):
            gz = ops.relu_gate(g, s[sname])
            ops.conv_wgrad_kxk(s[pname], gz, *gv[sname], window=s['win_' + sname])
            side[pname] = (sname, gz)
            win = s['win_' + dname]
            ops.deconv_wgrad(s[src], g, *gv[dname], stride=deconv.stride, window=win)
            g = ops.deconv_dgrad(g, deconv.W, deconv.stride, s[src].shape[2:], window=win)
        for name, xin, keep in (('score_fr', 'drop7', 'keep7'), ('fc7', 'drop6', 'keep6'), ('fc6', 'in_fc6', None)):
            gz = ops.relu_gate(g, s[name], dst=g)
            ops.conv_wgrad_kxk(s[xin], gz, *gv[name], mma=self._wgrad_kxk[name])
            g = dgrads(name, gz)
            if keep is not None and s[keep] is not None:
                ops.dropout_apply(g, s[keep], self.dropout)             # dropout's adjoint: the forward's mask
        for bi in range(len(_BLOCKS) - 1, -1, -1):
            names, pname = _BLOCKS[bi], 'pool%d' % (bi + 1)
            if pname in side:
                sname, gz = side[pname]
                oy, ox = s['win_' + sname][:2]
                dgrads(sname, gz, add=g, add_off=(oy, ox), out=g, place=(oy, ox))   # main first, + the side branch
            for ni in range(len(names) - 1, -1, -1):
                name = names[ni]
                # (inside a block g arrives gated: the data gradient behind it took this layer's output as `gate`)
                gz = ops.pool_relu_bwd(g, s[name], s[pname]) if ni == len(names) - 1 else g
                ops.conv_wgrad(s['in_' + name], gz, *gv[name], pad=self.convs[name].pad, mma=self.wgrad)
                if bi or ni:
                    g = dgrads(name, gz, gate=s[names[ni - 1]] if ni else None)
        return gv

    def refresh(self):
        """The parameters (`self.flat`) have been changed in place: every layer packs its weights again into the
        buffers it already has, and the data-gradient layers take the flipped / transposed filters again.  No
        host wait."""
        self._need_trainable('refresh')
        for conv in self.convs.values():
            conv.refresh()
        for deconv in (self.score2, self.score4, self.upsample):
            deconv.refresh()
        self.dgrads.refresh()
        self._border = {}


class FCN8DAE:
    """dae kind 'fcn8' (models/fcn8_dae.py:19-171): an FCN-8 on y with h concatenated at
    `concat_h`.  Callable like pred_dae_fn(h..., y); `scores` gives the pre-softmax map."""

    kind = 'fcn8'

    def __init__(self, params, n_classes, concat_h=('input',), pad=100, device='cuda',
                 dtype=torch.float32, mma=None):
        assert all(el in ['pool1', 'pool2', 'pool3', 'pool4', 'input'] for el in concat_h)  # :33-34
        self.concat_h = list(concat_h)
        # (the concat points of this kind are two-source gathers: fp32 NCHW activations)
        # (a default taken from ops.DEFAULT_MMA -- `--mma bf16c8` / IISEG_MMA -- maps the same way)
        mma = mma or ops.DEFAULT_MMA
        self.net = FCN8(params, n_classes, layer=['score'], pad=pad, device=device, dtype=dtype,
                        mma={'bf16c8': 'bf16', 'bf16x3': 'f32'}.get(mma, mma))
        self.net.fold_border = False       # the border depends on h here: sessions only
        self.licm = os.environ.get('IISEG_ENCODER_LICM', '1') != '0'

    def conv_layers(self):
        return self.net.convs

    def new_session(self, h_list=None, y=None, tags=None):
        """State of one refinement loop (h fixed, y evolving)."""
        return self.net.new_session() if self.licm else None

    def scores(self, h_list, y, mask_override=None, session=None):
        if len(h_list) != len(self.concat_h):
            raise ValueError('expected %d h tensors, got %d' % (len(self.concat_h), len(h_list)))
        return self.net.forward(y, hs=dict(zip(self.concat_h, h_list)), session=session)[0]

    def __call__(self, *args):
        score = self.scores(args[:-1], args[-1])
        return ops.crop_softmax(score, score.shape[2], score.shape[3], off=(0, 0))

    def residual(self, *args):
        score = self.scores(args[:-1], args[-1])
        return ops.crop_softmax(score, score.shape[2], score.shape[3], off=(0, 0),
                                minuend=args[-1])


def buildFCN8_DAE(input_concat_h_vars=None, input_mask_var=None, n_classes=11, nb_in_channels=3,
                  path_weights=None, model_name='fcn8_model.npz', trainable=False,
                  load_weights=False, pretrained=False, freeze=False, pretrained_path=None,
                  pascal=False, return_layer='probs_dimshuffle', concat_h=('input',), noise=0.1,
                  dropout=0.5, params=None, device='cuda', dtype=torch.float32):
    """Mirror of models/fcn8_dae.py:19-26 (inference only: noise / dropout are identities)."""
    import os
    if params is None:
        if not (load_weights and path_weights):
            raise ValueError('buildFCN8_DAE needs `params` or `path_weights`')
        params = load_param_list(os.path.join(path_weights, model_name), PARAM_ORDER)  # :174-178
    return FCN8DAE(params, n_classes, concat_h=concat_h, device=device, dtype=dtype)


def buildFCN8(nb_in_channels, input_var=None, path_weights=None, n_classes=21, load_weights=True,
              void_labels=(), trainable=False, layer=('probs_dimshuffle',), pascal=False,
              temperature=1.0, dropout=0.5, params=None, pad=100, device='cuda',
              dtype=torch.float32):
    """Mirror of models/fcn8.py:16-23.  Weights come from `params` (dict name -> (W, b)) or from
    an `arr_%d` .npz at `path_weights` in get_all_param_values order (:178-180).  `input_var` is
    accepted for signature compatibility.  trainable=True builds the module `train.FCN8Trainer` trains
    (`FCN8(..., trainable=True, dropout=dropout)`); otherwise dropout is the
    identity (P8).  pascal .mat import (:134-176) is not supported."""
    if pascal:
        raise NotImplementedError('pascal .mat weights are not supported')
    if params is None:
        if not (load_weights and path_weights):
            raise ValueError('buildFCN8 needs `params` or `path_weights`')
        params = load_param_list(path_weights, PARAM_ORDER)
    w0 = params['conv1_1'][0]
    if w0.shape[1] != nb_in_channels:
        raise ValueError('conv1_1 expects %d input channels, nb_in_channels=%d'
                         % (w0.shape[1], nb_in_channels))
    if trainable:
        return FCN8(params, n_classes, layer=layer, pad=pad, temperature=temperature, device=device,
                    dtype=dtype, mma='f32', trainable=True, dropout=dropout)
    return FCN8(params, n_classes, layer=layer, pad=pad, temperature=temperature, device=device,
                dtype=dtype)
