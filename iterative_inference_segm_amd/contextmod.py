"""Context-module DAE on the HIP kernels (mirror of reference models/contextmod_dae.py:19-138):
conv3x3(+ReLU) on [h=image, y] -> pad 32 -> six dilated 3x3 convs (dilation 1,2,4,8,16,1, ReLU)
-> 1x1 linear -> softmax, 11 channels throughout.  The PadLayer is the `pad` of the first dilated
conv; the 3x3 layers (dilation 1..16) run on the 16-channel halo kernel (`conv_halo16`, 16x16x4
MFMA; DilatedConv2DLayer weight layout W[in,out,k,k], P11); inside a refinement loop the concat is
a buffer whose y channels are refreshed per step, outside it the two-source gather.

`mma='bf16c8'` (float32 only) is the 16-bit leg: bf16 C8 activations between the layers,
every layer but the image half of conv1 on `ops.ConvC8Dil` (csrc/conv_c8_dil.hip), the score map in fp32.  The
other modes ('f32', 'bf16', 'bf16x3') run the fp32 kernels below: layers this narrow have no other 16-bit form."""
import os

import torch

from . import ops
from .datagrads import DataGrads, Layer
from .params import Trainable
from .weights import load_param_list

# inside a refinement loop the image half of the first layer (3 of its 14 input channels; h is the image and does not
# change) is computed once per batch and the y half CONTINUES its FMA chain from that map (bit-identical: the
# chain is bias, then the channels in order, h first -- P13); 0: the whole layer every step
CTX_HSPLIT = os.environ.get('IISEG_CTX_HSPLIT', '1') != '0'

PARAM_ORDER = ['conv1'] + ['dilconv%d' % i for i in range(1, 8)]   # get_all_param_values (P14)
DILATIONS = [1, 2, 4, 8, 16, 1]                                     # contextmod_dae.py:78-101
GRAD_MAX_CHANNELS = 16      # csrc/ctx_train.hip wgrad_check, csrc/ctx_grad.hip dgrad_check: Cin, Cout <= 16


class ContextModDAE(Trainable):
    kind = 'contextmod'

    def __init__(self, params, n_classes, concat_h=('input',), device='cuda',
                 dtype=torch.float32, mma=None):
        """mma: None (ops.DEFAULT_MMA) | 'f32' | 'bf16' | 'bf16x3' | 'bf16c8'.  Only 'bf16c8' changes anything
        here, and only for float32 (`self.c8`): float64 ignores it."""
        assert all(el in ['input'] for el in concat_h)               # contextmod_dae.py:42
        mma = (mma or ops.DEFAULT_MMA) if dtype == torch.float32 else 'f32'
        if mma not in ('f32', 'bf16', 'bf16c8', 'bf16x3'):
            raise ValueError("mma must be 'f32', 'bf16', 'bf16c8' or 'bf16x3'")
        self.mma = mma
        self.c8 = mma == 'bf16c8' and dtype == torch.float32
        if len(concat_h) != 1:
            raise NotImplementedError('one h (the image) is concatenated at the input')
        self.concat_h = list(concat_h)
        # ONE flat parameter buffer in PARAM_ORDER (W then b per layer): every ops.Conv below holds VIEWS of it,
        # so an optimizer step on `flat` followed by `refresh()` reaches every path (training, section 9)
        self.device, self.dtype = device, dtype
        self._views = params = self._store_params(params, PARAM_ORDER, dtype, device)
        self.conv1 = ops.Conv(params['conv1'][0], params['conv1'][1], pad=1, relu=True,
                              device=device, dtype=dtype)                         # :74-76
        self.dil = []
        pad = 32                                                     # PadLayer(width=32), :77
        for i, d in enumerate(DILATIONS):
            W, b = params['dilconv%d' % (i + 1)]
            self.dil.append(ops.Conv(W, b, pad=pad, relu=True, dil=d, layout='iohw', device=device,
                                     dtype=dtype))
            pad = 0
        W, b = params['dilconv7']
        self.last = ops.Conv(W, b, pad=0, relu=False, layout='iohw', device=device,
                             dtype=dtype)                                # :102-105
        # the same two padded layers as 'valid' convolutions of zero-bordered buffers (a refinement loop keeps
        # those buffers, `new_session`): zero padding = a border that is written once and never again, and a
        # 'valid' layer between <= 16 channels runs on the vector-ALU kernel (csrc/conv_small.hip)
        self.conv1_valid = ops.Conv(params['conv1'][0], params['conv1'][1], pad=0, relu=True,
                                    device=device, dtype=dtype)
        W, b = params['dilconv1']
        self.dil1_valid = ops.Conv(W, b, pad=0, relu=True, dil=DILATIONS[0], layout='iohw', device=device,
                                   dtype=dtype)
        self._hold_views(self._shared_convs())
        self._sessions = {}
        self._conv1_params = (params['conv1'][0], params['conv1'][1], device, dtype)
        self._hsplit = {}           # h channels -> (image-half conv, y-half conv) of the first layer
        # training: the data-gradient layers of dilconv1..7.  The adjoint of a 'valid' dilated 3x3 layer is the same
        # layer with the channel-transposed, spatially flipped filter on g_z inside a zero border of 2 d (the
        # weight-gradient kernel stores g_z there) -- W[in,out,k,k] flipped and READ as W[out,in,k,k] is that filter
        self.dgrads = DataGrads([(name, Layer(lambda W=params[name][0]: W.flip(2, 3),
                                              dict(pad=0, dil=d, layout='oihw', dtype=dtype)))
                                 for name, d in zip(PARAM_ORDER[1:], DILATIONS + [1])])
        self._train = {}            # training: buffers per geometry
        self._saved = None          # training: what `forward_train` kept for `backward`
        self._keep_pre, self._pre = False, None
        if self.c8:
            # the 16-bit leg's layers: views of `flat` read through their strides, packed to bf16 operand images
            if max(self.conv1.Cout, self.last.Cout, *(c.Cout for c in self.dil)) > 16:
                raise NotImplementedError("mma='bf16c8': the context module's layers have at most 16 channels")
            self._c8_first = {}     # h channels -> the y half of conv1 (its image half: `_split_convs`)
            self._c8_dil = [ops.ConvC8Dil(params['dilconv%d' % (i + 1)][0], params['dilconv%d' % (i + 1)][1],
                                          relu=True, dil=d, layout='iohw', device=device)
                            for i, d in enumerate(DILATIONS)]
            self._c8_last = ops.ConvC8Dil(params['dilconv7'][0], params['dilconv7'][1], relu=False, dil=1,
                                          layout='iohw', device=device)

    def _refuse_c8(self, what):
        if self.c8:
            raise NotImplementedError("mma='bf16c8' runs the context module's forward pass only (no keep_pre / "
                                      "backward_y / sqerr_backward, no forward_train / backward): %s needs "
                                      "mma='f32'" % what)

    def _refuse_wide(self, what):
        """The weight- and data-gradient kernels (ops.conv_small_wgrad / conv_small_dgrad) take at most
        GRAD_MAX_CHANNELS channels on either side, and conv1's input is [h, y].  Inference has no such limit (a
        wider conv1 is not on the small-channel kernel, that is all).  Refused HERE, before a launch: conv1 is the LAST layer a backward
        pass reaches."""
        if self.conv1.Cin > GRAD_MAX_CHANNELS:
            raise NotImplementedError(
                'context module: %s needs classes + h channels <= %d for training and gradient mode (conv1 has '
                '%d input channels); inference (scores / refine in residual mode) has no such limit'
                % (what, GRAD_MAX_CHANNELS, self.conv1.Cin))

    @property
    def keep_pre(self):
        """True: `scores` keeps the seven rectified layer outputs and the score map of its latest call, which
        `backward_y` / `sqerr_backward` read (api._refine sets it per call).  Setting it False drops them."""
        return self._keep_pre

    @keep_pre.setter
    def keep_pre(self, on):
        if on:
            self._refuse_c8('keep_pre (true-gradient mode)')
            self._refuse_wide('keep_pre (true-gradient mode)')
        self._keep_pre = bool(on)
        if not on:
            self._pre = None

    def _shared_convs(self):
        return [self.conv1, self.conv1_valid, self.dil1_valid, self.last] + self.dil

    def conv_layers(self):
        d = {'conv1': self.conv1, 'dilconv7': self.last}
        d.update({'dilconv%d' % (i + 1): c for i, c in enumerate(self.dil)})
        return d

    def new_session(self, h_list=None, y=None, tags=None):
        """State of one refinement loop (h fixed, y evolving): the ConcatLayer((h, y)) buffer of
        contextmod_dae.py:55-59 with h copied in once; each step only refreshes the y channels
        (plain device copies), so conv1 runs single-source."""
        if not h_list or y is None or len(h_list) != 1:
            return None
        h = h_list[0]
        B, ch, H, W = h.shape[0], h.shape[1], y.shape[2], y.shape[3]
        if self.c8:
            return self._new_session_c8(h, y)
        # The buffers are kept per geometry and handed out again (a captured refinement step points into them:
        # a new batch replays the same graph); what a call changes: the h channels (copied here) and the y
        # channels (every step).  The zero borders are written once.
        split = CTX_HSPLIT and y.dtype == torch.float32
        key = (B, ch, y.shape[1], H, W, y.dtype, str(y.device), split)
        sess = self._sessions.get(key)
        if sess is None:
            # [h, y] with the one-pixel zero border of conv1's pad, and conv1's output inside PadLayer(32)'s zeros;
            # split form: h and y in buffers of their own (both halves are dense single-source layers)
            zeros = lambda c, hh, ww: torch.zeros((B, c, hh, ww), dtype=y.dtype, device=y.device)
            pad32 = zeros(self.conv1.Cout, H + 64, W + 64)
            while len(self._sessions) >= 4:
                self._sessions.pop(next(iter(self._sessions)))
            if split:
                sess = {'hpad': zeros(ch, H + 2, W + 2), 'cat': zeros(y.shape[1], H + 2, W + 2), 'ch': 0,
                        'hb': torch.empty((B, self.conv1.Cout, H, W), dtype=y.dtype, device=y.device),
                        'pad32': pad32, 'split': self._split_convs(ch)}
            else:
                sess = {'cat': zeros(ch + y.shape[1], H + 2, W + 2), 'ch': ch, 'pad32': pad32, 'split': None}
            self._sessions[key] = sess
        if sess['split'] is not None:
            # the loop-invariant image half: bias + the h channels' taps, linear, once per batch
            sess['hpad'][:, :, 1:-1, 1:-1].copy_(h)
            sess['split'][0](sess['hpad'], out=sess['hb'])
        else:
            sess['cat'][:, :ch, 1:-1, 1:-1].copy_(h)
        sess['y_in_cat'] = False        # the y channels hold another loop's map
        return sess

    def _split_convs(self, ch):
        pair = self._hsplit.get(ch)
        if pair is None:
            W, b, device, dtype = self._conv1_params
            W = torch.as_tensor(W)
            kw = {'mma': 'f32'} if self.c8 else {}      # (the 16-bit leg keeps the image half in fp32)
            pair = self._hsplit[ch] = (
                ops.Conv(W[:, :ch].contiguous(), b, pad=0, relu=False, device=device, dtype=dtype, **kw),
                ops.Conv(W[:, ch:].contiguous(), None, pad=0, relu=True, device=device, dtype=dtype, **kw))
        return pair

    # ---- the 16-bit leg (mma='bf16c8') ----
    def _new_session_c8(self, h, y):
        """The C8 form of a session, per geometry and handed out again like the fp32 one: `y8` (the y channels
        as a dense C8 map: what `c8_feed` hands to ops.refine_update), `y8cat` (the same inside conv1's one-pixel
        zero border), `hb` (the image half W_h * h + b in fp32, once per batch), `pad32_8` (conv1's output inside
        PadLayer(32)'s zeros) and the six dilated layers' outputs."""
        B, ch, Cy, H, W = h.shape[0], h.shape[1], y.shape[1], y.shape[2], y.shape[3]
        if ch + Cy != self.conv1.Cin or Cy > 16:
            raise RuntimeError('context module: h %s, y %s' % (tuple(h.shape), tuple(y.shape)))
        key = (B, ch, Cy, H, W, 'c8', str(y.device))
        sess = self._sessions.get(key)
        if sess is None:
            dev = y.device
            z8 = lambda hh, ww: torch.zeros((B, 2, hh, ww, 8), dtype=torch.bfloat16, device=dev)
            acts, hh, ww = [], H + 64, W + 64
            for d in DILATIONS:
                hh, ww = hh - 2 * d, ww - 2 * d
                acts.append(ops.empty_c8(B, 16, hh, ww, dev))
            while len(self._sessions) >= 4:
                self._sessions.pop(next(iter(self._sessions)))
            sess = self._sessions[key] = {
                'c8': True, 'ch': ch, 'split': self._split_convs(ch), 'first': self._c8_first_layer(ch),
                'hpad': torch.zeros((B, ch, H + 2, W + 2), dtype=y.dtype, device=dev),
                'hb': torch.empty((B, self.conv1.Cout, H, W), dtype=y.dtype, device=dev),
                'y8': ops.empty_c8(B, Cy, H, W, dev), 'y8cat': z8(H + 2, W + 2), 'pad32_8': z8(H + 64, W + 64),
                'acts': acts}
        sess['hpad'][:, :, 1:-1, 1:-1].copy_(h)
        sess['split'][0](sess['hpad'], out=sess['hb'])
        sess['y8_fresh'] = False        # y8 holds another loop's map
        return sess

    def _c8_first_layer(self, ch):
        conv = self._c8_first.get(ch)
        if conv is None:
            # conv1's y half: a slice of the parameter along its input channels, no bias (it is in `hb`)
            conv = self._c8_first[ch] = ops.ConvC8Dil(self._views['conv1'][0][:, ch:], None, relu=True, dil=1,
                                                      layout='oihw', device=self.device)
        return conv

    def c8_feed(self, session):
        """The C8 buffer a fused refinement update may write the new y into for the NEXT `scores` call of this
        session (ops.refine_update(..., y8=)), or None; `c8_fed(session)` afterwards."""
        if not self.c8 or not isinstance(session, dict) or not session.get('c8'):
            return None
        return session['y8']

    def c8_fed(self, session):
        session['y8_fresh'] = True

    def _scores_c8(self, y, session):
        if not session.get('y8_fresh'):
            ops.nchw_to_c8(y, out=session['y8'])
        session['y8_fresh'] = False
        # (ops.refine_update writes dense maps: y8 goes inside conv1's zero border with one strided device copy)
        session['y8cat'][:, :, 1:-1, 1:-1].copy_(session['y8'])
        session['first'](session['y8cat'], add=session['hb'], out=session['pad32_8'], place=(32, 32))
        t = session['pad32_8']
        for conv, out in zip(self._c8_dil, session['acts']):
            t = conv(t, out=out)
        return self._c8_last(t, out_format='nchw')

    def _front(self, session, y):
        """The first two layers of a session step: y into the concat buffer unless a fused step has left it
        there, conv1 into the PadLayer(32) buffer (the whole layer on [h, y], or its y half continuing from the
        cached image half), dilconv1 as a 'valid' layer on that buffer.  Returns dilconv1's output."""
        if not session.get('y_in_cat'):
            session['cat'][:, session['ch']:, 1:-1, 1:-1].copy_(y)
        if session['split'] is not None:
            session['split'][1](session['cat'], add=session['hb'], add_off=(0, 0), out=session['pad32'],
                                place=(32, 32))
        else:
            self.conv1_valid(session['cat'], out=session['pad32'], place=(32, 32))
        return self.dil1_valid(session['pad32'])

    def scores(self, h_list, y, mask_override=None, session=None):
        if len(h_list) != 1:
            raise ValueError('expected 1 h tensor, got %d' % len(h_list))
        if self.c8:
            # (without a session: the same layers on the same per-geometry buffers)
            if not isinstance(session, dict) or not session.get('c8'):
                session = self.new_session(h_list, y)
            return self._scores_c8(y, session)
        if session is None and self.keep_pre:
            # true-gradient mode outside a loop: the same 'valid' layers on the same per-geometry buffers as a
            # loop's session, so the kept maps -- and the gradient -- have the same bits with and without one
            # (the padded forms of conv1 / dilconv1 sum in another order in fp32)
            session = self.new_session(h_list, y)
        if session is not None:
            t = self._front(session, y)
            session['y_in_cat'] = False      # (the caller's update changes y, not the buffer: see `fused_step`)
            rest = self.dil[1:]
            kept = [(session['pad32'], (32, 32)), (t, (0, 0))]       # conv1's map lives inside PadLayer(32)'s zeros
        else:
            t = self.conv1(h_list[0], x2=y)                          # h first (P13)
            rest = self.dil
            kept = [(t, (0, 0))]
        for conv in rest:
            t = conv(t)
            kept.append((t, (0, 0)))
        score = self.last(t)
        # true-gradient mode: the seven rectified outputs (tensor, where the map starts in it) and the score map
        self._pre = {'outs': kept, 'score': score, 'ch': h_list[0].shape[1]} if self.keep_pre else None
        return score

    # ---- true-gradient refinement ----
    def _chain(self, g, L_from, masked, y_shape):
        pre = self._pre
        if pre is None:
            raise RuntimeError('backward_y needs the layer outputs of the forward pass: set dae.keep_pre = True '
                               'before calling scores()')
        outs, ch = pre['outs'], pre['ch']
        B, Cy, H, W = (int(v) for v in y_shape)
        if ch + Cy != self.conv1.Cin or g.shape[0] != B or tuple(g.shape[2:]) != (H, W):
            raise RuntimeError('backward_y: gradient %s for y %s' % (tuple(g.shape), tuple(y_shape)))
        for L in range(L_from, 0, -1):
            # g is the gradient at dilconv L's output: masked by [out_L > 0] while it is read (dilconv7 is linear,
            # and the head has applied dilconv6's mask already)
            out, off = (None, (0, 0)) if (L == 7 or masked) else outs[L]
            masked = False
            d = 1 if L == 7 else DILATIONS[L - 1]
            # PadLayer(32)'s adjoint is the crop at (32, 32): only that window of dilconv1's data gradient
            g = ops.conv_small_dgrad(g, out, self._views['dilconv%d' % L][0], dil=d, layout='iohw', out_off=off,
                                     window=(32, 32, H, W) if L == 1 else None)
        # conv1 (pad 1) is a 'valid' layer on the bordered [h, y] buffer: its adjoint is the interior of that
        # border, and only the y channels are needed (h is a constant of the loop)
        out, off = outs[0]
        return ops.conv_small_dgrad(g, out, self._views['conv1'][0], dil=1, layout='oihw', out_off=off,
                                    window=(1, 1, H, W), ci=(ch, Cy))

    def backward_y(self, g_score, y_shape):
        """J^T g_score: the gradient w.r.t. the y channels of the input, for an upstream gradient on the score
        map of the latest `scores` call (made with `keep_pre` set).  Eight launches; the ReLU masks are applied
        while the gradient maps are read."""
        self._refuse_c8('backward_y')
        self._refuse_wide('backward_y')
        return self._chain(g_score.contiguous(), 7, False, y_shape)

    def sqerr_backward(self, score, y):
        """`backward_y(ops.sqerr_softmax_bwd(score, y), y.shape)` with the softmax backward, dilconv7's adjoint
        and dilconv6's mask as ONE launch (ops.ctx_grad_head): the same bits, one launch fewer."""
        self._refuse_c8('sqerr_backward')
        self._refuse_wide('sqerr_backward')
        if self._pre is None:
            raise RuntimeError('sqerr_backward needs the layer outputs of the forward pass: set dae.keep_pre = '
                               'True before calling scores()')
        out6, _ = self._pre['outs'][6]
        g6 = ops.ctx_grad_head(score, y, out6, self._views['dilconv7'][0], layout='iohw')
        return self._chain(g6, 6, True, y.shape)

    def y_updated(self, session, y):
        """The caller has just updated y outside `fused_step` (the first step of a loop, which also hands out
        the score map): refresh the y channels of the concat buffer, so that every later step -- eager or
        replayed from a captured graph -- starts with the buffer equal to y."""
        if session.get('c8'):
            return                       # (the 16-bit leg's y arrives through `c8_feed`, or is converted by `scores`)
        session['cat'][:, session['ch']:, 1:-1, 1:-1].copy_(y)
        session['y_in_cat'] = True

    def fused_step(self, h_list, y, state, step, session):
        """One refinement step (scores + softmax + update of y, in place) with the last two layers and the
        update as one launch that also refreshes the y channels of the concat buffer (csrc/conv_small.hip
        ctx_tail_kernel): bit-identical y, three launches and the per-step copy of y fewer.  Returns the number
        of norm partials per image written (for ops.refine_finalize), or None when this geometry / dtype has no
        fused form (the caller then runs scores + refine_update)."""
        if self.c8 or session is None or not ops.ctx_tail_supported(self.dil[-1], self.last, y):
            return None                  # (a fused bf16 tail is not built: the caller runs scores + refine_update)
        t = self._front(session, y)
        for conv in self.dil[1:-1]:
            t = conv(t)
        nblk = ops.ctx_tail(self.dil[-1], self.last, t, y, state, step, ycat=session['cat'],
                            cat_c0=session['ch'], cat_off=(1, 1))
        session['y_in_cat'] = True
        return nblk

    # ---- training (reference train_dae.py with dae kind 'contextmod') ----
    @property
    def _adj(self):
        """The data-gradient layers in layer order (None until a `backward` has built them); for tests."""
        return None if self.dgrads.layers is None else list(self.dgrads.layers.values())

    def refresh(self):
        """The parameters (`self.flat`) have been changed in place: every layer object that holds them -- the
        padded and 'valid' forms of conv1 / dilconv1, the image / y halves of conv1 a session uses, the
        data-gradient layers -- packs its weights again into the buffers it already has, and every session's cached
        image half (`hb`) is computed again from the image it holds.  The 16-bit leg's layers pack their bf16
        operand images again from `flat`.  No host wait."""
        if self.c8:
            for conv in self._c8_dil + [self._c8_last] + list(self._c8_first.values()):
                conv.refresh()
        for conv in self._shared_convs():
            conv.refresh()
        W1 = self._views['conv1'][0]
        for ch, (ch_conv, y_conv) in self._hsplit.items():
            ch_conv.W.copy_(W1[:, :ch])
            y_conv.W.copy_(W1[:, ch:])
            ch_conv.refresh()
            y_conv.refresh()
        for sess in self._sessions.values():          # the cached image half of a session that is still in use
            if sess['split'] is not None:
                sess['split'][0](sess['hpad'], out=sess['hb'])
        self.dgrads.refresh()

    def _train_buffers(self, B, ch, Cy, H, W, device):
        key = (B, ch, Cy, H, W)
        buf = self._train.get(key)
        if buf is None:
            zeros = lambda c, hh, ww: torch.zeros((B, c, hh, ww), dtype=self.dtype, device=device)
            Cc = self.conv1.Cout
            buf = {'cat': zeros(ch + Cy, H + 2, W + 2), 'pad32': zeros(Cc, H + 64, W + 64), 'gz': []}
            hh, ww = H + 64, W + 64
            for d in DILATIONS:                  # g_z of dilconv1..6 inside a zero border of 2 d
                hh, ww = hh - 2 * d, ww - 2 * d
                buf['gz'].append(zeros(Cc, hh + 4 * d, ww + 4 * d))
            while len(self._train) >= 2:
                self._train.pop(next(iter(self._train)))
            self._train[key] = buf
        return buf

    def forward_train(self, h_list, y, noise=0.0, generator=None, eps=None):
        """The training-mode forward pass: GaussianNoiseLayer on y (contextmod_dae.py:50-57: y + noise * N(0, 1),
        `eps` = the caller's standard-normal sample, else drawn from `generator`), then the eight layers, whose
        outputs are kept for `backward`.  h_list: the one h map in a list, as `scores` takes it; the bare tensor,
        which this method took before it took a list, is still accepted.  Returns the score map (B,C,H,W) before
        the softmax."""
        self._refuse_c8('forward_train')
        self._refuse_wide('forward_train')
        if isinstance(h_list, torch.Tensor):
            h_list = [h_list]
        if len(h_list) != 1:
            raise ValueError('expected 1 h tensor, got %d' % len(h_list))
        h = h_list[0]
        B, ch, H, W = h.shape
        if tuple(y.shape[2:]) != (H, W) or y.shape[0] != B or ch + y.shape[1] != self.conv1.Cin:
            raise RuntimeError('forward_train: h %s, y %s' % (tuple(h.shape), tuple(y.shape)))
        buf = self._train_buffers(B, ch, y.shape[1], H, W, y.device)
        y = ops.gaussian_noise(y, noise, generator, eps)
        buf['cat'][:, :ch, 1:-1, 1:-1].copy_(h)                      # h first (P13)
        buf['cat'][:, ch:, 1:-1, 1:-1].copy_(y)
        self.conv1_valid(buf['cat'], out=buf['pad32'], place=(32, 32))
        acts = [buf['pad32'], self.dil1_valid(buf['pad32'])]
        for conv in self.dil[1:]:
            acts.append(conv(acts[-1]))
        score = self.last(acts[-1])
        self._saved = {'buf': buf, 'acts': acts, 'score': score, 'hw': (H, W)}
        return score

    def saved_outputs(self):
        """The eight layer outputs of the last `forward_train` (conv1 as its (H, W) map), for tests."""
        s = self._saved
        H, W = s['hw']
        return [s['acts'][0][:, :, 32:32 + H, 32:32 + W]] + s['acts'][1:] + [s['score']]

    def backward(self, g_score):
        """{name: (dW, db)} (views of one flat gradient buffer laid out as `self.flat`) for dL/dscore =
        g_score, after `forward_train`.  Per layer, last to first: the weight-gradient kernel (which applies
        the ReLU mask and stores g_z inside its zero border), then the data gradient as a 'valid' layer."""
        self._refuse_c8('backward')
        self._refuse_wide('backward')
        s = self._saved
        if s is None:
            raise RuntimeError('backward() needs forward_train() first')
        gv, dgrads, acts, buf = self._params.grad_views(), self.dgrads, s['acts'], s['buf']
        dgrads.prepare()
        H, W = s['hw']
        ops.conv_small_wgrad(acts[6], g_score, None, *gv['dilconv7'], dil=1, layout='iohw')
        g = dgrads('dilconv7', g_score)
        for L in range(6, 0, -1):
            d = DILATIONS[L - 1]
            gz = buf['gz'][L - 1]
            ops.conv_small_wgrad(acts[L - 1], g, acts[L], *gv['dilconv%d' % L], dil=d, layout='iohw', gz=gz,
                                 gz_off=(2 * d, 2 * d))
            # PadLayer(32)'s adjoint is the crop at (32, 32): only that window of dilconv1's data gradient
            g = dgrads('dilconv%d' % L, gz, window=(32, 32, H, W) if L == 1 else None)
        c1 = acts[0][:, :, 32:32 + H, 32:32 + W].contiguous()
        ops.conv_small_wgrad(buf['cat'], g, c1, *gv['conv1'], dil=1, layout='oihw')
        return gv

    def __call__(self, *args):
        score = self.scores(args[:-1], args[-1])
        return ops.crop_softmax(score, score.shape[2], score.shape[3], off=(0, 0))

    def residual(self, *args):
        score = self.scores(args[:-1], args[-1])
        return ops.crop_softmax(score, score.shape[2], score.shape[3], off=(0, 0),
                                minuend=args[-1])


def buildDAE_contextmod(input_concat_h_vars=None, input_mask_var=None, n_classes=11,
                        path_weights=None, model_name='dae_model.npz', trainable=False,
                        load_weights=False, out_nonlin='softmax', concat_h=('input',), noise=0.1,
                        params=None, device='cuda', dtype=torch.float32, mma=None):
    """Mirror of models/contextmod_dae.py:19-23 (inference only: noise is the identity).  mma: see
    ContextModDAE (None = ops.DEFAULT_MMA; 'bf16c8' = the 16-bit leg)."""
    if params is None:
        if not (load_weights and path_weights):
            raise ValueError('buildDAE_contextmod needs `params` or `path_weights`')
        params = load_param_list(os.path.join(path_weights, model_name), PARAM_ORDER)  # :127-132
    return ContextModDAE(params, n_classes, concat_h=concat_h, device=device, dtype=dtype, mma=mma)
