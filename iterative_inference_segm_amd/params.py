"""The parameters of a trainable DAE as ONE flat buffer (W then b per layer, in the checkpoint's order and the
checkpoint's layouts) with views per layer, and its gradient twin: what the optimizer step (ops.opt_step) walks
and what every layer object of the DAE holds views of (DESIGN.md sections 9 and 12); the parameter side every
trainable net shares (`Trainable`) and the 16-bit training switches of the trainable modules.
Plain torch: works on host tensors too, needs no library.  torch is imported where a tensor is made or compared, not
with the module: the training drivers read the switches' names before they parse their arguments."""

# The 16-bit training switches (keyword and attribute of the trainable modules -- FCN8 and StandardDAE have
# several, FCDenseNet has 'wgrad', 'deconv' and 'fwd' (there: the dense-block layers' fused BatchNorm + ReLU +
# convolution) --, option of the drivers): what each is called in messages.  Every one takes MODES_16BIT.
SWITCHES_16BIT = {'wgrad': 'weight gradient', 'dgrad': 'data gradient', 'kxk': 'fc6 / fc7 gradients',
                  'fwd': 'training forward', 'deconv': 'transposed-convolution gradients'}
MODES_16BIT = ('f32', 'bf16')


def check_mode(switch, mode, dtype, trainable=None):
    """`mode` of the 16-bit training switch `switch` (host only), returned.  Of a run of precision `dtype` (a
    torch dtype or its name), or -- `trainable` given -- of a module: 'bf16' is for float32 (trainable) only."""
    if trainable is None:
        if mode not in MODES_16BIT:
            raise ValueError('%s must be one of %s (got %r)' % (switch, ', '.join(MODES_16BIT), mode))
        if mode == 'bf16' and str(dtype).replace('torch.', '') != 'float32':
            raise NotImplementedError("%s='bf16' rounds float32 operands for the 16-bit matrix pipe: dtype must "
                                      'be float32 (got %s)' % (switch, dtype))
    else:
        import torch
        if mode not in MODES_16BIT:
            raise ValueError("%s=%r is not one of %s" % (switch, mode, MODES_16BIT))
        if mode == 'bf16' and not (trainable and dtype == torch.float32):
            raise NotImplementedError("%s='bf16': the 16-bit %s of a trainable float32 module (trainable=%r, dtype=%s)"
                                      % (switch, SWITCHES_16BIT[switch], bool(trainable), dtype))
    return mode


class ParamStore:
    def __init__(self, params, order, dtype, device):
        """params: {name: (W, b)} (arrays or tensors); order: the names, in the order of the flat buffer."""
        import torch
        host = [(n, torch.as_tensor(params[n][0]), torch.as_tensor(params[n][1])) for n in order]
        self._layout = [(n, tuple(W.shape), W.numel(), b.numel()) for n, W, b in host]
        self.flat = torch.empty(sum(nW + nb for _, _, nW, nb in self._layout), dtype=dtype, device=device)
        self.views = self._carve(self.flat)
        for n, W, b in host:
            self.views[n][0].copy_(W.to(dtype))
            self.views[n][1].copy_(b.to(dtype))
        self._gflat = self._gviews = None

    def _carve(self, flat):
        views, off = {}, 0
        for n, shape, nW, nb in self._layout:
            views[n] = (flat[off:off + nW].view(shape), flat[off + nW:off + nW + nb])
            off += nW + nb
        return views

    @property
    def gflat(self):
        """The gradient buffer, laid out as `flat`: zeros, allocated at first use."""
        if self._gflat is None:
            import torch
            self._gflat = torch.zeros_like(self.flat)
            self._gviews = self._carve(self._gflat)
        return self._gflat

    def grad_views(self):
        """{name: (dW, db)}: views of `gflat`."""
        self.gflat
        return dict(self._gviews)

    def holds(self, t):
        """t is a view of `flat`, not a copy (what every layer of the DAE is asserted on)."""
        lo = self.flat.data_ptr()
        return lo <= t.data_ptr() < lo + self.flat.numel() * self.flat.element_size()

    def state_arrays(self):
        """{name: (W, b)} as host arrays (float32, what weights.save_param_list writes); waits for the device."""
        return {n: (W.detach().cpu().float().numpy(), b.detach().cpu().float().numpy())
                for n, (W, b) in self.views.items()}


class Trainable:
    """The parameter side of a trainable net (ContextModDAE, StandardDAE, FCN8): one ParamStore, its views handed
    to the layers, and what a trainer and a checkpoint read of it.  A class names itself in `_BUILT` ('a
    StandardDAE') and says in `trainable` whether this instance was built to be trained."""

    trainable, flat, _params = True, None, None

    def _store_params(self, params, order, dtype, device):
        """The parameters into ONE flat buffer in `order` (W then b per layer): returns {name: (W, b)}, views of
        `self.flat`, for the layers to be built on."""
        self._params = ParamStore(params, order, dtype, device)
        self.flat = self._params.flat
        return self._params.views

    def _hold_views(self, layers, plain=False):
        """Every layer holds views of `flat`, not copies; plain: and runs on the direct / halo / tap kernels only
        (no weight transform to keep in step, Conv.refresh)."""
        for layer in layers:
            assert self._params.holds(layer.W) and self._params.holds(layer.b)
            if plain:
                layer.wino = layer.wino_f64 = False

    def _need_trainable(self, what):
        if not self.trainable:
            raise RuntimeError('%s needs %s built with trainable=True' % (what, self._BUILT))

    def parameters(self):
        """{name: (W, b)} in the order of `flat`: views of it, the checkpoint's arrays in the checkpoint's layouts.
        After changing them in place call `refresh()`."""
        self._need_trainable('parameters')
        return dict(self._params.views)

    def state_arrays(self):
        """{name: (W, b)} as host arrays (float32, what weights.save_param_list writes); waits for the device."""
        self._need_trainable('state_arrays')
        return self._params.state_arrays()

    @property
    def gflat(self):
        """The flat gradient buffer `backward` writes, laid out as `self.flat` (ParamStore.gflat)."""
        self._need_trainable('gflat')
        return self._params.gflat

    def weight_ranges(self):
        """[(lo, hi)] of the weight arrays (not the biases) inside `flat`: what ops.l2_term walks."""
        self._need_trainable('weight_ranges')
        lo, size = self.flat.data_ptr(), self.flat.element_size()
        return [((W.data_ptr() - lo) // size, (W.data_ptr() - lo) // size + W.numel())
                for W, _ in self._params.views.values()]
