"""The parameters of a trainable DAE as ONE flat buffer (W then b per layer, in the checkpoint's order and the
checkpoint's layouts) with views per layer, and its gradient twin: what the optimizer step (ops.opt_step) walks
and what every layer object of the DAE holds views of (DESIGN.md sections 9 and 12); the 16-bit training switches
of the trainable modules and the bf16 filter images their data gradients keep.  Plain torch:
works on host tensors too, needs no library."""
import torch

# The 16-bit training switches (keyword and attribute of FCN8 / StandardDAE, option of the drivers): what each is
# called in messages.  Every one takes MODES_16BIT.
SWITCHES_16BIT = {'wgrad': 'weight gradient', 'dgrad': 'data gradient', 'kxk': 'fc6 / fc7 gradients',
                  'fwd': 'training forward'}
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
        if mode not in MODES_16BIT:
            raise ValueError("%s=%r is not one of %s" % (switch, mode, MODES_16BIT))
        if mode == 'bf16' and not (trainable and dtype == torch.float32):
            raise NotImplementedError("%s='bf16': the 16-bit %s of a trainable float32 module (trainable=%r, dtype=%s)"
                                      % (switch, SWITCHES_16BIT[switch], bool(trainable), dtype))
    return mode


class PackedImages:
    """{name: bf16 image of a layer's filter} (ops.conv_dgrad_pack / conv_dgrad_kxk_pack) and the names packed since
    the parameters last changed: an image is packed on first use after `invalidate()`, into the buffer it has."""

    def __init__(self):
        self.images, self.fresh = {}, set()

    def image(self, name, pack):
        """The image of `name`; stale or missing: pack(out) makes it, into `out` (None: a new tensor)."""
        if name not in self.fresh:
            self.images[name] = pack(self.images.get(name))
            self.fresh.add(name)
        return self.images[name]

    def invalidate(self):
        self.fresh.clear()


class ParamStore:
    def __init__(self, params, order, dtype, device):
        """params: {name: (W, b)} (arrays or tensors); order: the names, in the order of the flat buffer."""
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
