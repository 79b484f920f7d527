"""The parameters of a trainable DAE as ONE flat buffer (W then b per layer, in the checkpoint's order and the
checkpoint's layouts) with views per layer, and its gradient twin: what the optimizer step (ops.opt_step) walks
and what every layer object of the DAE holds views of (DESIGN.md sections 9 and 12).  Plain torch: works on host
tensors too."""
import torch


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
