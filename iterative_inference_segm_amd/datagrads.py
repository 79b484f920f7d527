"""The data gradients of a trainable net's layers, in one place: per layer either the fp32
flipped-filter form -- backward-data of a stride-1 conv = the forward conv of the gradient with the
channel-transposed, spatially flipped filter, an ops.Conv on a copy of that filter -- or the bf16 form on the
parameter itself (ops.conv_dgrad / ops.conv_dgrad_kxk on a packed bf16 image of it).  Which one a layer takes is
fixed when its net is built; the nets' backward walks only say `grads(name, g_z, ...)`."""
import collections

import torch

from . import ops


def flipped(W):
    """The filter of the backward-data conv of a layer with filter W[out, in, k, k] (a view)."""
    return W.transpose(0, 1).flip(2, 3)


def _embed(g, hw, off):
    """Adjoint of a crop: a zeroed map of planes `hw` with `g` at offset `off` (NCHW or C8: dims 2, 3 are the
    planes in both)."""
    out = torch.zeros(tuple(g.shape[:2]) + tuple(hw) + tuple(g.shape[4:]), dtype=g.dtype, device=g.device)
    out[:, :, off[0]:off[0] + g.shape[2], off[1]:off[1] + g.shape[3]].copy_(g)
    return out


# How one layer's data gradient is formed.
# filt: callable -> the flipped (or flipped and transposed) filter view of the layer's parameter; None: the layer never
#       takes the flipped-filter form (no fp32 copy of its filter is built).
# conv_kw: the ops.Conv keywords of the flipped-filter layer (pad, dil, layout, dtype, mma); plain: clear its `wino` /
#       `wino_f64` (no weight transform to keep in step, Conv.refresh).
# border: the zero border g_z is embedded in first (K - 1 for a 'valid' K x K layer: fc6).
# op: None, or the bf16 form -- 'conv_dgrad' (3x3 pad 1) or 'conv_dgrad_kxk' ('valid' K x K), looked up in ops at every
#       call, with its '<op>_pack' -- on `layer`.W (the forward layer: its parameter, read in place), for the input
#       channels [ci0, ci0 + cin): behind a concat the feature channels only, h is a constant.
Layer = collections.namedtuple('Layer', 'filt conv_kw plain border op layer ci0 cin',
                               defaults=(False, 0, None, None, 0, None))


class Views:
    """The data-gradient state of a net (`self.dgrads`) under the names it had on the nets themselves: read-only,
    for tests and scripts."""
    _bwd = property(lambda self: self.dgrads.layers)           # None until built, then {name: Conv}
    _dpack = property(lambda self: self.dgrads.images)
    _dpack_fresh = property(lambda self: self.dgrads.fresh)

    def _bwd_convs(self):
        return self.dgrads.flipped_layers()

    def _flipped_filters(self):
        """(name, filter) of every flipped-filter layer."""
        return ((name, e.filt()) for name, e in self.dgrads.table.items() if e.filt is not None)


class DataGrads:
    def __init__(self, table, refuse=None):
        """table: [(name, Layer)] in the order the flipped-filter layers are built.  refuse: called before they are
        (a net whose configuration has no gradient mode raises there).  No device work."""
        self.table = collections.OrderedDict(table)
        self.refuse = refuse
        self.layers = None                       # {name: ops.Conv on the flipped filter}, built at first use
        self.images, self.fresh = {}, set()      # {name: bf16 filter image}, those packed since `refresh`

    def flipped_layers(self):
        """{name: flipped-filter ops.Conv} of every layer that has a `filt`: built once, all together, at first use."""
        if self.layers is None:
            if self.refuse is not None:
                self.refuse()
            layers = {}
            for name, e in self.table.items():
                if e.filt is None:
                    continue
                Wt = e.filt()
                conv = layers[name] = ops.Conv(Wt.contiguous(), None, relu=False, device=Wt.device, **e.conv_kw)
                if e.plain:
                    conv.wino = conv.wino_f64 = False
            self.layers = layers
        return self.layers

    def prepare(self, flipped=False):
        """Before a walk's first launch: builds the flipped-filter layers if a call of the walk would take one."""
        if flipped or any(e.op is None for e in self.table.values()):
            self.flipped_layers()

    def __call__(self, name, gz, acc=None, gate=None, window=None, flipped=False, **kw):
        """The data gradient of layer `name` for g_z: + acc (summed in place), times [gate > 0], `window` of it.
        flipped: the flipped-filter form whatever the layer was configured with.  kw: further keywords of the
        flipped-filter launch (a C8 layer's mask_in / unpool_hw / add / out_format; add / add_off / out / place).
        bf16 form: accumulate and gate ride in the launch, a window is refused; the image of the filter is packed on
        first use after `refresh`, into the buffer it already has.  fp32 form: the zero border first, `acc` as the
        launch's add and target, the gate as an ops.relu_gate launch behind it."""
        e = self.table[name]
        if e.op is not None and not flipped:
            if window is not None:
                raise NotImplementedError("dgrad='bf16': the pad-100 first layer's window stays on the fp32 path")
            W, layout = e.layer.W, e.layer.layout
            if name not in self.fresh:
                self.images[name] = getattr(ops, e.op + '_pack')(W, tuple(gz.shape), e.ci0, e.cin, layout,
                                                                 out=self.images.get(name))
                self.fresh.add(name)
            return getattr(ops, e.op)(gz, W, ci0=e.ci0, cin=e.cin, layout=layout, out=acc,
                                      accumulate=acc is not None, gate=gate, packed=self.images[name])
        conv = self.flipped_layers()[name]
        if e.border:
            b = e.border
            gz = _embed(gz, (gz.shape[2] + 2 * b, gz.shape[3] + 2 * b), (b, b))
        if acc is not None:
            kw.update(add=acc, out=acc)
        if window is not None:
            kw['window'] = window
        g = conv(gz, **kw)
        return g if gate is None else ops.relu_gate(g, gate, dst=g)

    def refresh(self):
        """The parameters have been changed in place: the flipped-filter layers that exist take their filters
        again and pack them into the buffers they have; every bf16 image is stale."""
        if self.layers is not None:
            for name, conv in self.layers.items():
                conv.W.copy_(self.table[name].filt())
            for conv in self.layers.values():
                conv.refresh()
        self.fresh.clear()
