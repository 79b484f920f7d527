"""CPU: datagrads.DataGrads alone, on stub layers and stubbed ops functions (host tensors, no library): the form
each table entry was configured with is the one its call takes, `flipped=True` forces the flipped-filter form, the
flipped-filter layers are built once and all together, `refresh()` copies the filters again into the layers that
exist, and a bf16 image is packed on first use after `refresh()` into the buffer it already has."""
import types

import pytest
import torch

from iterative_inference_segm_amd import datagrads as DG


class _Conv:
    """ops.Conv's stand-in: keeps its filter and keywords, logs its launches."""

    def __init__(self, W, b, log=None, **kw):
        assert b is None and W.is_contiguous()
        self.W, self.kw, self.wino, self.wino_f64 = W.clone(), kw, True, True
        self.log = log
        log.append(('build', id(self)))

    def __call__(self, gz, **kw):
        self.log.append(('conv', id(self), tuple(gz.shape), dict(kw)))
        return kw['out'] if kw.get('out') is not None else torch.full((1,), float(self.W.sum()))

    def refresh(self):
        self.log.append(('refresh', id(self)))


class _Fwd:
    """A forward layer: the parameter the bf16 form reads in place."""

    def __init__(self, W, layout='oihw'):
        self.W, self.layout, self.Cin = W, layout, W.shape[1]


def _stub_ops(log):
    def pack(op):
        def f(W, gz_shape, ci0, cin, layout, out=None):
            log.append((op + '_pack', gz_shape, ci0, cin, layout, None if out is None else out.data_ptr()))
            if out is None:
                out = torch.empty(W.numel(), dtype=torch.bfloat16)
            return out.copy_(W.reshape(-1))
        return f

    def run(op):
        def f(gz, W, ci0=0, cin=None, layout='oihw', out=None, accumulate=False, gate=None, packed=None):
            log.append((op, ci0, cin, layout, out, accumulate, gate, packed.data_ptr(), float(packed.float().sum())))
            return gz
        return f

    def relu_gate(g, out, dst=None):
        log.append(('relu_gate', g, out, dst))
        return dst

    return types.SimpleNamespace(Conv=lambda W, b, **kw: _Conv(W, b, log=log, **kw), relu_gate=relu_gate,
                                 conv_dgrad=run('conv_dgrad'), conv_dgrad_pack=pack('conv_dgrad'),
                                 conv_dgrad_kxk=run('conv_dgrad_kxk'), conv_dgrad_kxk_pack=pack('conv_dgrad_kxk'))


@pytest.fixture
def net(monkeypatch):
    """Four layers: 'a' fp32 only; 'b' bf16 3x3 behind a concat, with a flipped filter too; 'c' bf16 K x K without
    one; 'd' fp32 with a zero border of 2."""
    log = []
    monkeypatch.setattr(DG, 'ops', _stub_ops(log))
    W = {n: torch.arange(2 * 3 * k * k, dtype=torch.float32).reshape(2, 3, k, k) + i
         for i, (n, k) in enumerate((('a', 3), ('b', 3), ('c', 1), ('d', 3)))}
    fb, fc = _Fwd(W['b']), _Fwd(W['c'], 'iohw')
    dg = DG.DataGrads([
        ('a', DG.Layer(lambda: DG.flipped(W['a']), dict(pad=1, mma='f32'), plain=True)),
        ('b', DG.Layer(lambda: DG.flipped(W['b'][:, 1:]), dict(pad=1), op='conv_dgrad', layer=fb, ci0=1, cin=2)),
        ('c', DG.Layer(None, {}, op='conv_dgrad_kxk', layer=fc)),
        ('d', DG.Layer(lambda: DG.flipped(W['d']), dict(pad=0, dil=2), border=2))])
    return dg, W, log


def test_creating_it_builds_nothing(net):
    dg, _, log = net
    assert log == [] and dg.layers is None and dg.images == {} and dg.fresh == set()


def test_the_flipped_layers_are_built_once_all_together_in_table_order(net):
    dg, W, log = net
    layers = dg.flipped_layers()
    assert list(layers) == ['a', 'b', 'd']                                     # 'c' has no filt: never a flipped layer
    assert [e[0] for e in log] == ['build'] * 3 and dg.flipped_layers() is layers and len(log) == 3
    assert torch.equal(layers['a'].W, W['a'].transpose(0, 1).flip(2, 3))
    assert torch.equal(layers['b'].W, W['b'][:, 1:].transpose(0, 1).flip(2, 3))  # the feature channels only
    assert layers['a'].kw == dict(relu=False, device=W['a'].device, pad=1, mma='f32')
    assert layers['d'].kw == dict(relu=False, device=W['d'].device, pad=0, dil=2)
    assert (layers['a'].wino, layers['a'].wino_f64) == (False, False)          # plain
    assert (layers['d'].wino, layers['d'].wino_f64) == (True, True)


def test_prepare_builds_only_when_a_call_would_take_a_flipped_layer(net, monkeypatch):
    dg, W, log = net
    dg.prepare()                                                                # 'a' and 'd' are fp32
    assert dg.layers is not None
    only16 = DG.DataGrads([('b', dg.table['b'])])
    only16.prepare()
    assert only16.layers is None
    only16.prepare(flipped=True)
    assert list(only16.layers) == ['b']


def test_a_refusal_is_raised_when_the_layers_are_built_not_before(net):
    def refuse():
        raise NotImplementedError('gradient mode: no')
    dg = DG.DataGrads(list(net[0].table.items()), refuse)
    dg(*('c', torch.zeros(1, 2, 4, 4)))                                         # the bf16 form builds nothing
    with pytest.raises(NotImplementedError, match='gradient mode'):
        dg.flipped_layers()
    with pytest.raises(NotImplementedError, match='gradient mode'):
        dg('a', torch.zeros(1, 2, 4, 4))
    assert dg.layers is None


def test_each_entry_takes_the_form_it_was_configured_with(net):
    dg, W, log = net
    gz, acc, gate = torch.zeros(1, 2, 4, 5), torch.ones(1, 3, 4, 5), torch.ones(1, 3, 4, 5)
    # fp32: acc is the launch's add and target, the gate a launch behind it
    out = dg('a', gz, acc=acc, gate=gate)
    a = dg.layers['a']
    assert log[-2][:3] == ('conv', id(a), (1, 2, 4, 5)) and set(log[-2][3]) == {'add', 'out'}
    assert log[-2][3]['add'] is acc and log[-2][3]['out'] is acc
    assert log[-1][0] == 'relu_gate' and log[-1][1] is acc and log[-1][2] is gate and log[-1][3] is acc and out is acc
    n = len(log)
    dg('a', gz, window=(1, 2, 3, 4), mask_in='m', out_format='nchw')            # window and a C8 layer's keywords
    assert log[n:] == [('conv', id(a), (1, 2, 4, 5), dict(window=(1, 2, 3, 4), mask_in='m', out_format='nchw'))]
    n = len(log)
    dg('a', gz)
    assert log[n:] == [('conv', id(a), (1, 2, 4, 5), {})]
    # fp32 with a border: g_z inside zeros first
    n = len(log)
    dg('d', torch.ones(1, 2, 4, 5))
    assert log[n:] == [('conv', id(dg.layers['d']), (1, 2, 8, 9), {})]
    # bf16 3x3: the layer's own parameter and channel slice, accumulate and gate in the launch, no flipped layer
    n = len(log)
    assert dg('b', gz, acc=acc, gate=gate) is gz
    assert [e[0] for e in log[n:]] == ['conv_dgrad_pack', 'conv_dgrad']
    assert log[n][1:5] == ((1, 2, 4, 5), 1, 2, 'oihw')
    op, ci0, cin, layout, o, accumulate, g, ptr, _ = log[n + 1]
    assert (ci0, cin, layout, accumulate) == (1, 2, 'oihw', True) and o is acc and g is gate
    assert ptr == dg.images['b'].data_ptr()
    # bf16 K x K: its own op, the parameter's layout, the defaults of a layer without a concat
    n = len(log)
    dg('c', gz)
    assert [e[0] for e in log[n:]] == ['conv_dgrad_kxk_pack', 'conv_dgrad_kxk']
    assert log[n + 1][1:7] == (0, None, 'iohw', None, False, None)
    with pytest.raises(NotImplementedError, match="dgrad='bf16': the pad-100 first layer's window"):
        dg('b', gz, window=(0, 0, 1, 1))


def test_the_flipped_form_can_be_forced_and_an_entry_without_a_filter_has_none(net):
    dg, W, log = net
    gz = torch.zeros(1, 2, 4, 5)
    dg('b', gz, flipped=True, window=(0, 0, 1, 1))
    assert log[-1] == ('conv', id(dg.layers['b']), (1, 2, 4, 5), dict(window=(0, 0, 1, 1)))
    assert dg.images == {} and not any(e[0].startswith('conv_dgrad') for e in log)
    with pytest.raises(KeyError):
        dg('c', gz, flipped=True)


def test_the_ops_are_looked_up_at_the_call(net, monkeypatch):
    dg, W, log = net
    seen = []
    monkeypatch.setattr(DG.ops, 'conv_dgrad', lambda gz, W_, **kw: seen.append(kw['packed']) or gz)
    dg('b', torch.zeros(1, 2, 4, 5))
    assert len(seen) == 1 and seen[0] is dg.images['b']


def test_refresh_copies_into_the_layers_that_exist_and_marks_the_images_stale(net):
    dg, W, log = net
    gz = torch.zeros(1, 2, 4, 5)
    dg.refresh()                                                                # nothing built: nothing to do
    assert log == [] and dg.layers is None
    dg('b', gz), dg('c', gz), dg('b', gz)
    assert [e[0] for e in log].count('conv_dgrad_pack') == 1 and dg.fresh == {'b', 'c'}   # packed once while fresh
    layers, ptrs = dg.flipped_layers(), {n: t.data_ptr() for n, t in dg.images.items()}
    held = {n: c.W.data_ptr() for n, c in layers.items()}
    for w in W.values():
        w.add_(100.0)                                                           # an optimizer step, in place
    n = len(log)
    dg.refresh()
    assert log[n:] == [('refresh', id(c)) for c in layers.values()]            # every layer, after every copy
    assert dg.flipped_layers() is layers and {n: c.W.data_ptr() for n, c in layers.items()} == held
    assert torch.equal(layers['a'].W, W['a'].transpose(0, 1).flip(2, 3))
    assert torch.equal(layers['b'].W, W['b'][:, 1:].transpose(0, 1).flip(2, 3))
    assert dg.fresh == set() and set(dg.images) == {'b', 'c'}                   # stale, kept
    n = len(log)
    dg('b', gz), dg('b', gz)
    packs = [e for e in log[n:] if e[0] == 'conv_dgrad_pack']
    assert len(packs) == 1 and packs[0][5] == ptrs['b']                         # again, once, into the buffer it had
    assert dg.images['b'].data_ptr() == ptrs['b'] and dg.fresh == {'b'}
    runs = [e for e in log[n:] if e[0] == 'conv_dgrad']
    assert runs[0][8] == float(W['b'].to(torch.bfloat16).float().sum())         # the image of the new parameter
