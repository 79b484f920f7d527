"""CPU: the flat parameter store of the trainable DAEs (iterative_inference_segm_amd/params.py) on host tensors --
layout, aliasing, the gradient twin, the checkpoint round trip -- and the trainable StandardDAE's refusal of the
noise-emulation masks before anything is allocated."""
import numpy as np
import pytest
import torch

import ctx_train_ref as CR
import std_train_ref as SR
from iterative_inference_segm_amd import synthetic as S

DT = {'f32': torch.float32, 'f64': torch.float64}


def _cases():
    from iterative_inference_segm_amd import contextmod, dae
    ctx = S.make_contextmod_params(11, 3, seed=31)                  # dilconv*: W[in,out,k,k] ('iohw')
    assert ctx['dilconv1'][0].shape[:2] == ctx['dilconv7'][0].shape[:2] and ctx['conv1'][0].shape[1] == 14
    cfg = SR.SECOND[3]
    order = dae.param_order(['pool2'], 1, 2)
    assert order == SR.order_of(cfg)
    std = S.make_dae_params(11, (16,), concat_h=cfg['concat_h'], n_filters=cfg['n_filters'],
                            additional_pool=cfg['additional_pool'], seed=105)
    return {'contextmod': (ctx, list(contextmod.PARAM_ORDER), CR.flatten(ctx)),
            'standard': (std, order, SR.flatten(std, order))}


def _offsets(views, flat):
    return {n: tuple((t.data_ptr() - flat.data_ptr()) // flat.element_size() for t in wb) for n, wb in views.items()}


@pytest.mark.parametrize('prec', ['f32', 'f64'])
@pytest.mark.parametrize('which', ['contextmod', 'standard'])
def test_param_store_on_host_tensors(which, prec, tmp_path):
    from iterative_inference_segm_amd.params import ParamStore
    from iterative_inference_segm_amd.weights import load_param_list, save_param_list
    params, order, ref = _cases()[which]
    params = {n: tuple(np.asarray(a, np.float32) for a in params[n]) for n in order}   # what a checkpoint holds
    dt = DT[prec]
    st = ParamStore(params, order, dt, 'cpu')
    assert st.flat.dtype == dt and st.flat.dim() == 1 and list(st.views) == order
    assert np.array_equal(st.flat.numpy(), ref.astype(np.float32))                    # W then b, layer by layer
    # every view aliases flat, at the offsets of that concatenation, in the parameter's own shape
    off = 0
    for n in order:
        W, b = st.views[n]
        assert tuple(W.shape) == params[n][0].shape and tuple(b.shape) == params[n][1].shape
        assert st.holds(W) and st.holds(b)
        assert _offsets(st.views, st.flat)[n] == (off, off + W.numel())
        off += W.numel() + b.numel()
    assert off == st.flat.numel()
    assert not st.holds(st.flat.clone()) and not st.holds(st.views[order[0]][0].contiguous().clone())
    st.flat.mul_(2.0)                                                                 # an in-place step ...
    assert all(np.array_equal(st.views[n][0].numpy(), 2 * params[n][0]) for n in order)   # ... reaches the views
    st.views[order[-1]][1].fill_(3.0)
    assert bool((st.flat[-st.views[order[-1]][1].numel():] == 3.0).all())
    # the gradient twin: ONE zero buffer, allocated at first use, views at the same offsets
    assert st._gflat is None
    gv = st.grad_views()
    g = st.gflat
    assert g is st.gflat and g.shape == st.flat.shape and g.dtype == dt and not bool(g.any())
    assert g.data_ptr() != st.flat.data_ptr()
    assert list(gv) == order and _offsets(gv, g) == _offsets(st.views, st.flat)
    assert all(a.shape == b.shape for n in order for a, b in zip(gv[n], st.views[n]))
    gv[order[0]][0].fill_(1.0)
    assert int(g.sum()) == gv[order[0]][0].numel() and st.grad_views()[order[0]][0].data_ptr() == g.data_ptr()
    # the checkpoint round trip
    path = str(tmp_path / 'dae_model_best.npz')
    save_param_list(path, st.state_arrays(), order)
    again = ParamStore(load_param_list(path, order), order, dt, 'cpu')
    assert torch.equal(again.flat, st.flat)


def test_trainable_standard_dae_refuses_noise_emulation_without_a_gpu():
    from iterative_inference_segm_amd.dae import StandardDAE
    params, order, _ = _cases()['standard']
    cfg = SR.SECOND[3]
    for noise in (0.0, 0.1):
        with pytest.raises(NotImplementedError, match='emulate_noise'):
            StandardDAE(params, 11, device='cuda', dtype=torch.float32, mma='f32', trainable=True,
                        emulate_noise=True, noise=noise, **cfg)
