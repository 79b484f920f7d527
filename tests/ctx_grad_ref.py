"""Float64 (numpy) restatement of the true-gradient refinement step through the context-module DAE:
E(y) = sum (r(y|h) - y)^2 with r = softmax(DAE(h, y)), its gradient w.r.t. y by hand-written reverse mode on
tests/ctx_train_ref.py's forward / data-gradient and oracle/nn.py, and the refinement loop that descends it.
TEST INFRASTRUCTURE: pinned by central finite differences (tests/test_ctx_grad_ref.py); the HIP path
(csrc/ctx_grad.hip, ContextModDAE.backward_y / sqerr_backward) is checked against it.

Conventions as oracle/dae_grad.py: relu'(0) = 0."""
import numpy as np

import ctx_train_ref as R
from oracle import nn
from oracle.contextmod import DILATIONS


def softmax_sqerr_bwd(score, y):
    """(g_s, r): r = softmax(score), g_s = dE/dscore for E = sum (r - y)^2 with y held fixed."""
    r = nn.softmax_channels(score)
    gr = 2.0 * (r - y)
    return r * (gr - (r * gr).sum(axis=1, keepdims=True)), r


def masked_bwd_data(g, out, W_iohw, d):
    """The data gradient of a 'valid' layer from g = dE/d(its rectified output `out`); out=None: linear."""
    return R._bwd_data(g if out is None else np.where(out > 0, g, 0.0), W_iohw, d)


def head(score, y, out6, W7):
    """(g_z of dilconv6, g_s): the softmax backward, dilconv7's adjoint and dilconv6's mask."""
    gs, _ = softmax_sqerr_bwd(score, y)
    g6 = R._bwd_data(gs, W7, 1)
    return np.where(out6 > 0, g6, 0.0), gs


def backward_y(params, outs, g_score, ch):
    """J^T g_score w.r.t. the y channels (those after the first `ch`) from the layer outputs of
    ctx_train_ref.forward."""
    H, W = outs[0].shape[2:]
    g = R._bwd_data(g_score, params['dilconv7'][0], 1)
    for L in range(6, 0, -1):
        g = masked_bwd_data(g, outs[L], params['dilconv%d' % L][0], DILATIONS[L - 1])
    g = g[:, :, 32:32 + H, 32:32 + W]                        # PadLayer(32)'s adjoint
    Wc = np.transpose(params['conv1'][0], (1, 0, 2, 3))      # W[out,in,k,k] -> W[in,out,k,k]
    g = masked_bwd_data(g, outs[0], Wc, 1)                   # w.r.t. the bordered [h, y] buffer
    return g[:, ch:, 1:-1, 1:-1]


def ctx_sqerr_grad(params, h, y):
    """(dE/dy, r) for E(y) = sum (r(y|h) - y)^2: J_r^T 2 (r - y) - 2 (r - y)."""
    _, outs = R.forward(params, h, y)
    gs, r = softmax_sqerr_bwd(outs[-1], y)
    return backward_y(params, outs, gs, h.shape[1]) - 2.0 * (r - y), r


def sqerr(params, h, y):
    _, outs = R.forward(params, h, y)
    return float(((nn.softmax_channels(outs[-1]) - y) ** 2).sum())


def refine_gradient(params, h, y, step, num_iter):
    """The gradient-mode loop of api._refine without early stop: (y, last mean_px ||grad||_2 per image)."""
    yy, last = y.copy(), None
    for _ in range(num_iter):
        g, _ = ctx_sqerr_grad(params, h, yy)
        last = np.linalg.norm(g, axis=1).mean(axis=(1, 2))
        yy = np.clip(yy - step * g, 0.0, 1.0)
    return yy, last
