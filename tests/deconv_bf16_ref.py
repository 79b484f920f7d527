"""Float64 (numpy) statement of what deconv='bf16' computes: the gradients of a K = 3, stride-2
transposed convolution on x (B,Cin,H,W) with W[Cin][Cout][3][3], from g = dL/d(window (oy0, ox0, OH, OW) of the
(2H + 1) x (2W + 1) full output).  With gf = g at the window's offset inside the full output and zero elsewhere, for
a, c in {0, 1, 2}:

    dW[ci][co][2-a][2-c] = sum_{b,i,j}  x[b][ci][i][j]      gf[b][co][2i+a][2j+c]
    gx[b][ci][i][j]      = sum_{co,a,c} W[ci][co][2-a][2-c] gf[b][co][2i+a][2j+c]
    db[co]               = sum g

written as nine strided slices of gf.  The kernels round x, g and W to bf16 (`rounded`) before the products of dW and
gx and sum db over the unrounded g; `grads` takes whatever it is handed.  TEST INFRASTRUCTURE: pinned against
tests/densenet_train_ref.deconv_bwd and the adjoint identity by tests/test_deconv_bf16_ref.py."""
import numpy as np
import torch


def rounded(t):
    """float64 numpy of a float32 tensor (or array) rounded to bf16 on the CPU, nearest with ties to even."""
    t = torch.as_tensor(np.asarray(t.detach().cpu() if torch.is_tensor(t) else t))
    assert t.dtype == torch.float32
    return t.to(torch.bfloat16).double().numpy()


def full_window(H, W):
    return (0, 0, 2 * H + 1, 2 * W + 1)


def _gf(g, H, W, window):
    oy, ox, OH, OW = window
    assert g.shape[2:] == (OH, OW) and oy >= 0 and ox >= 0 and oy + OH <= 2 * H + 1 and ox + OW <= 2 * W + 1
    gf = np.zeros(g.shape[:2] + (2 * H + 1, 2 * W + 1), dtype=np.float64)
    gf[:, :, oy:oy + OH, ox:ox + OW] = g
    return gf


def grads(x, g, W, window=None):
    """(dW, gx, db) in float64 of the three formulas above; x (B,Cin,H,W), g (B,Cout,OH,OW), W (Cin,Cout,3,3)."""
    x, g, W = (np.asarray(v, dtype=np.float64) for v in (x, g, W))
    B, Cin, H, Wd = x.shape
    assert W.shape == (Cin, g.shape[1], 3, 3) and g.shape[0] == B
    gf = _gf(g, H, Wd, full_window(H, Wd) if window is None else window)
    dW, gx = np.zeros_like(W), np.zeros_like(x)
    for a in range(3):
        for c in range(3):
            gs = gf[:, :, a:a + 2 * H - 1:2, c:c + 2 * Wd - 1:2]                # gf[2i + a][2j + c]
            dW[:, :, 2 - a, 2 - c] = np.tensordot(x, gs, axes=([0, 2, 3], [0, 2, 3]))
            gx += np.tensordot(W[:, :, 2 - a, 2 - c], gs, axes=([1], [1])).transpose(1, 0, 2, 3)
    return dW, gx, g.sum(axis=(0, 2, 3))


def mags(x, g, W, window=None):
    """The same sums over absolute values: sum |a b| per entry of dW and gx, sum |g| per entry of db."""
    return grads(np.abs(np.asarray(x, dtype=np.float64)), np.abs(np.asarray(g, dtype=np.float64)),
                 np.abs(np.asarray(W, dtype=np.float64)), window)
