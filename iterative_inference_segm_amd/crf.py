"""Dense-CRF mean field on MI355X: the post-processing baseline of the reference's crf_inference.py
(pydensecrf's DenseCRF2D with a Gaussian smoothness kernel and a bilateral appearance kernel, Potts
compatibility, symmetric normalisation), with the pairwise sums computed exactly inside a
(2R+1) x (2R+1) window by the HIP kernels of csrc/crf.hip (DESIGN.md "Dense-CRF baseline").

    crf = DenseCRF()                       # the reference's parameters (crf_inference.py:164-177)
    Q = crf.inference(Y, X, num_iter=80)   # Y (B, C, H, W) probabilities, X (B, 3, H, W) image

Tensors live on the device; the dtype of Y (float32 or float64) selects the kernels.
"""
import ctypes as C
import math

import torch

from . import _lib
from ._lib import CrfDesc, check
from .ops import _ptr, _stream

_SUFFIX = {torch.float32: 'f32', torch.float64: 'f64'}


class DenseCRF:
    """The reference's DenseCRF2D set-up: addPairwiseGaussian(sxy=sxy_g, compat=w_g) and
    addPairwiseBilateral(sxy=sxy_b, srgb=srgb, compat=w_b), unary_from_softmax(clip=clip).
    radius: half-width R of the summation window (default ceil(4 max(sxy_g, sxy_b)) = 12)."""

    def __init__(self, sxy_g=3, w_g=3, sxy_b=3, srgb=13, w_b=10, radius=None, clip=1e-5):
        self.sxy_g, self.w_g, self.sxy_b, self.srgb, self.w_b = (
            float(sxy_g), float(w_g), float(sxy_b), float(srgb), float(w_b))
        self.clip = float(clip)
        self.radius = int(math.ceil(4 * max(self.sxy_g, self.sxy_b))) if radius is None else int(radius)
        self._ws = {}       # (B, C, H, W, dtype, device) -> workspaces

    def desc(self, B, Cn, H, W, bilateral=True, input_0_255=False):
        d = CrfDesc()
        d.B, d.C, d.H, d.W, d.R = int(B), int(Cn), int(H), int(W), self.radius
        d.flags = (_lib.CRF_BILATERAL if bilateral else 0) | (_lib.CRF_INPUT_0_255 if input_0_255 else 0)
        d.sxy_g, d.w_g, d.sxy_b, d.srgb, d.w_b, d.clip = (self.sxy_g, self.w_g, self.sxy_b, self.srgb,
                                                          self.w_b, self.clip)
        return d

    def supported(self, B, Cn, H, W):
        return bool(_lib.load().iiseg_crf_supported(C.byref(self.desc(B, Cn, H, W))))

    def workspaces(self, B, Cn, H, W, dtype, device):
        """U, I, n^g, n^b and a ping-pong buffer for Q, cached per shape."""
        key = (B, Cn, H, W, dtype, str(device))
        ws = self._ws.get(key)
        if ws is None:
            e = lambda *s: torch.empty(s, dtype=dtype, device=device)
            ws = self._ws[key] = {'U': e(B, Cn, H, W), 'I': e(B, 3, H, W), 'ng': e(B, H, W),
                                  'nb': e(B, H, W), 'Q': e(B, Cn, H, W)}
        return ws

    def inference(self, Y, X, num_iter, bilateral=True, input_0_255=False, out=None):
        """Q after `num_iter` mean-field iterations (0: softmax(-U)).  Y (B, C, H, W) probabilities, X
        (B, 3, H, W) image in [0, 1] (0..255 with input_0_255), same dtype, on the device.  Returns a new
        tensor (or `out`); the work is enqueued on the current stream."""
        dt = Y.dtype
        if dt not in _SUFFIX:
            raise RuntimeError('DenseCRF supports float32 and float64, not %s' % dt)
        B, Cn, H, W = Y.shape
        if tuple(X.shape) != (B, 3, H, W):
            raise RuntimeError('image must be (B, 3, H, W) = %s, got %s' % ((B, 3, H, W), tuple(X.shape)))
        num_iter = int(num_iter)
        if num_iter < 0:
            raise ValueError('num_iter must be >= 0')
        d = self.desc(B, Cn, H, W, bilateral, input_0_255)
        lib = _lib.load()
        sfx = _SUFFIX[dt]
        ws = self.workspaces(B, Cn, H, W, dt, Y.device)
        if out is None:
            out = torch.empty_like(Y, memory_format=torch.contiguous_format)
        s = _stream()
        # ping-pong so that the last iteration lands in `out`
        a, b = (out, ws['Q']) if num_iter % 2 == 0 else (ws['Q'], out)
        p = lambda t: _ptr(t, dt)
        check(getattr(lib, 'iiseg_crf_prepare_' + sfx)(s, C.byref(d), p(Y), p(X), p(ws['U']), p(a), p(ws['I']),
                                                        p(ws['ng']), p(ws['nb'])), 'iiseg_crf_prepare')
        step = getattr(lib, 'iiseg_crf_step_' + sfx)
        for _ in range(num_iter):
            check(step(s, C.byref(d), p(ws['U']), p(a), p(ws['I']), p(ws['ng']), p(ws['nb']), p(b)),
                  'iiseg_crf_step')
            a, b = b, a
        return out
