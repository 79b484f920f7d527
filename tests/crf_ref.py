"""Float64 restatement of the dense-CRF mean field of DESIGN.md "Dense-CRF baseline" (the model of
pydensecrf's DenseCRF2D as the reference's crf_inference.py:164-180 configures it, with the pairwise
sums taken exactly).  numpy, CPU, one image at a time.  A helper module of the tests, not a test file.

    ImageCRF(P, X, ...)           per-image set-up: U, Q0, I, n^g, n^b and the per-tap weight images
    .step(Q) / .run(num_iter)     mean-field iterations
    crf_inference(P, X, n, ...)   a batch, (B, C, H, W) -> (B, C, H, W)

`untruncated=True` replaces the (2R+1)^2 window by all pixel pairs of the image (O(N^2); small images).
"""
import math

import numpy as np

DEFAULTS = dict(sxy_g=3.0, w_g=3.0, sxy_b=3.0, srgb=13.0, w_b=10.0, clip=1e-5)


def default_radius(sxy_g=3.0, sxy_b=3.0):
    return int(math.ceil(4 * max(sxy_g, sxy_b)))


def softmax(a, axis=0):
    e = np.exp(a - a.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def colour_features(X, in255=False):
    """(3, H, W) image -> float64 features: floor of the float32 product 255 x, clamped to [0, 255]."""
    v = np.asarray(X, dtype=np.float32)
    if not in255:
        v = np.float32(255) * v
    return np.clip(np.floor(v.astype(np.float64)), 0.0, 255.0)


def unary(P, clip=1e-5):
    return -np.log(np.clip(np.asarray(P, dtype=np.float64), clip, 1.0))


class ImageCRF:
    def __init__(self, P, X, R=None, bilateral=True, in255=False, untruncated=False, **kw):
        prm = dict(DEFAULTS)
        prm.update(kw)
        self.prm = prm
        self.R = default_radius(prm['sxy_g'], prm['sxy_b']) if R is None else int(R)
        self.bilateral = bilateral
        self.U = unary(P, prm['clip'])
        self.C, self.H, self.W = self.U.shape
        self.Q0 = softmax(-self.U)
        self.I = colour_features(X, in255)
        cg = 1.0 / (2 * prm['sxy_g'] ** 2)
        cb = 1.0 / (2 * prm['sxy_b'] ** 2)
        cc = 1.0 / (2 * prm['srgb'] ** 2)
        H, W = self.H, self.W
        self.untruncated = untruncated
        if untruncated:
            yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
            pos = np.stack([yy.ravel(), xx.ravel()], 1).astype(np.float64)
            d2 = ((pos[:, None, :] - pos[None, :, :]) ** 2).sum(-1)
            f = self.I.reshape(3, -1).T
            c2 = ((f[:, None, :] - f[None, :, :]) ** 2).sum(-1)
            self.Kg = np.exp(-d2 * cg)
            self.Kb = np.exp(-d2 * cb - c2 * cc)
            self.ng = (1 / np.sqrt(self.Kg.sum(1))).reshape(H, W)
            self.nb = (1 / np.sqrt(self.Kb.sum(1))).reshape(H, W)
            return
        # per-tap weight images, computed once: k(i, i + (dy, dx)) for every pixel i (0 where the
        # neighbour lies outside the image)
        R = self.R
        Ip = np.zeros((3, H + 2 * R, W + 2 * R))
        Ip[:, R:R + H, R:R + W] = self.I
        inside = np.zeros((H + 2 * R, W + 2 * R))
        inside[R:R + H, R:R + W] = 1.0
        self.taps = []
        sg = np.zeros((H, W))
        sb = np.zeros((H, W))
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                m = inside[R + dy:R + dy + H, R + dx:R + dx + W]
                d2 = dy * dy + dx * dx
                c2 = ((self.I - Ip[:, R + dy:R + dy + H, R + dx:R + dx + W]) ** 2).sum(0)
                kg = math.exp(-d2 * cg)
                kb = np.exp(-d2 * cb - c2 * cc) * m
                sg += kg * m
                sb += kb
                self.taps.append((dy, dx, kg, kb))
        self.ng = 1 / np.sqrt(sg)
        self.nb = 1 / np.sqrt(sb)

    def messages(self, Q):
        """(m^g, m^b), each (C, H, W), normalised on both sides."""
        C, H, W = Q.shape
        if self.untruncated:
            qg = (Q * self.ng).reshape(C, -1)
            qb = (Q * self.nb).reshape(C, -1)
            mg = (qg @ self.Kg.T).reshape(C, H, W) * self.ng
            mb = (qb @ self.Kb.T).reshape(C, H, W) * self.nb
            return mg, mb
        R = self.R
        qg = np.zeros((C, H + 2 * R, W + 2 * R))
        qb = np.zeros((C, H + 2 * R, W + 2 * R))
        qg[:, R:R + H, R:R + W] = Q * self.ng
        qb[:, R:R + H, R:R + W] = Q * self.nb
        mg = np.zeros((C, H, W))
        mb = np.zeros((C, H, W))
        for dy, dx, kg, kb in self.taps:
            mg += kg * qg[:, R + dy:R + dy + H, R + dx:R + dx + W]
            if self.bilateral:
                mb += kb * qb[:, R + dy:R + dy + H, R + dx:R + dx + W]
        return mg * self.ng, mb * self.nb

    def step(self, Q):
        mg, mb = self.messages(Q)
        a = -self.U + self.prm['w_g'] * mg
        if self.bilateral:
            a = a + self.prm['w_b'] * mb
        return softmax(a)

    def run(self, num_iter, Q=None):
        Q = self.Q0 if Q is None else Q
        for _ in range(num_iter):
            Q = self.step(Q)
        return Q


def crf_inference(P, X, num_iter, bilateral=True, R=None, in255=False, untruncated=False, **kw):
    """P (B, C, H, W) probabilities, X (B, 3, H, W) image -> Q (B, C, H, W) float64."""
    return np.stack([ImageCRF(P[b], X[b], R=R, bilateral=bilateral, in255=in255,
                              untruncated=untruncated, **kw).run(num_iter) for b in range(len(P))])
