"""Float64 restatements, in plain numpy, of the per-pixel tail (csrc/tail.hip, tail_math.h), the metrics
accumulator (csrc/metrics.hip) and the two pool adjoints (csrc/pool_unpool.hip).  TEST INFRASTRUCTURE: no
GPU code, no import of the package's `ops`.  One function per operation with the arguments of its `ops`
wrapper, except that the `RefineState` of the wrappers is spelled out as the arrays it holds.
tests/test_tail_ref.py pins every function to the oracle or to float64 autograd; tests/test_gpu_tail_edges.py
compares the kernels with them."""
import numpy as np


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _window(score, H, W, off):
    SH, SW = score.shape[2:]
    sy0, sx0 = off if off is not None else ((SH - H) // 2, (SW - W) // 2)
    assert 0 <= sy0 and 0 <= sx0 and sy0 + H <= SH and sx0 + W <= SW, (score.shape, H, W, off)
    return _f64(score)[:, :, sy0:sy0 + H, sx0:sx0 + W]


def _softmax(v):
    e = np.exp(v - v.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def crop_softmax(score, H, W, off=None, minuend=None):
    """softmax over the channels of the (H, W) window of `score` at `off` (default: the centre crop,
    (dim - target) // 2); with `minuend`: minuend - softmax."""
    r = _softmax(_window(score, H, W, off))
    return r if minuend is None else _f64(minuend) - r


def _clipped_step(y, grad, active, step):
    """(y - step * grad clipped to [0, 1] for the images with a non-zero `active`, the others unchanged;
    the per-image mean over pixels of the per-pixel L2 norm of grad -- of every image)."""
    new = np.clip(y - float(step) * grad, 0.0, 1.0)
    on = np.asarray(active) != 0
    new = np.where(on[:, None, None, None], new, y)
    norms = np.sqrt((grad * grad).sum(axis=1)).mean(axis=(1, 2))
    return new, norms


def refine_step(score, y, active, step, off=None):
    """r = softmax(score window); de = y - r; y <- clip(y - step * de, 0, 1).  Returns (new y, norms)."""
    y = _f64(y)
    r = _softmax(_window(score, y.shape[2], y.shape[3], off))
    return _clipped_step(y, y - r, active, step)


def sqerr_softmax_bwd(score, y, off=None):
    """dE/dscore of E = sum (softmax(score window) - y)^2:  g_c = r_c (g_r_c - sum_k r_k g_r_k),
    g_r = 2 (r - y)."""
    y = _f64(y)
    r = _softmax(_window(score, y.shape[2], y.shape[3], off))
    gr = 2.0 * (r - y)
    return r * (gr - (r * gr).sum(axis=1, keepdims=True))


def grad_step(score, gthrough, y, active, step, off=None):
    """grad = gthrough - 2 (r - y); y <- clip(y - step * grad, 0, 1).  Returns (new y, norms)."""
    y = _f64(y)
    r = _softmax(_window(score, y.shape[2], y.shape[3], off))
    return _clipped_step(y, _f64(gthrough) - 2.0 * (r - y), active, step)


def finalize(sums, active, iters, last_norm, HW, eps):
    """The early-stop decision from the per-image sums of the per-pixel norms.  For the images that were
    active: iters += 1, last_norm = sum / HW, active = 0 iff that norm < eps; the others keep all three.
    Returns new (active, iters, last_norm)."""
    active = np.array(active, dtype=np.int32)
    iters = np.array(iters, dtype=np.int32)
    last_norm = np.array(last_norm, dtype=np.float64)
    for b in range(active.shape[0]):
        if active[b]:
            norm = float(sums[b]) / float(HW)
            iters[b] += 1
            last_norm[b] = norm
            if norm < eps:
                active[b] = 0
    return active, iters, last_norm


def confusion(y, t, active=None):
    """cm[i, j] = number of pixels with argmax(prediction) == i and argmax(target) == j: C x (C + 1), the
    target's void plane last, np.argmax = the first maximal index on both sides.  sums = [sum over pixels of
    mean_c((y - t)^2) * mask, sum mask] with mask = t[:, :C].sum(1).  With `active` only the images whose
    flag is non-zero count."""
    y, t = _f64(y), _f64(t)
    B, C = y.shape[:2]
    assert t.shape == (B, C + 1) + y.shape[2:]
    if active is not None:
        on = np.asarray(active) != 0
        y, t = y[on], t[on]
    p = np.argmax(y, axis=1).ravel()
    q = np.argmax(t, axis=1).ravel()
    cm = np.zeros((C, C + 1), dtype=np.int64)
    np.add.at(cm, (p, q), 1)
    mask = t[:, :C].sum(axis=1)
    loss = ((y - t[:, :C]) ** 2).mean(axis=1)
    return cm, np.array([(loss * mask).sum(), mask.sum()], dtype=np.float64)


def _windows(a, h, w):
    """(B, C, h, 2, w, 2) view of the 2 x 2 windows of `a` (an odd last row / column belongs to none)."""
    B, C = a.shape[:2]
    return a[:, :, :2 * h, :2 * w].reshape(B, C, h, 2, w, 2)


def depool_bwd(gout, pre, pooled):
    """Adjoint of DePool2D with respect to its input: g_up[i, j] = the sum over the 2 x 2 window of
    (pre == pooled[i, j]) ? g_out : 0 -- every tied position counts, no gradient through the mask."""
    gout, pre, pooled = _f64(gout), _f64(pre), _f64(pooled)
    h, w = pooled.shape[2:]
    assert (h, w) == (pre.shape[2] // 2, pre.shape[3] // 2) and gout.shape == pre.shape
    eq = _windows(pre, h, w) == pooled[:, :, :, None, :, None]
    return np.where(eq, _windows(gout, h, w), 0.0).sum(axis=(3, 5))


def pool_relu_bwd(gpool, pre, pooled):
    """Adjoint of maxpool2x2(relu(z)) with respect to z, given pre = relu(z):
    g_z[y, x] = (pre == pooled[y/2, x/2] and pre > 0) ? g_pool[y/2, x/2] : 0 -- every position equal to the
    window maximum receives the gradient, relu'(0) = 0, an odd last row / column gets 0."""
    gpool, pre, pooled = _f64(gpool), _f64(pre), _f64(pooled)
    h, w = pooled.shape[2:]
    assert (h, w) == (pre.shape[2] // 2, pre.shape[3] // 2) and gpool.shape == pooled.shape
    win = _windows(pre, h, w)
    take = (win == pooled[:, :, :, None, :, None]) & (win > 0)
    gz = np.zeros_like(pre)
    gz[:, :, :2 * h, :2 * w] = np.where(take, gpool[:, :, :, None, :, None], 0.0).reshape(
        pre.shape[0], pre.shape[1], 2 * h, 2 * w)
    return gz


def to_c8_bf16(y, chunks=None):
    """The bf16 C8 mirror of a float32 map y (B, C, H, W): torch's round-to-nearest-even y.to(bfloat16), laid
    out (B, chunks, H, W, 8) with channel c in lane c % 8 of chunk c // 8; lanes >= C and whole chunks past
    ceil(C / 8) are zero.  A torch CPU tensor."""
    import torch
    yb = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).to(torch.bfloat16)
    B, C, H, W = yb.shape
    need = (C + 7) // 8
    chunks = need if chunks is None else int(chunks)
    assert chunks >= need
    out = torch.zeros((B, chunks, H, W, 8), dtype=torch.bfloat16)
    for c in range(C):
        out[:, c // 8, :, :, c % 8] = yb[:, c]
    return out
