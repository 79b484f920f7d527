"""Float64 restatements, in plain numpy, of the host networks' small kernels: BatchNorm (csrc/bn.hip and the C8
statistics / fold of csrc/conv_c8_m16.hip), 2x2 max-pool and the materialised DePool2D (csrc/pool_unpool.hip,
forward kernels), the small-channel transposed convolution (csrc/deconv.hip, csrc/deconv_phase.hip) and the
NCHW <-> bf16 C8 converters (csrc/conv_c8_bf16.hip).  TEST INFRASTRUCTURE: no GPU code, no import of the
package's `ops`.  One function per `ops` wrapper with that wrapper's arguments; a tensor the wrapper writes in
place is returned as a new array (the caller's array is never modified).  tests/test_bn_pool_ref.py pins every
function to the oracle and to torch CPU float64; tests/test_gpu_bn_pool_deconv_edges.py compares the kernels
with them."""
import math

import numpy as np


def _f64(a):
    return np.asarray(a, dtype=np.float64)


# ---- BatchNorm -------------------------------------------------------------------------------------------------
def bn_stats(buf, c0, n, eps=1e-4):
    """(mean, inv_std) of channels [c0, c0 + n) of `buf` (B, Ctot, H, W) over (B, H, W): batch mean and BIASED
    variance, inv_std = 1 / sqrt(var + eps).  Two passes, every sum by math.fsum (exactly rounded), the second
    pass with the correction term of the residual mean: more accurate than any float64 kernel."""
    buf = _f64(buf)
    mean, inv_std = np.empty(n), np.empty(n)
    for j in range(n):
        v = buf[:, c0 + j].ravel()
        cnt = float(v.size)
        m = math.fsum(v) / cnt
        d = v - m
        r = math.fsum(d) / cnt                       # what the rounding of m left over
        var = math.fsum(d * d) / cnt - r * r
        mean[j] = m + r
        inv_std[j] = 1.0 / math.sqrt(max(var, 0.0) + eps)
    return mean, inv_std


def _per_channel(v):
    return _f64(v)[None, :, None, None]


def bn_relu(buf, n, beta, gamma, mean, inv_std):
    """relu((x - mean) * (gamma * inv_std) + beta) of the first n channels of `buf` -> dense (B, n, H, W).  The
    parameter vectors may be longer than n."""
    x = _f64(buf)[:, :n]
    beta, gamma, mean, inv_std = (_f64(v)[:n] for v in (beta, gamma, mean, inv_std))
    y = (x - _per_channel(mean)) * _per_channel(gamma * inv_std) + _per_channel(beta)
    return np.maximum(y, 0.0)


def bn_affine(x, bnp, window=None):
    """x = (x - mean) * (gamma * inv_std) + beta per channel on the window (y0, x0, h, w) of x's planes (default:
    everywhere); the rest of x as it was.  bnp = (beta, gamma, mean, inv_std)."""
    out = _f64(x).copy()
    B, C, H, W = out.shape
    y0, x0, wh, ww = window if window is not None else (0, 0, H, W)
    assert 0 <= y0 and 0 <= x0 and wh > 0 and ww > 0 and y0 + wh <= H and x0 + ww <= W, (out.shape, window)
    beta, gamma, mean, inv_std = (_f64(v) for v in bnp)
    w = out[:, :, y0:y0 + wh, x0:x0 + ww]
    out[:, :, y0:y0 + wh, x0:x0 + ww] = (w - _per_channel(mean)) * _per_channel(gamma * inv_std) + _per_channel(beta)
    return out


def bn_fold(beta, gamma, mean, inv_std, n):
    """(a, b) with max(a x + b, 0) == bn_relu(x): a = gamma inv_std, b = beta - mean a, first n channels."""
    beta, gamma, mean, inv_std = (_f64(v)[:n] for v in (beta, gamma, mean, inv_std))
    a = gamma * inv_std
    return a, beta - mean * a


# ---- 2x2 max-pool and DePool2D ---------------------------------------------------------------------------------
def _quads(x, h, w):
    """The four members of every 2 x 2 window, index (y & 1) * 2 + (x & 1); an odd last row / column is in none."""
    return [x[:, :, dy:2 * h:2, dx:2 * w:2] for dy in (0, 1) for dx in (0, 1)]


def maxpool2x2(x, out=None, window=None, mask=None):
    """2 x 2 max, stride 2, ignore_border: (B, C, H // 2, W // 2).  `window` = (y0, x0, h, w) in POOLED
    coordinates: only that region is produced, the rest is `out` (required then) as it was.  With `mask` (uint8,
    the pooled shape) returns (out, mask) with the DePool2D mask bytes of the same region: bit (y & 1) * 2 + (x & 1)
    is set iff that member of the window equals the maximum (every tie)."""
    x = np.asarray(x)
    B, C, H, W = x.shape
    h, w = H // 2, W // 2
    q = _quads(x, h, w)
    # max(a, b) = a > b ? a : b, rows first: of -0.0 and +0.0, which compare equal, the later one is returned
    gt = lambda a, b: np.where(a > b, a, b)
    full = gt(gt(q[0], q[1]), gt(q[2], q[3]))
    bits = np.zeros((B, C, h, w), np.uint8)
    for k in range(4):
        bits |= (q[k] == full).astype(np.uint8) << k
    y0, x0, wh, ww = window if window is not None else (0, 0, h, w)
    assert 0 <= y0 and 0 <= x0 and wh > 0 and ww > 0 and y0 + wh <= h and x0 + ww <= w, (x.shape, window)
    sel = (slice(None), slice(None), slice(y0, y0 + wh), slice(x0, x0 + ww))
    if out is None:
        assert window is None or (y0, x0, wh, ww) == (0, 0, h, w), 'a window needs the tensor it is written into'
        res = full.copy()
    else:
        res = np.array(out, dtype=x.dtype)
        res[sel] = full[sel]
    if mask is None:
        return res
    m = np.array(mask, dtype=np.uint8)
    m[sel] = bits[sel]
    return res, m


def unpool_eqmask(up, pre, pooled, out=None, window=None):
    """DePool2D, materialised: out[y, x] = (pre[y, x] == pooled[y / 2, x / 2]) ? up[y / 2, x / 2] : 0 for y < 2 h,
    x < 2 w and 0 in an odd last row / column.  `window` = (y0, x0, h, w) in the coordinates of `pre`: only that
    region is produced, the rest is `out` (required then) as it was."""
    up, pre, pooled = np.asarray(up), np.asarray(pre), np.asarray(pooled)
    B, C, H, W = pre.shape
    h, w = H // 2, W // 2
    assert up.shape == (B, C, h, w) == pooled.shape
    full = np.zeros(pre.shape, dtype=pre.dtype)
    rep = lambda a: np.repeat(np.repeat(a, 2, axis=2), 2, axis=3)
    full[:, :, :2 * h, :2 * w] = np.where(pre[:, :, :2 * h, :2 * w] == rep(pooled), rep(up), 0)
    if window is None:
        return full
    y0, x0, wh, ww = window
    assert 0 <= y0 and 0 <= x0 and wh > 0 and ww > 0 and y0 + wh <= H and x0 + ww <= W, (pre.shape, window)
    res = np.array(out, dtype=pre.dtype)
    res[:, :, y0:y0 + wh, x0:x0 + ww] = full[:, :, y0:y0 + wh, x0:x0 + ww]
    return res


# ---- transposed convolution ------------------------------------------------------------------------------------
def deconv(x, W, b, stride, add=None, add_off=(0, 0), window=None):
    """Lasagne Deconv2DLayer with its spatial flip (P3), W[in, out, K, K], any K and stride:
      full[c, s i + a, s j + b] += x[o, i, j] W[o, c, K - 1 - a, K - 1 - b],  full size (H - 1) s + K.
    `window` = (oy0, ox0, OH, OW) of the full output (default: all of it); `add` (B, Cout, AH, AW): its window of
    the same size at `add_off` is added; `b` may be None."""
    x, W = _f64(x), _f64(W)
    B, Cin, H, Wd = x.shape
    Cin2, Cout, K, K2 = W.shape
    assert Cin2 == Cin and K == K2
    s = int(stride)
    FH, FW = (H - 1) * s + K, (Wd - 1) * s + K
    full = np.zeros((B, Cout, FH, FW))
    for a in range(K):
        for c in range(K):
            full[:, :, a:a + (H - 1) * s + 1:s, c:c + (Wd - 1) * s + 1:s] += \
                np.einsum('bohw,oc->bchw', x, W[:, :, K - 1 - a, K - 1 - c])
    if b is not None:
        full += _per_channel(b)
    oy0, ox0, OH, OW = window if window is not None else (0, 0, FH, FW)
    assert 0 <= oy0 and 0 <= ox0 and OH > 0 and OW > 0 and oy0 + OH <= FH and ox0 + OW <= FW, (full.shape, window)
    out = full[:, :, oy0:oy0 + OH, ox0:ox0 + OW].copy()
    if add is not None:
        add = _f64(add)
        ay0, ax0 = add_off
        assert 0 <= ay0 and 0 <= ax0 and ay0 + OH <= add.shape[2] and ax0 + OW <= add.shape[3]
        out += add[:, :, ay0:ay0 + OH, ax0:ax0 + OW]
    return out


# ---- bf16 C8 ---------------------------------------------------------------------------------------------------
def bf16_round(x):
    """float32 -> the nearest bfloat16 (ties to even), as float32.  Finite inputs only."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16
    return u.astype(np.uint32).view(np.float32)


def nchw_to_c8_slice(x, out8, c0):
    """Channels of x (B, C, H, W) rounded to bf16 into channels [c0, c0 + C) of the C8 tensor `out8`
    (B, C8tot, H, W, 8; float32 holding bf16 values), channel c in lane c % 8 of chunk plane c // 8.  The
    ceil(C / 8) planes from c0 / 8 on are written whole: lanes past C are zero.  Every other plane as it was."""
    x = np.asarray(x, dtype=np.float32)
    B, C, H, W = x.shape
    assert c0 % 8 == 0 and out8.shape[0] == B and out8.shape[2:] == (H, W, 8)
    n8 = (C + 7) // 8
    assert c0 // 8 + n8 <= out8.shape[1]
    res = np.array(out8, dtype=np.float32)
    padded = np.zeros((B, n8 * 8, H, W), np.float32)
    padded[:, :C] = bf16_round(x)
    res[:, c0 // 8:c0 // 8 + n8] = padded.reshape(B, n8, 8, H, W).transpose(0, 1, 3, 4, 2)
    return res


def c8_slice_to_nchw(x8, c0, channels):
    """Channels [c0, c0 + channels) of the C8 tensor `x8` (B, C8tot, H, W, 8) -> (B, channels, H, W)."""
    x8 = np.asarray(x8)
    B, C8tot, H, W, _ = x8.shape
    assert c0 % 8 == 0 and c0 + channels <= C8tot * 8
    flat = x8.transpose(0, 1, 4, 2, 3).reshape(B, C8tot * 8, H, W)
    return flat[:, c0:c0 + channels].copy()


def bn_stats_c8(buf8, c0, n, eps=1e-4):
    """bn_stats of channels [c0, c0 + n) of the C8 tensor `buf8` (B, C8tot, H, W, 8): of the STORED values."""
    buf8 = np.asarray(buf8)
    B, C8tot, H, W, _ = buf8.shape
    return bn_stats(buf8.transpose(0, 1, 4, 2, 3).reshape(B, C8tot * 8, H, W), c0, n, eps)
