"""Float64 (torch, CPU) restatement of the standard DAE's backward pass on its 16-bit C8 leg
(StandardDAE(mma='bf16c8').backward_y, csrc/c8_grad.hip + the C8 conv kernels on the flipped filters) with the
leg's rounding points:
  * the flipped weights to bf16, round to nearest-even, when they are packed;
  * g_score to bf16 on its way in;
  * every C8 store to bf16 (RNE), once, from an fp32 sum: the conv outputs (with the skip's share added before the
    rounding), depool_bwd_c8 (its four-term sum runs in fp32 in the order k = 0, 1, 2, 3);
  * the ReLU gate and the mask select are exact;
  * the first layer's data gradient leaves as fp32.
Conv sums are exact to float64 here; the kernel's differ by fp32 accumulation only.  The backward takes the DePool2D
mask BYTES (bit dy * 2 + dx of a channel's byte: that position equals the window maximum) and the pooled maps as
inputs -- on the GPU the ones the forward wrote -- and `forward` produces them with the C8 forward's rounding points.
Conventions of oracle/dae_grad.py: every position equal to the window maximum receives the gradient, relu'(0) = 0.
TEST INFRASTRUCTURE: with the rounding switched off it is oracle/dae_grad.py (tests/test_c8_grad_ref.py)."""
import numpy as np
import torch
import torch.nn.functional as F


def bf16(t):
    """float64 -> nearest bf16 (ties to even) -> float64."""
    return t.to(torch.bfloat16).to(torch.float64)


def f32(t):
    return t.to(torch.float32).to(torch.float64)


def _same(t):
    return t


def _t(a):
    return a.to(torch.float64) if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a), dtype=torch.float64)


def center(big, small):
    return (big - small) // 2


def n_pool(concat_h, additional_pool):
    n = int(concat_h[-1][-1]) if 'pool' in concat_h[-1] else 0
    return n, n + additional_pool


# ---- DePool2D mask bytes ----
def pack_masks(pre, pooled):
    """uint8 (B, C, h2, w2): bit dy * 2 + dx set where pre[2 qy + dy, 2 qx + dx] == pooled[qy, qx] (the unpaired
    last row / column of an odd map belongs to no window)."""
    h2, w2 = pooled.shape[2], pooled.shape[3]
    out = torch.zeros(pooled.shape, dtype=torch.uint8)
    for k in range(4):
        eq = pre[:, :, (k >> 1):2 * h2:2, (k & 1):2 * w2:2] == pooled
        out |= eq.to(torch.uint8) << k
    return out


def unpack_masks(mask, hw):
    """bool (B, C, hw[0], hw[1]): the positions the bytes select; False past the last whole window."""
    B, C, h2, w2 = mask.shape
    out = torch.zeros((B, C) + tuple(hw), dtype=torch.bool)
    for k in range(4):
        out[:, :, (k >> 1):2 * h2:2, (k & 1):2 * w2:2] = ((mask >> k) & 1).bool()
    return out


def unpool(t, mask, hw):
    """DePool2D of t (B, C, h2, w2) under the bytes, at size hw."""
    sel = unpack_masks(mask, hw)
    rep = torch.zeros(sel.shape, dtype=t.dtype)
    h2, w2 = t.shape[2], t.shape[3]
    rep[:, :, :2 * h2, :2 * w2] = t.repeat_interleave(2, 2).repeat_interleave(2, 3)
    return torch.where(sel, rep, torch.zeros((), dtype=t.dtype))


def depool_bwd(g_u, mask, rounding=True):
    """sum over the selected positions of each window, k = 0, 1, 2, 3 from 0 -- in fp32 with the rounding points on
    (what depool_bwd_c8_kernel does before its one bf16 rounding, which the caller applies)."""
    B, C, h2, w2 = mask.shape
    dt = torch.float32 if rounding else torch.float64
    acc = torch.zeros(mask.shape, dtype=dt)
    for k in range(4):
        v = g_u[:, :, (k >> 1):2 * h2:2, (k & 1):2 * w2:2].to(dt)
        acc = acc + torch.where(((mask >> k) & 1).bool(), v, torch.zeros((), dtype=dt))
    return acc.to(torch.float64)


def relu_gate(g, pooled):
    return torch.where(pooled > 0, g, torch.zeros((), dtype=g.dtype))


def flipped(W):
    """(Cout, Cin, 3, 3) -> the backward-data filter (Cin, Cout, 3, 3), spatially flipped."""
    return W.transpose(0, 1).flip(2, 3).contiguous()


def embed(g, hw, off):
    out = torch.zeros(tuple(g.shape[:2]) + tuple(hw), dtype=g.dtype)
    out[:, :, off[0]:off[0] + g.shape[2], off[1]:off[1] + g.shape[3]] = g
    return out


def sqerr_softmax_bwd(score, y):
    """dE/dscore of E = sum (softmax(score) - y)^2 through the softmax only; (g_score, r)."""
    score, y = _t(score), _t(y)
    r = torch.softmax(score, 1)
    g_r = 2.0 * (r - y)
    return r * (g_r - (r * g_r).sum(1, keepdim=True)), r


def _first_pad(concat_h, padding):
    return padding if (len(concat_h) == 1 and concat_h[-1] != 'input' and padding > 0) else 1


def forward(params, h_list, y, rounding=True, concat_h=('pool4',), padding=100, n_filters=64,
            conv_before_pool=1, additional_pool=2, skip=True, unpool_type='trackind'):
    """The C8 forward (`StandardDAE._scores_c8`): {'score': (B, C, H, W), 'pooled': {level: (B, C, h2, w2)} as
    stored (bf16 values), 'masks': {level: uint8 bytes}, 'pre_hw': {level: (ph, pw)}}, float64 torch tensors.
    Rounding points: y, h and the weights to bf16; the h half of the conv behind a concat an fp32 map; max-pool and
    mask bytes from the unrounded results; every C8 store (pooled maps, decoder maps) to bf16; the scores fp32."""
    assert conv_before_pool == 1 and unpool_type in ('trackind', 'inverse')
    rw, rf = (bf16, f32) if rounding else (_same, _same)
    concat_h = list(concat_h)
    _, total = n_pool(concat_h, additional_pool)
    y = _t(y)
    t = rw(y)
    pooled, masks, pre_hw = {}, {}, {}
    for p in range(total):
        W, b = (_t(a) for a in params['conv%d_1' % (p + 1)])
        pad = _first_pad(concat_h, padding) if p == 0 else 1
        at = 'input' if p == 0 else 'pool%d' % p
        if at in concat_h:                                   # h first (P13)
            h = _t(h_list[concat_h.index(at)])
            ch = h.shape[1]
            hb = rf(F.conv2d(rw(h), rw(W[:, :ch]), b, padding=pad))
            z = F.conv2d(t, rw(W[:, ch:]), None, padding=pad) + hb
        else:
            z = F.conv2d(t, rw(W), b, padding=pad)
        pre = torch.relu(z)
        pl = F.max_pool2d(pre, 2)
        pre_hw[p + 1] = (pre.shape[2], pre.shape[3])
        masks[p + 1] = pack_masks(pre, pl)
        t = pooled[p + 1] = rw(pl)
    for p in range(total, 0, -1):
        W, b = (_t(a) for a in params['up_conv%d' % p])
        u = F.conv2d(unpool(t, masks[p], pre_hw[p]), rw(W), b, padding=1)
        other = pooled[p - 1] if p > 1 else y
        oh, ow = min(u.shape[2], other.shape[2]), min(u.shape[3], other.shape[3])
        cy, cx = center(u.shape[2], oh), center(u.shape[3], ow)
        u = u[:, :, cy:cy + oh, cx:cx + ow]
        if skip and p > 1:
            oy, ox = center(other.shape[2], oh), center(other.shape[3], ow)
            u = u + other[:, :, oy:oy + oh, ox:ox + ow]
        t = rw(u) if p > 1 else rf(u)
    return {'score': t, 'pooled': pooled, 'masks': masks, 'pre_hw': pre_hw}


def backward_y(params, g_score, y_shape, pooled, masks, rounding=True, concat_h=('pool4',), padding=100,
               n_filters=64, conv_before_pool=1, additional_pool=2, skip=True, unpool_type='trackind'):
    """dE/dy THROUGH the DAE (float64 numpy, (B, C, H, W)) for the upstream gradient g_score w.r.t. the score map:
    the walk of StandardDAE._adjoint_walk on C8 maps.  pooled / masks: {level: pooled map (values), mask bytes
    (B, C, h2, w2) uint8} of the forward."""
    assert conv_before_pool == 1 and unpool_type in ('trackind', 'inverse')
    rw, rf = (bf16, f32) if rounding else (_same, _same)
    concat_h = list(concat_h)
    _, total = n_pool(concat_h, additional_pool)
    pooled = {p: _t(v) for p, v in pooled.items()}
    masks = {p: torch.as_tensor(np.asarray(v)).to(torch.uint8) for p, v in masks.items()}
    H, W_ = int(y_shape[2]), int(y_shape[3])
    pad1 = _first_pad(concat_h, padding)
    pre_hw = {1: (H + 2 * pad1 - 2, W_ + 2 * pad1 - 2)}
    for p in range(2, total + 1):
        pre_hw[p] = (pooled[p - 1].shape[2], pooled[p - 1].shape[3])
    g_pool = {}
    g_f = rw(_t(g_score))
    for p in range(1, total + 1):                        # decoder, output to input
        ph, pw = pre_hw[p]
        other_hw = (pooled[p - 1].shape[2], pooled[p - 1].shape[3]) if p > 1 else (H, W_)
        oh, ow = min(ph, other_hw[0]), min(pw, other_hw[1])
        g_c = embed(g_f, (ph, pw), (center(ph, oh), center(pw, ow)))
        if skip and p > 1:
            g_pool[p - 1] = embed(g_f, other_hw, (center(other_hw[0], oh), center(other_hw[1], ow)))
        g_u = rw(F.conv2d(g_c, rw(flipped(_t(params['up_conv%d' % p][0]))), None, padding=1))
        g_f = rw(depool_bwd(g_u, masks[p], rounding))
        if p == total:
            g_f = relu_gate(g_f, pooled[p])
    g_pool[total] = g_f
    prev = [int(g_score.shape[1])] + [int(params['conv%d_1' % (p + 1)][0].shape[0]) for p in range(total)]
    g_in = None
    for p in range(total, 0, -1):                        # encoder, deep to shallow
        gp = g_pool[p]
        if p != total:
            gp = relu_gate(gp, pooled[p])
        Wc = _t(params['conv%d_1' % p][0])
        Wc = Wc[:, Wc.shape[1] - prev[p - 1]:]           # after a concat only the non-h half
        z = F.conv2d(unpool(gp, masks[p], pre_hw[p]), rw(flipped(Wc)), None, padding=1)
        if p > 1:
            acc = g_pool.get(p - 1)
            g_pool[p - 1] = rw(z if acc is None else z + acc)
        else:
            g_in = rf(z[:, :, pad1 - 1:pad1 - 1 + H, pad1 - 1:pad1 - 1 + W_])
    return g_in.numpy()


# ---- C8 layout (B, C/8, H, W, 8) <-> (B, C, H, W) on the host ----
def from_c8(t8, channels):
    """A C8 tensor of any dtype (host) -> (B, channels, H, W)."""
    B, C8n, H, W, _ = t8.shape
    return t8.permute(0, 1, 4, 2, 3).reshape(B, C8n * 8, H, W)[:, :channels]


def to_c8(t, chunks):
    """(B, C, H, W) -> (B, chunks, H, W, 8), channels past C zero."""
    B, C, H, W = t.shape
    full = torch.zeros((B, chunks * 8, H, W), dtype=t.dtype)
    full[:, :C] = t
    return full.reshape(B, chunks, 8, H, W).permute(0, 1, 3, 4, 2).contiguous()
