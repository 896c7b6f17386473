"""Eager PyTorch references for every madnn kernel.

Used (a) on CPU tensors, where the gloo tier of the test suite runs, and (b)
as the fp32 numerics oracle in the GPU kernel tests.  Semantics are the
kernels' exactly (same argument order, same optional fused pieces).
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch


def is_dense(t: torch.Tensor) -> bool:
    """True if ``t`` covers one gap-free, non-overlapping block of memory (any stride order)."""
    expected = 1
    for d in sorted(range(t.dim()), key=lambda d: t.stride(d)):
        if t.size(d) == 1:
            continue
        if t.stride(d) != expected:
            return False
        expected *= t.size(d)
    return True


def _flat_view(t: torch.Tensor) -> torch.Tensor:
    """1-D view of a dense tensor in its PHYSICAL order (e.g. NHWC for channels_last)."""
    if t.is_contiguous():
        return t.reshape(-1)
    if not is_dense(t):
        raise ValueError("bucket tensors must be non-overlapping and dense")
    perm = sorted(range(t.dim()), key=lambda d: -t.stride(d))
    return t.permute(*perm).reshape(-1)


def bucket_pack(tensors: Sequence[torch.Tensor], flat: torch.Tensor, offsets: Sequence[int], scale: float = 1.0):
    for t, off in zip(tensors, offsets):
        n = t.numel()
        v = _flat_view(t)
        flat[off:off + n].copy_(v.to(flat.dtype).mul(scale) if scale != 1.0 else v)


def bucket_unpack(tensors: Sequence[torch.Tensor], flat: torch.Tensor, offsets: Sequence[int], scale: float = 1.0):
    for t, off in zip(tensors, offsets):
        n = t.numel()
        src = flat[off:off + n]
        if scale != 1.0:
            src = src.to(torch.promote_types(src.dtype, torch.float32)).mul(scale)
        if t.is_contiguous():
            t.view(-1).copy_(src)
        else:
            perm = sorted(range(t.dim()), key=lambda d: -t.stride(d))
            t.permute(*perm).copy_(src.view([t.shape[d] for d in perm]))


def sgd_step(master, grad, mom, model, *, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False,
             first_step=False, grad_scale=1.0, dscale: Optional[torch.Tensor] = None):
    g = grad.to(torch.float32) * grad_scale
    if dscale is not None:
        g = g * dscale[0]
    if weight_decay:
        g = g + weight_decay * master
    if momentum:
        if first_step:
            mom.copy_(g)
        else:
            mom.mul_(momentum).add_(g, alpha=1.0 - dampening)
        g = g + momentum * mom if nesterov else mom
    master.add_(g, alpha=-lr)
    if model is not None:
        model.copy_(master)


def adam_step(master, grad, m1, m2, model, *, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, adamw=True,
              step=1, grad_scale=1.0, dscale: Optional[torch.Tensor] = None):
    g = grad.to(torch.float32) * grad_scale
    if dscale is not None:
        g = g * dscale[0]
    if weight_decay and not adamw:
        g = g + weight_decay * master
    if weight_decay and adamw:
        master.mul_(1.0 - lr * weight_decay)
    m1.mul_(beta1).add_(g, alpha=1.0 - beta1)
    m2.mul_(beta2).addcmul_(g, g, value=1.0 - beta2)
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    denom = m2.sqrt() / math.sqrt(bc2) + eps
    master.addcdiv_(m1, denom, value=-lr / bc1)
    if model is not None:
        model.copy_(master)


def grad_norm(flats: Sequence[torch.Tensor], max_norm: float = 0.0, scale: float = 1.0) -> torch.Tensor:
    sq = sum(float((f.to(torch.float32) * scale).pow(2).sum()) for f in flats)
    norm = math.sqrt(sq)
    coef = 1.0
    if max_norm > 0:
        coef = min(1.0, max_norm / (norm + 1e-6))
    return torch.tensor([norm, coef], dtype=torch.float32, device=flats[0].device)


def norm(x, weight, bias, eps, rms, residual=None):
    s = x + residual if residual is not None else x
    xf = s.float()
    if rms:
        y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    else:
        mu = xf.mean(-1, keepdim=True)
        var = (xf - mu).pow(2).mean(-1, keepdim=True)
        y = (xf - mu) * torch.rsqrt(var + eps)
    if weight is not None:
        y = y * weight.float()
    if bias is not None:
        y = y + bias.float()
    y = y.to(x.dtype)
    return (y, s) if residual is not None else y


def batch_norm_act(x, weight, bias, running_mean, running_var, num_batches_tracked=None, *, training, momentum=0.1,
                   eps=1e-5, relu=False, residual=None):
    import torch.nn.functional as F

    if training and num_batches_tracked is not None:
        num_batches_tracked.add_(1)
        if momentum is None:
            momentum = 1.0 / float(num_batches_tracked)
    y = F.batch_norm(x, running_mean, running_var, weight, bias, training, momentum if momentum is not None else 0.0,
                     eps)
    if residual is not None:
        y = y + residual
    if relu:
        y = torch.relu(y)
    return y


def cross_entropy(logits, targets, *, shift=False, vocab=None, ignore_index=-100):
    import torch.nn.functional as F

    v = vocab or logits.size(-1)
    if shift:
        logits, targets = logits[:, :-1], targets[:, 1:]
    return F.cross_entropy(logits[..., :v].reshape(-1, v).float(), targets.reshape(-1), ignore_index=ignore_index)


def attention_valid(seqlens: torch.Tensor, S: int) -> torch.Tensor:
    """bool [B, S]: position s of sequence b is a real token, ``s < clamp(seqlens[b], 0, S)``."""
    return torch.arange(S, device=seqlens.device)[None, :] < seqlens.clamp(0, S)[:, None]


def attention_seqlens_mask(seqlens: torch.Tensor, S: int, causal: bool) -> torch.Tensor:
    """bool [B, 1, S, S] attention mask of a right-padded batch (True = attend): a valid query row sees
    the valid keys (up to itself when causal).  A padded query row sees every key (up to itself when
    causal) so that no row is empty -- an empty softmax row is NaN, which the later ``where`` would drop
    in the forward but not in the backward; its output is replaced by zeros by the caller."""
    valid = attention_valid(seqlens, S)
    m = valid[:, None, None, :] | ~valid[:, None, :, None]
    if causal:
        m = m & torch.ones(S, S, dtype=torch.bool, device=seqlens.device).tril()
    return m


def attention(q, k, v, *, causal=True, scale=None, dropout_p=0.0, seqlens=None):
    """[B, S, H, D] / [B, S, Hkv, D] -> [B, S, H, D] via SDPA (fp32 oracle when given fp32).
    ``dropout_p`` is SDPA's own dropout (torch's mask, not K8's).  A ``scale`` that is not finite and
    positive is computed from plain ops in fp32 instead: SDPA's math path takes the square root of
    the scale, and its fused bf16 backward on the device returned NaN gradients for a negative one.

    ``seqlens`` (integer [B]): a right-padded batch, K8's contract (:func:`madnn.ops.attention`).
    Padded positions of q, k and v are replaced by zeros with ``torch.where`` before anything is
    computed (their values, NaN included, reach no result and their gradients are exact zeros), valid
    query rows see the valid keys only, and padded rows of the output are exact zeros."""
    import torch.nn.functional as F

    h, hkv = q.size(2), k.size(2)
    mask = None
    if seqlens is not None:
        S = q.size(1)
        seqlens = seqlens.to(q.device)
        valid = attention_valid(seqlens, S)[:, :, None, None]
        q, k, v = (torch.where(valid, t, torch.zeros((), dtype=t.dtype, device=t.device)) for t in (q, k, v))
        mask = attention_seqlens_mask(seqlens, S, causal)
    if scale is not None and not (math.isfinite(scale) and scale > 0):
        qt, kt, vt = (t.transpose(1, 2).float() for t in (q, k, v))
        if h != hkv:
            kt, vt = kt.repeat_interleave(h // hkv, dim=1), vt.repeat_interleave(h // hkv, dim=1)
        s = (qt @ kt.transpose(-1, -2)) * scale
        if mask is not None:
            s = s.masked_fill(~mask, float("-inf"))
        elif causal:
            n = s.size(-1)
            s = s.masked_fill(~torch.ones(n, n, dtype=torch.bool, device=s.device).tril(), float("-inf"))
        p = F.dropout(torch.softmax(s, dim=-1), dropout_p)
        o = (p @ vt).to(q.dtype).transpose(1, 2).contiguous()
    else:
        o = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), attn_mask=mask,
                                           dropout_p=dropout_p, is_causal=causal and mask is None, scale=scale,
                                           enable_gqa=h != hkv)
        o = o.transpose(1, 2).contiguous()
    if seqlens is not None:
        o = torch.where(valid, o, torch.zeros((), dtype=o.dtype, device=o.device))
    return o


DROPOUT_BITS = 8  # K8's dropout mask: one byte per attention probability


def attention_dropout_threshold(p: float) -> int:
    """K8 keeps an element iff its mask byte is below ``floor((1 - p) * 256 + 0.5)`` (p quantised to
    1/256; the kept ones are scaled by ``256 / threshold``).  Raises for p outside [0, 1) and for a p
    that quantises to keep-nothing."""
    if not 0.0 <= p < 1.0:
        raise ValueError(f"attention dropout p must be in [0, 1), got {p}")
    thr = int(math.floor((1.0 - float(p)) * 256.0 + 0.5))
    if thr < 1:
        raise ValueError(f"attention dropout p = {p} keeps nothing at the mask's 1/256 resolution")
    return thr


def attention_dropout_mask(B: int, H: int, S: int, p: float, seed: int, offset: int) -> torch.Tensor:
    """The keep mask of K8's attention dropout, bool [B, H, S, S] (h = query head), on the CPU in
    integer arithmetic: bit-identical to the device function ``drop_block`` of ``csrc/attn.hip``.
    Philox4x32-10, key (seed lo, seed hi ^ offset hi), counter (offset lo, b*H + h, q >> 2, k >> 2);
    the four output words are the 16 bytes of the 4 x 4 block: element (q, k) owns byte ``k & 3`` of
    word ``q & 3`` and is kept iff it is ``< threshold``."""
    import numpy as np

    thr = attention_dropout_threshold(p)
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    m32 = np.uint64(0xFFFFFFFF)
    nb = (S + 3) // 4
    shape = (B * H, nb, nb)
    c0 = np.full(shape, offset & 0xFFFFFFFF, dtype=np.uint64)
    c1 = np.broadcast_to(np.arange(B * H, dtype=np.uint64)[:, None, None], shape).copy()
    c2 = np.broadcast_to(np.arange(nb, dtype=np.uint64)[None, :, None], shape).copy()
    c3 = np.broadcast_to(np.arange(nb, dtype=np.uint64)[None, None, :], shape).copy()
    k0, k1 = seed & 0xFFFFFFFF, ((seed >> 32) ^ (offset >> 32)) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2   # 32 x 32 -> 64 bit, exact
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & m32,
                          (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & m32)
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    words = np.stack([c0, c1, c2, c3], axis=2)                              # [BH, qb, q & 3, kb]
    shifts = (np.arange(4, dtype=np.uint64) * np.uint64(8))
    byts = (words[..., None] >> shifts) & np.uint64(0xFF)                   # [BH, qb, q & 3, kb, k & 3]
    keep = (byts < np.uint64(thr)).reshape(B, H, 4 * nb, 4 * nb)[:, :, :S, :S]
    return torch.from_numpy(np.ascontiguousarray(keep))


def hidden_dropout_mask(rows: int, H: int, p: float, seed: int, offset: int, row0: int = 0) -> torch.Tensor:
    """The keep mask of the hidden (residual) dropout of K3 / K16 for rows ``row0 .. row0 + rows - 1``
    of a ``[*, H]`` activation, bool [rows, H], on the CPU in integer arithmetic: bit-identical to the
    device function ``hidden_block`` of ``csrc/dropout.h``.  Philox4x32-10, key (seed lo, seed hi ^
    offset hi) as K8's, counter (offset lo, row lo, row hi, col >> 4); the four output words are the 16
    mask bytes of columns ``16 (col >> 4) .. + 15``: column ``col`` owns byte ``col & 3`` of word
    ``(col >> 2) & 3`` and is kept iff it is ``< threshold``.  A pure function of (seed, offset, row,
    col, threshold): ``H`` only bounds the columns returned."""
    import numpy as np

    thr = attention_dropout_threshold(p)
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    m32 = np.uint64(0xFFFFFFFF)
    nb = (H + 15) // 16
    shape = (rows, nb)
    r = np.arange(rows, dtype=np.uint64) + np.uint64(int(row0))
    c0 = np.full(shape, offset & 0xFFFFFFFF, dtype=np.uint64)
    c1 = np.broadcast_to((r & m32)[:, None], shape).copy()
    c2 = np.broadcast_to((r >> np.uint64(32))[:, None], shape).copy()
    c3 = np.broadcast_to(np.arange(nb, dtype=np.uint64)[None, :], shape).copy()
    k0, k1 = seed & 0xFFFFFFFF, ((seed >> 32) ^ (offset >> 32)) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2   # 32 x 32 -> 64 bit, exact
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & m32,
                          (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & m32)
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    words = np.stack([c0, c1, c2, c3], axis=2)                              # [rows, block, word]
    shifts = (np.arange(4, dtype=np.uint64) * np.uint64(8))
    byts = (words[..., None] >> shifts) & np.uint64(0xFF)                   # [rows, block, word, byte]
    keep = (byts < np.uint64(thr)).reshape(rows, 16 * nb)[:, :H]
    return torch.from_numpy(np.ascontiguousarray(keep))
