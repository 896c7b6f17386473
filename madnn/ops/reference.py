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


def segment_bounds(ids: torch.Tensor) -> torch.Tensor:
    """int32 [B, 2, S] document bounds of packed rows from integer ids [B, S], in plain torch ops (the
    host mirror of K8's ``attn_segment_bounds_kernel``).  A document is a maximal run of equal
    consecutive ids; ``[:, 0, s]`` is the index of the first token of token s's document, ``[:, 1, s]``
    one past its last."""
    if ids.dim() != 2 or ids.is_floating_point() or ids.dtype == torch.bool:
        raise ValueError(f"segment ids must be an integer [B, S] tensor, got {tuple(ids.shape)} {ids.dtype}")
    B, S = ids.shape
    ids = ids.to(torch.int32)   # as the device path: ids are compared as int32 values (wider ones wrap)
    pos = torch.arange(S, device=ids.device).expand(B, S)
    start = torch.ones(B, S, dtype=torch.bool, device=ids.device)
    start[:, 1:] = ids[:, 1:] != ids[:, :-1]
    lo = torch.cummax(torch.where(start, pos, torch.zeros_like(pos)), dim=1).values
    nxt = torch.full_like(pos, S)           # nxt[s] = s + 1 if a document starts there, else S
    nxt[:, :-1] = torch.where(start[:, 1:], pos[:, 1:], nxt[:, 1:])
    hi = torch.cummin(nxt.flip(1), dim=1).values.flip(1)
    return torch.stack([lo, hi], dim=1).to(torch.int32)


def _segments_bounds(segments: torch.Tensor, B: int, S: int) -> torch.Tensor:
    """``segments`` as bounds [B, 2, S]: ids [B, S] are scanned, bounds are taken as they are."""
    if segments.dim() == 2 and tuple(segments.shape) == (B, S):
        return segment_bounds(segments)
    if segments.dim() == 3 and tuple(segments.shape) == (B, 2, S) and not segments.is_floating_point():
        return segments
    raise ValueError(f"segments must be integer ids [B = {B}, S = {S}] or bounds [B, 2, S], got "
                     f"{tuple(segments.shape)} {segments.dtype}")


def attention_segments_mask(bounds: torch.Tensor, causal: bool) -> torch.Tensor:
    """bool [B, 1, S, S] block-diagonal mask of packed rows from their bounds [B, 2, S] (True =
    attend): query q sees the keys ``lo[q] <= k < hi[q]``, up to itself when causal."""
    S = bounds.size(2)
    kpos = torch.arange(S, device=bounds.device)[None, None, :]
    m = (kpos >= bounds[:, 0, :, None]) & (kpos < bounds[:, 1, :, None])
    if causal:
        m = m & torch.ones(S, S, dtype=torch.bool, device=bounds.device).tril()
    return m[:, None]


def attention(q, k, v, *, causal=True, scale=None, dropout_p=0.0, seqlens=None, segments=None):
    """[B, S, H, D] / [B, S, Hkv, D] -> [B, S, H, D] via SDPA (fp32 oracle when given fp32).
    ``dropout_p`` is SDPA's own dropout (torch's mask, not K8's).  A ``scale`` that is not finite and
    positive is computed from plain ops in fp32 instead: SDPA's math path takes the square root of
    the scale, and its fused bf16 backward on the device returned NaN gradients for a negative one.

    ``seqlens`` (integer [B]): a right-padded batch, K8's contract (:func:`madnn.ops.attention`).
    Padded positions of q, k and v are replaced by zeros with ``torch.where`` before anything is
    computed (their values, NaN included, reach no result and their gradients are exact zeros), valid
    query rows see the valid keys only, and padded rows of the output are exact zeros.

    ``segments`` (integer ids [B, S], or their :func:`segment_bounds` [B, 2, S]): packed rows, every
    token attends inside its own document only (up to itself when causal), through the materialised
    block-diagonal mask.  Not together with ``seqlens`` (``ValueError``): a padded tail is simply a
    document of its own."""
    import torch.nn.functional as F

    h, hkv = q.size(2), k.size(2)
    mask = None
    if segments is not None:
        if seqlens is not None:
            raise ValueError("attention: segments and seqlens exclude each other")
        mask = attention_segments_mask(_segments_bounds(segments.to(q.device), q.size(0), q.size(1)), causal)
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


# --------------------------------------------------------------------------- K17 (fp8 Linear)
# format -> (torch dtype, largest finite value FMAX, EF with FMAX = 0.875 * 2^EF)
FP8_FORMATS = {"e4m3": (torch.float8_e4m3fn, 448.0, 9), "e5m2": (torch.float8_e5m2, 57344.0, 16)}


def fp8_scale(amax, fmt: str = "e4m3") -> torch.Tensor:
    """The per-tensor scale of the fp8 path, fp32: ``2^floor(log2(FMAX / amax))``, formed from amax's
    exponent and fraction without a rounded division (``amax = m 2^ea`` with m in [0.5, 1): the exponent is
    ``EF - ea``, one less when ``m > 0.875``).  ``amax == 0`` gives 1; the exponent is clamped to +-126 so
    that the scale and its reciprocal are normal fp32 numbers (a subnormal amax meets the clamp)."""
    ef = FP8_FORMATS[fmt][2]
    a = torch.as_tensor(amax).detach().to(torch.float32)
    m, ea = torch.frexp(a)
    e = ef - ea.to(torch.int32) - (m > 0.875).to(torch.int32)
    e = torch.where(torch.isfinite(a), e, torch.full_like(e, -126)).clamp(-126, 126)
    e = torch.where(a == 0, torch.zeros_like(e), e)
    return ((e + 127) << 23).view(torch.float32)


def fp8_quantize(x: torch.Tensor, fmt: str = "e4m3"):
    """``(q, scale)``: ``x * scale`` (exact in fp32: the scale is a power of two) cast to the fp8 format
    with round-to-nearest-even, and the 1-element fp32 scale of :func:`fp8_scale`."""
    scale = fp8_scale(x.detach().abs().max(), fmt).reshape(1)
    return (x.detach().to(torch.float32) * scale).to(FP8_FORMATS[fmt][0]), scale


class _LinearFp8(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, residual, wgrad=False):
        acc = torch.float32 if x.dtype in (torch.bfloat16, torch.float16) else x.dtype
        x8, sx = fp8_quantize(x, "e4m3")
        w8, sw = fp8_quantize(w, "e4m3")
        wd = w8.to(acc) / sw.to(acc)
        y = (x8.to(acc) / sx.to(acc)) @ wd.t()
        if b is not None:
            y = y + b.to(acc)
        if residual is not None:
            y = y + residual.to(acc)
        # with wgrad the backward sees the dequantised e4m3 image of x, not x
        ctx.save_for_backward(x8.to(acc) / sx.to(acc) if wgrad else x, wd)
        ctx.meta = (acc, x.dtype, w.dtype, b.dtype if b is not None else None, residual is not None, wgrad)
        return y.to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        x, wd = ctx.saved_tensors
        acc, xdt, wdt, bdt, has_res, wgrad = ctx.meta
        g8, sg = fp8_quantize(g, "e5m2")
        gd = g8.to(acc) / sg.to(acc)
        dx = (gd @ wd).to(xdt)
        g2, x2 = g.reshape(-1, g.shape[-1]).to(acc), x.reshape(-1, x.shape[-1]).to(acc)
        dw = ((gd.reshape(-1, g.shape[-1]) if wgrad else g2).t() @ x2).to(wdt)
        db = g2.sum(0).to(bdt) if bdt is not None else None
        return dx, dw, db, (g if has_res else None), None


def linear_fp8(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor] = None,
               residual: Optional[torch.Tensor] = None, wgrad: bool = False) -> torch.Tensor:
    """The FP8 Linear of ``ops.linear(fp8=True)`` in plain torch, on any device and in any float dtype: the
    forward multiplies the dequantised e4m3 images of ``x`` and ``w`` (accumulating in fp32, or in the
    input's dtype when that is wider), adds bias and residual and rounds once; the data gradient multiplies
    the dequantised e5m2 image of the output gradient with the same dequantised weight; the weight gradient
    uses the unquantised tensors -- or, with ``wgrad`` (``ops.linear(fp8="wgrad")``, K17W), the same two
    dequantised images: ``dW = (dy8 / sg)^T @ (x8 / sx)``, accumulated likewise and rounded once."""
    return _LinearFp8.apply(x, w, b, residual, wgrad)


# --------------------------------------------------------------------------- K17X (MX fp8 Linear)
MX_BLOCK = 32
MX_EMAX = {"e4m3": 8, "e5m2": 15}   # exponent of the format's largest binade


def mx_quantize(x: torch.Tensor, fmt: str = "e4m3"):
    """``(q, e)``: OCP MX quantisation of ``x`` in blocks of 32 along its last dimension (a multiple of 32).
    ``e`` (uint8, last dimension / 32) is the E8M0 scale ``clamp(floor(log2 amax_block) + 127 - emax, 0, 254)``,
    127 for an all-zero block; ``q`` is ``x * 2^(127 - e)`` (exact), clamped to the format's +-FMAX and cast with
    round-to-nearest-even.  ``x ~ q * 2^(e - 127)`` (:func:`mx_dequantize`)."""
    dtype, fmax, _ = FP8_FORMATS[fmt]
    xd = x.detach()
    xf = xd.to(torch.float32) if xd.dtype in (torch.bfloat16, torch.float16) else xd
    xb = xf.reshape(*xf.shape[:-1], xf.shape[-1] // MX_BLOCK, MX_BLOCK)
    amax = xb.abs().amax(-1)
    _, ea = torch.frexp(amax)                      # amax = m 2^ea, m in [0.5, 1): floor(log2 amax) = ea - 1
    e = (ea.to(torch.int32) - 1 + 127 - MX_EMAX[fmt]).clamp(0, 254)
    e = torch.where(amax == 0, torch.full_like(e, 127), e)
    q = (xb * torch.exp2((127 - e).to(xb.dtype)).unsqueeze(-1)).clamp(-fmax, fmax).reshape(xf.shape).to(dtype)
    return q, e.to(torch.uint8)


def mx_dequantize(q: torch.Tensor, e: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """``q * 2^(e - 127)`` block by block along the last dimension, in ``dtype``."""
    s = torch.exp2(e.to(dtype) - 127).repeat_interleave(MX_BLOCK, -1)
    return q.to(dtype) * s


def mx_quantize_columns(x: torch.Tensor, fmt: str = "e4m3"):
    """``(qc, ec)``: the 2-D ``x`` [R, C] quantised in blocks of 32 ROWS per column, for a GEMM that reduces over
    the rows (the weight gradient, K17XW): :func:`mx_quantize` of ``x.t()`` with the rows zero-padded to a multiple
    of 32, transposed back and cut to ``R``.  ``qc`` [R, C], ``ec`` uint8 [ceil(R / 32), C]; any ``R``."""
    r = x.shape[0]
    qt, et = mx_quantize(torch.nn.functional.pad(x.detach(), (0, 0, 0, -r % MX_BLOCK)).t(), fmt)
    return qt.t()[:r].contiguous(), et.t().contiguous()


def mx_dequantize_columns(qc: torch.Tensor, ec: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """``qc[r, c] * 2^(ec[r // 32, c] - 127)`` in ``dtype``."""
    return qc.to(dtype) * torch.exp2(ec.to(dtype) - 127).repeat_interleave(MX_BLOCK, 0)[:qc.shape[0]]


class _LinearMx(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, residual, wgrad=False):
        acc = torch.float32 if x.dtype in (torch.bfloat16, torch.float16) else x.dtype
        y = mx_dequantize(*mx_quantize(x, "e4m3"), acc) @ mx_dequantize(*mx_quantize(w, "e4m3"), acc).t()
        if b is not None:
            y = y + b.to(acc)
        if residual is not None:
            y = y + residual.to(acc)
        # with wgrad the backward sees the token-blocked e4m3 image of x, not x
        xs = mx_dequantize_columns(*mx_quantize_columns(x.reshape(-1, x.shape[-1]), "e4m3"), acc) if wgrad else x
        # the data gradient reduces over out-features: W^T quantised anew in blocks along them
        ctx.save_for_backward(xs, mx_dequantize(*mx_quantize(w.t(), "e4m3"), acc))
        ctx.meta = (acc, x.dtype, w.dtype, b.dtype if b is not None else None, residual is not None, wgrad)
        return y.to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        x, wtd = ctx.saved_tensors
        acc, xdt, wdt, bdt, has_res, wgrad = ctx.meta
        dx = (mx_dequantize(*mx_quantize(g, "e4m3"), acc) @ wtd.t()).to(xdt)
        g2, x2 = g.reshape(-1, g.shape[-1]).to(acc), x.reshape(-1, x.shape[-1]).to(acc)
        gw = mx_dequantize_columns(*mx_quantize_columns(g.reshape(-1, g.shape[-1]), "e4m3"), acc) if wgrad else g2
        dw = (gw.t() @ x2).to(wdt)
        db = g2.sum(0).to(bdt) if bdt is not None else None
        return dx, dw, db, (g if has_res else None), None


def linear_mx(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor] = None,
              residual: Optional[torch.Tensor] = None, wgrad: bool = False) -> torch.Tensor:
    """The MX FP8 Linear of ``ops.linear(fp8="mx")`` in plain torch, on any device and in any float dtype: the
    forward multiplies the dequantised block-scaled e4m3 images of ``x`` and ``w`` (blocks of 32 along
    in-features), adds bias and residual and rounds once; the data gradient multiplies the dequantised e4m3
    image of the output gradient with that of ``w`` RE-QUANTISED in blocks along out-features (its reduction);
    weight, bias and residual gradients use the unquantised tensors -- or, with ``wgrad``
    (``ops.linear(fp8="mx_wgrad")``, K17XW), the weight gradient multiplies the e4m3 images of the output gradient
    and of ``x`` quantised a second time in blocks of 32 TOKENS per column (:func:`mx_quantize_columns`):
    ``dW = dq(dy_c)^T @ dq(x_c)``, accumulated as the other products and rounded once.  Feature counts are
    multiples of 32."""
    return _LinearMx.apply(x, w, b, residual, wgrad)
