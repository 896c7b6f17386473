"""Put madnn's hand-written gfx950 kernels under an ARBITRARY model.

``distribute()`` calls :func:`use_madnn_kernels` on the model before tracing it,
so a Hugging Face GPT-2 / BERT / Llama (or any torch model) trains on the same
kernels as madnn's zoo, not only on the fused optimizer and bucket kernels:

* ``nn.LayerNorm``          -> :class:`FusedLayerNorm` (K3, fp32 statistics);
* ``*RMSNorm`` (HF Llama)   -> :class:`FusedRMSNorm` (K3 RMS variant);
* ``nn.BatchNorm2d``        -> :class:`FusedBatchNorm2d` (K5 NHWC kernels on
  channels_last activations, eager elsewhere);
* Hugging Face attention    -> the K8 MFMA flash-attention kernel, registered as
  the ``"madnn_k8"`` attention implementation (HF's ``AttentionInterface``):
  unmasked (or causal-only) bf16 attention with head dim 64/128 runs K8 straight
  from HF's [B, H, S, D] views, attention dropout included (in-kernel mask);
  a RIGHT-padded ``attention_mask`` runs K8 too, as per-sequence lengths
  (:func:`madnn_mask`); any other mask, position biases and decoding fall back to
  HF's SDPA path, and so does dropout with ``MADNN_ATTN_DROPOUT=0`` or under
  stream capture.

Every swap keeps parameter and buffer names (state dicts interchange with the
original model).  The reference had no kernels of its own at all.
"""
from __future__ import annotations

from typing import Dict

import torch
from torch import nn

from .. import ops
from .norm import FusedBatchNorm2d, FusedLayerNorm, FusedRMSNorm

ATTN_IMPL = "madnn_k8"
_registered = {"done": False}


def _is_rmsnorm(m: nn.Module) -> bool:
    if isinstance(m, FusedRMSNorm) or not type(m).__name__.endswith("RMSNorm"):
        return False
    w = getattr(m, "weight", None)
    eps = getattr(m, "variance_epsilon", getattr(m, "eps", None))
    return isinstance(w, nn.Parameter) and w.dim() == 1 and eps is not None and not list(m.children())


def _swap(model: nn.Module, counts: Dict[str, int]) -> None:
    for name, child in list(model.named_children()):
        new = None
        if type(child) is nn.LayerNorm and len(child.normalized_shape) == 1 and child.elementwise_affine \
                and ops.hidden_supported(child.normalized_shape[0]):
            new = FusedLayerNorm(child.normalized_shape, child.eps, bias=child.bias is not None,
                                 device=child.weight.device, dtype=child.weight.dtype)
            key = "layernorm"
        elif _is_rmsnorm(child) and ops.hidden_supported(child.weight.numel()):
            eps = getattr(child, "variance_epsilon", getattr(child, "eps", 1e-6))
            new = FusedRMSNorm(child.weight.numel(), eps=float(eps), device=child.weight.device,
                               dtype=child.weight.dtype)
            key = "rmsnorm"
        elif type(child) is nn.BatchNorm2d:
            dev = child.running_mean.device if child.track_running_stats else None
            new = FusedBatchNorm2d(child.num_features, child.eps, child.momentum, child.affine,
                                   child.track_running_stats, device=dev)
            key = "batchnorm"
        if new is None:
            _swap(child, counts)
            continue
        # adopt the original tensors themselves (no copy; works on the meta device too)
        new.load_state_dict(child.state_dict(), strict=True, assign=True)
        new.train(child.training)
        setattr(model, name, new)
        counts[key] = counts.get(key, 0) + 1


_SEQLENS = "_madnn_seqlens"   # by-product attached to the mask tensor: (int32 [B] lengths, causal)


def right_padded_lengths(attention_mask: torch.Tensor):
    """int32 [B] row sums of a 2-D padding mask if every row is ones followed by zeros (right-padded),
    else None.  One host sync (the comparison's result is read)."""
    m = attention_mask.to(torch.bool)
    lens = m.sum(-1)
    right = m == (torch.arange(m.size(-1), device=m.device)[None, :] < lens[:, None])
    return lens.to(torch.int32) if bool(right.all()) else None


def _has_cross_attention(config) -> bool:
    """A model whose config can build CROSS-attention masks (encoder-decoder models, decoders with
    ``add_cross_attention``): HF builds those through the same mask function from the ENCODER's padding
    mask, and with source and target padded to one length they look like self-attention masks."""
    return bool(getattr(config, "is_encoder_decoder", False) or getattr(config, "add_cross_attention", False))


def _is_cross_attention(module) -> bool:
    return bool(getattr(module, "is_cross_attention", False)) or "CrossAttention" in type(module).__name__


def madnn_mask(batch_size, q_length, kv_length, q_offset=0, kv_offset=0, mask_function=None, attention_mask=None,
               config=None, **kwargs):
    """The ``"madnn_k8"`` mask function: HF's ``sdpa_mask``, unchanged, whose result additionally
    carries the per-sequence lengths when the batch is right-padded self-attention over whole
    sequences -- a 2-D ``attention_mask``, ``q_length == kv_length``, both offsets 0, the stock causal
    or bidirectional ``mask_function``, no stream capture in progress (the check below reads a value
    on the host) and ``attention_mask == (arange < attention_mask.sum(-1))``.  The check costs one host
    sync per model forward (HF builds the mask once and hands it to every layer), not one per layer.
    :func:`madnn_attention_forward` runs K8 with ``seqlens`` on such a mask.

    Self-attention only: the kernels take ONE length per sequence for queries and keys alike.  Nothing
    is attached for a ``config`` (HF hands the model's to the mask function) that can cross-attend
    (:func:`_has_cross_attention`): the encoder's padding mask, applied to decoder queries of the same
    padded length, is indistinguishable here from a self-attention mask, and zeroing decoder rows past
    the SOURCE length would be wrong.  Such models keep SDPA for every masked call."""
    from transformers.masking_utils import bidirectional_mask_function, causal_mask_function, sdpa_mask

    if mask_function is None:
        mask_function = causal_mask_function
    mask = sdpa_mask(batch_size, q_length, kv_length, q_offset, kv_offset, mask_function=mask_function,
                     attention_mask=attention_mask, config=config, **kwargs)
    if (not _has_cross_attention(config) and isinstance(mask, torch.Tensor)
            and isinstance(attention_mask, torch.Tensor) and attention_mask.dim() == 2
            and attention_mask.size(-1) == kv_length and q_length == kv_length
            and isinstance(q_offset, int) and isinstance(kv_offset, int) and q_offset == 0 and kv_offset == 0
            and mask_function in (causal_mask_function, bidirectional_mask_function)
            and not (attention_mask.is_cuda and torch.cuda.is_current_stream_capturing())):
        lens = right_padded_lengths(attention_mask)
        if lens is not None:
            ops._attach(mask, _SEQLENS, (lens, mask_function is causal_mask_function))
    return mask


def madnn_attention_forward(module, query, key, value, attention_mask, dropout: float = 0.0, scaling=None,
                            is_causal=None, position_bias=None, **kwargs):
    """HF attention-interface entry: K8 for what it supports, HF SDPA for the rest.

    A mask that carries lengths (:func:`madnn_mask`: a right-padded batch) runs K8 with ``seqlens``.
    K8 then returns ZEROS at the padded query rows where SDPA returns values (there a padded query
    still attends to the valid keys); the valid positions, and therefore any loss that ignores the
    pads (labels of -100), are unaffected.  Any other non-null mask runs SDPA, and so does a
    cross-attention module whatever its mask carries (key lengths are not query lengths there)."""
    is_causal = is_causal if is_causal is not None else getattr(module, "is_causal", True)
    q_len, kv_len = query.shape[2], key.shape[2]
    lens = ops._attached(attention_mask, _SEQLENS) if isinstance(attention_mask, torch.Tensor) else None
    if lens is not None and _is_cross_attention(module):
        lens = None
    if ((attention_mask is None or lens is not None) and position_bias is None and q_len == kv_len
            and not kwargs.get("output_attentions", False)
            and ops.attention_supported(query, query.shape[-1], dropout) and key.dtype == query.dtype):
        if lens is not None:   # the mask holds the causal structure itself (HF passes is_causal=False with it)
            seqlens, causal = lens
        else:
            seqlens, causal = None, bool(is_causal and q_len > 1)
        o = ops.attention(query.transpose(1, 2), key.transpose(1, 2), value.transpose(1, 2),
                          causal=causal, scale=scaling, dropout_p=dropout, seqlens=seqlens)
        _stats["k8"] += 1
        return o, None
    from transformers.integrations.sdpa_attention import sdpa_attention_forward

    _stats["sdpa"] += 1
    return sdpa_attention_forward(module, query, key, value, attention_mask, dropout=dropout, scaling=scaling,
                                  is_causal=is_causal, position_bias=position_bias, **kwargs)


_stats = {"k8": 0, "sdpa": 0}


def attention_stats() -> Dict[str, int]:
    """How many HF attention calls ran K8 vs fell back to SDPA (diagnostics / tests)."""
    return dict(_stats)


def register_hf_attention() -> bool:
    if _registered["done"]:
        return True
    try:
        from transformers import AttentionInterface
        from transformers.masking_utils import AttentionMaskInterface
    except Exception:  # noqa: BLE001 - transformers absent or too old: nothing to route
        return False
    AttentionInterface.register(ATTN_IMPL, madnn_attention_forward)
    AttentionMaskInterface.register(ATTN_IMPL, madnn_mask)
    _registered["done"] = True
    return True


def _route_hf_attention(model: nn.Module) -> int:
    cfg = getattr(model, "config", None)
    if cfg is None or not hasattr(cfg, "_attn_implementation") or not register_hf_attention():
        return 0
    n = 0
    for m in model.modules():
        c = getattr(m, "config", None)
        if c is not None and hasattr(c, "_attn_implementation"):
            try:
                c._attn_implementation = ATTN_IMPL
            except Exception:  # noqa: BLE001
                c._attn_implementation_internal = ATTN_IMPL
            n += 1
    return n


def use_madnn_kernels(model: nn.Module) -> Dict[str, int]:
    """Swap in madnn's kernels (see module doc) in place; returns what was swapped."""
    counts: Dict[str, int] = {}
    _swap(model, counts)
    if _route_hf_attention(model):
        counts["hf_attention"] = 1
    return counts
