"""The in-model caller of the attention path: minitorch's ``MultiHeadAttention`` data flow
(``minitorch/modules_transfomer.py:67-157``: project -> split heads -> flash attention -> merge heads -> out projection)
over device-resident tensors, with the head split / merge FUSED into the kernels.

The reference materialises four full-tensor copies per layer around its flash operator:
``projection(x).view(B, N, H, d).permute(0, 2, 1, 3)`` followed by ``.contiguous()`` for q, k and v (:80-88, :113-115) and
``output.permute(0, 2, 1, 3).contiguous()`` for the result (:152).  Here the projection's ``(B, N, H*d)`` output is handed to the
kernels as ``[B][N][H][d]`` (``fa_mi355x_fwd_layout / _bwd_layout``, element (b, n, h, :) at ((b*N + n)*H + h)*d) and the
attention output comes back in that layout, i.e. already merged: no permute, no copy, forward or backward.

Only the attention operator is this repository's product; the projections are the caller's GEMMs (the reference runs them on
its own matmul kernels, ``src/combine.cu:150-252``, out of scope per SURVEY.md section 2) and are plain ``torch.matmul`` here.
LayerNorm, the feed-forward block and the embedding of ``DecoderLM`` (:255-351) are out of scope for the same reason:
``attention_stack`` chains residual attention layers only, which is what exercises the operator the way the 4-layer model does
(causal, forward and backward through several layers).
"""
from __future__ import annotations

import collections
import math
import numbers

import torch

from . import _lib, device_ops


def _attention(q, k, v, causal, layout, softmax_scale=None):
    """flash_attn2 with autograd (``q.flash_attn2(kT, v, self.causal)``, modules_transfomer.py:119-120)."""
    return device_ops._FlashAttnFn.apply(q, k, v, causal, _lib.FA_VARIANT_FA2, layout, softmax_scale)


LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453


def _expand_kv(t, n_head):
    """(B, N, Hkv, d) -> (B, N, n_head, d): every kv head repeated for the G = n_head // Hkv query heads that read it (one copy; under
    autograd its backward sums the group's gradients).  The tensor itself when Hkv == n_head."""
    B, N, Hkv, d = t.shape
    if Hkv == n_head:
        return t
    return t[:, :, :, None, :].expand(B, N, Hkv, n_head // Hkv, d).reshape(B, N, n_head, d)


class Rotary:
    """The rotary position embedding of a stack: the (cos, sin) tables (contiguous float32 (max_pos, rot / 2) on the stack's device,
    device_ops.rotary_table or the caller's own), ``interleaved`` (GPT-J pairs (x[2j], x[2j+1]) instead of NeoX / Llama pairs
    (x[j], x[j + rot/2])) and ``rot`` = the rotary dimension, which may be smaller than the head dim (the other columns pass)."""

    def __init__(self, cos, sin, interleaved: bool = False):
        if cos is None or sin is None:
            raise ValueError("Rotary needs both tables, cos and sin")
        self.rot, self.max_pos, _ = device_ops._check_rotary(cos, sin, getattr(cos, "device", None), interleaved)
        self.cos, self.sin, self.interleaved = cos, sin, bool(interleaved)

    @classmethod
    def table(cls, max_pos, rot, base=10000.0, device=None, interleaved: bool = False):
        return cls(*device_ops.rotary_table(max_pos, rot, base, device), interleaved)

    def keywords(self):
        """The keywords that make a device_ops KV-cache call a roped one."""
        return dict(rotary_cos=self.cos, rotary_sin=self.sin, rotary_interleaved=self.interleaved)

    def apply(self, t, seqlen_offsets=None):
        """t (B, N, heads, d) rotated at positions seqlen_offsets[b] + i (None: i); differentiable."""
        return device_ops.apply_rotary(t, self.cos, self.sin, seqlen_offsets, self.interleaved)


def multi_head_attention(x, wq, wk, wv, wo, n_head: int, causal: bool = True, fused_layout: bool = True, fold_scale: bool = False,
                         rope=None, window=None, sink=None, softcap=None, sink_logits=None):
    """MultiHeadAttention.forward (modules_transfomer.py:141-157).  x: (B, N, E); wq, wo: (E, E); wk, wv: (E, E), or (E, Hkv * d) for
    grouped-query heads (Hkv divides n_head, d = E // n_head; query head h reads kv head h // (n_head // Hkv)).  With ``fused_layout``
    the kernels read the Hkv heads of k and v in place, forward and backward (device_ops.flash_attn_gqa: no expanded copy, and the
    group's dK / dV are added by the library's ordered group sum); ``fused_layout=False`` expands k and v to n_head heads in front of
    the operator and reproduces the reference's four permute + contiguous copies (for comparison); both give the same values.
    Bias-free, as the reference's ``Linear(..., bias=False)`` projections (:40-52).
    ``fold_scale`` (with ``fused_layout``): log2(e)/sqrt(d) is folded into the query projection's weights and the operator is called
    with softmax_scale = ln 2 -- the same function of x, but the bf16 MFMA-slot kernels' folded scale is then exactly 1: no extra
    operand rounding whatever the magnitude of the activations (DESIGN.md section 3 "Scaling").
    ``rope`` (a Rotary): q and k are rotated by position (token i at position i) between the projection and the operator
    (device_ops.apply_rotary, whose backward is the inverse rotation: the path is trainable).
    ``window`` = W, ``sink`` = S: the sliding-window mask a KVCache(window=W, sink=S) generates under (token i sees the last W
    positions and the first S), forward and backward (device_ops.flash_attn_gqa(window=, sink=)); the rotation comes first, as
    without a window.  None or 0, W >= N or S >= N: the layer without them.
    ``softcap`` = C (causal only): the logit cap a KVCache(softcap=C) generates under, C * tanh(score / C) on the scaled score before
    the mask, forward and backward (device_ops.flash_attn_gqa(softcap=)); it composes with ``rope``, ``window``, ``sink`` and
    ``fold_scale`` (the cap acts on softmax_scale * q.k, which folding leaves the same).  None or 0: the layer without a cap.
    ``sink_logits`` (causal only; float32 (n_head,), which may require grad): the learned sink logits a KVCache(sink_logits=) generates
    under, one column more in every softmax of a head (device_ops.flash_attn_gqa(sink_logits=)); composes with ``rope``, ``window``
    and ``fold_scale`` (the logit is in logit units: no scale touches it); not beside ``sink`` or ``softcap``."""
    B, N, E = x.shape
    capped = device_ops._check_softcap(softcap) is not None
    # (a cap, and learned sink logits: kernels of the window family, whatever the window)
    windowed = capped or sink_logits is not None or device_ops._training_window(window, sink, causal, N) is not None
    if fused_layout:
        q, k, v = _project(x, wq * (LOG2E / (E // n_head) ** 0.5) if fold_scale else wq, wk, wv, n_head)
        if rope is not None:
            q, k = rope.apply(q), rope.apply(k)
        if windowed:   # grouped or not: k and v stay (B, N, Hkv, d)
            o = device_ops.flash_attn_gqa(q, k, v, causal, LN2 if fold_scale else None, "bnhd", window, sink, softcap, sink_logits)
        elif k.shape[2] == n_head:
            o = _attention(q, k, v, causal, _lib.FA_LAYOUT_BNHD, LN2 if fold_scale else None)   # (B, N, H, d) fp32: already merged
        else:   # grouped-query heads: k and v stay (B, N, Hkv, d)
            o = device_ops.flash_attn_gqa(q, k, v, causal, LN2 if fold_scale else None, "bnhd")
        merged = o.reshape(B * N, E)
    else:
        q, k, v = _project(x, wq, wk, wv, n_head)
        if rope is not None:
            q, k = rope.apply(q), rope.apply(k)
        q, k, v = (t.permute(0, 2, 1, 3).contiguous() for t in (q, _expand_kv(k, n_head), _expand_kv(v, n_head)))
        if windowed:
            o = device_ops.flash_attn_gqa(q, k, v, causal, None, "bhnd", window, sink, softcap, sink_logits)
        else:
            o = _attention(q, k, v, causal, _lib.FA_LAYOUT_BHND)                              # (B, H, N, d)
        merged = o.permute(0, 2, 1, 3).contiguous().view(B * N, E)
    return (merged.to(x.dtype) @ wo).view(B, N, E)


def attention_stack(x, layers, n_head: int, causal: bool = True, fused_layout: bool = True, fold_scale: bool = False, rope=None,
                    window=None, sink=None, softcap=None, sink_logits=None):
    """x <- x + MultiHeadAttention_l(x) for every (wq, wk, wv, wo) in ``layers``: the attention data flow of the reference's
    4-layer causal DecoderLM (modules_transfomer.py:255-351) without its out-of-scope LayerNorm / FFN blocks.  ``rope``: every
    layer rotates its q and k (multi_head_attention).  ``window``, ``sink``: every layer attends under the sliding-window mask of a
    KVCache(window=, sink=), so a model that generates through such a cache trains under the mask it runs with.  ``softcap``: every
    layer soft-caps its logits as a KVCache(softcap=) does (multi_head_attention), likewise.  ``sink_logits``: float32
    (n_layers, n_head), layer l attends with row l as its learned sink logits, as a KVCache(sink_logits=) does."""
    if sink_logits is not None and (not isinstance(sink_logits, torch.Tensor) or sink_logits.dim() != 2 or sink_logits.shape[0] != len(layers)):
        raise ValueError("sink_logits must be a float32 (n_layers, n_head) tensor: one row of learned logits per layer")
    for li, (wq, wk, wv, wo) in enumerate(layers):
        x = x + multi_head_attention(x, wq, wk, wv, wo, n_head, causal, fused_layout, fold_scale, rope, window, sink, softcap,
                                     None if sink_logits is None else sink_logits[li])
    return x


def multi_head_attention_packed(x, cu_seqlens, wq, wk, wv, wo, n_head: int, fold_scale: bool = False, rope=None, window=None,
                                sink=None):
    """multi_head_attention over a PACKED batch of sequences of different lengths: x (T, E), sequence b owns the rows
    cu_seqlens[b] .. cu_seqlens[b + 1] - 1 (contiguous int32 (nseq + 1,) on x's device, handed to the kernels and never read on the
    host), and every token attends causally within its own sequence (device_ops.flash_attn_varlen: no padding, no key mask).
    Weights, grouped-query heads, ``fold_scale``, ``window`` and ``sink`` as multi_head_attention (the fused layout; causal only).
    ``rope`` (a Rotary): positions restart at every sequence (device_ops.apply_rotary_varlen).  Rows no sequence owns give zero
    attention output, hence zero rows of the result."""
    T, E = x.shape
    q, k, v = _project(x[None], wq * (LOG2E / (E // n_head) ** 0.5) if fold_scale else wq, wk, wv, n_head)
    q, k, v = q[0], k[0], v[0]   # (T, heads, d)
    if rope is not None:
        q, k = (device_ops.apply_rotary_varlen(t, rope.cos, rope.sin, cu_seqlens, rope.interleaved) for t in (q, k))
    o = device_ops.flash_attn_varlen(q, k, v, cu_seqlens, True, LN2 if fold_scale else None, window, sink)
    return o.reshape(T, E).to(x.dtype) @ wo


def attention_stack_packed(x, cu_seqlens, layers, n_head: int, fold_scale: bool = False, rope=None, window=None, sink=None):
    """attention_stack over a packed batch: x <- x + multi_head_attention_packed_l(x) for every (wq, wk, wv, wo) in ``layers``.  Per
    sequence it is attention_stack on that sequence alone; ``cu_seqlens`` goes to every layer's kernels as it is."""
    for (wq, wk, wv, wo) in layers:
        x = x + multi_head_attention_packed(x, cu_seqlens, wq, wk, wv, wo, n_head, fold_scale, rope, window, sink)
    return x


def prefix_gather_index(cu_seqlens, cu_seqlens_prefix, T: int, Tp: int):
    """int64 (Tp + T,): for every row of the packed keys under cu_seqlens_k = cu_seqlens + cu_seqlens_prefix, its source row in
    cat(prefix rows, token rows): sequence b's keys are its prefix rows followed by its own tokens.  Built on the arrays' device
    from the arrays alone (searchsorted; nothing is read on the host).  A row no sequence owns under cu_seqlens_k takes some row
    inside the buffer: the kernels neither read it nor give it a gradient."""
    cu, cup = cu_seqlens.long(), cu_seqlens_prefix.long()
    cuk = cu + cup
    t = torch.arange(Tp + T, device=cu.device)
    b = (torch.searchsorted(cuk[1:].contiguous(), t, right=True)).clamp_(max=cu.shape[0] - 2)   # cuk[b] <= t < cuk[b + 1]
    j = t - cuk[b]
    n_prefix = cup[b + 1] - cup[b]
    src = torch.where(j < n_prefix, cup[b] + j, Tp + cu[b] + j - n_prefix)
    return src.clamp_(0, Tp + T - 1)


def multi_head_attention_packed_prefix(x, cu_seqlens, prefix_k, prefix_v, cu_seqlens_prefix, wq, wk, wv, wo, n_head: int):
    """multi_head_attention_packed behind a PREFIX of keys and values that are given, not projected: x (T, E) as there, prefix_k and
    prefix_v (Tp, Hkv, d) with sequence b owning the rows cu_seqlens_prefix[b] .. cu_seqlens_prefix[b + 1] - 1 (prefix tuning, where
    they are the trained parameters; a cached prompt; the earlier chunks of a long sequence).  Every token attends its sequence's
    prefix rows and, causally, its sequence's own tokens: the keys of a sequence are its prefix rows followed by its tokens' keys
    (prefix_gather_index, differentiable through torch's indexing: prefix_k.grad and prefix_v.grad flow), cu_seqlens_k =
    cu_seqlens + cu_seqlens_prefix, and device_ops.flash_attn_varlen_prefix does the rest.  Neither array is read on the host.
    No ``rope``: apply_rotary_varlen restarts positions at every sequence and has no offset for the tokens behind a prefix."""
    T, E = x.shape
    q, k, v = _project(x[None], wq, wk, wv, n_head)
    q, k, v = q[0], k[0], v[0]   # (T, heads, d)
    if prefix_k.shape != prefix_v.shape or prefix_k.dim() != 3 or prefix_k.shape[1:] != k.shape[1:]:
        raise ValueError(f"prefix_k and prefix_v must both be (Tp, Hkv, d) = (Tp, {k.shape[1]}, {k.shape[2]}), the projected keys' heads")
    if cu_seqlens_prefix.shape != cu_seqlens.shape:
        raise ValueError("cu_seqlens and cu_seqlens_prefix must have one length: the same sequences, counted in tokens and in prefix rows")
    src = prefix_gather_index(cu_seqlens, cu_seqlens_prefix, T, prefix_k.shape[0])
    k_all, v_all = (torch.cat((p.to(t.dtype), t))[src] for p, t in ((prefix_k, k), (prefix_v, v)))
    o = device_ops.flash_attn_varlen_prefix(q, k_all, v_all, cu_seqlens, cu_seqlens + cu_seqlens_prefix)
    return o.reshape(T, E).to(x.dtype) @ wo


def attention_stack_packed_prefix(x, cu_seqlens, prefixes, cu_seqlens_prefix, layers, n_head: int):
    """attention_stack_packed behind per-layer prefixes: x <- x + multi_head_attention_packed_prefix_l(x) for every (wq, wk, wv, wo)
    in ``layers`` with its (prefix_k, prefix_v) of ``prefixes``; one cu_seqlens_prefix for all layers."""
    if len(prefixes) != len(layers):
        raise ValueError(f"one (prefix_k, prefix_v) per layer: {len(prefixes)} prefixes for {len(layers)} layers")
    for (prefix_k, prefix_v), (wq, wk, wv, wo) in zip(prefixes, layers):
        x = x + multi_head_attention_packed_prefix(x, cu_seqlens, prefix_k, prefix_v, cu_seqlens_prefix, wq, wk, wv, wo, n_head)
    return x


def multi_head_attention_packed_bidir(x, cu_seqlens, wq, wk, wv, wo, n_head: int, rope=None, window=None):
    """Encoder self-attention over a packed batch: multi_head_attention_packed's data flow and weights, but every token attends to
    EVERY token of its own sequence (device_ops.flash_attn_varlen_bidir with one array for queries and keys: no padding, no key
    mask).  ``rope`` (a Rotary): positions restart at every sequence.  Rows no sequence owns give zero rows of the result.
    ``window`` = (left, right): local attention, every token attends the ``left`` tokens before and the ``right`` tokens behind it
    in its own sequence (device_ops.flash_attn_varlen_local; -1 or None: unbounded on that side); None: no window, the call above."""
    T, E = x.shape
    q, k, v = _project(x[None], wq, wk, wv, n_head)
    q, k, v = q[0], k[0], v[0]   # (T, heads, d)
    if rope is not None:
        q, k = (device_ops.apply_rotary_varlen(t, rope.cos, rope.sin, cu_seqlens, rope.interleaved) for t in (q, k))
    if window is None:
        o = device_ops.flash_attn_varlen_bidir(q, k, v, cu_seqlens)
    else:
        o = device_ops.flash_attn_varlen_local(q, k, v, cu_seqlens, window=window)
    return o.reshape(T, E).to(x.dtype) @ wo


def _layer_windows(window, n_layers):
    """``window`` of a stack as one entry per layer: None (no layer has one), one pair (every layer has it), or a sequence of
    ``n_layers`` entries, each a pair or None."""
    if window is None:
        return [None] * n_layers
    window = list(window)
    if len(window) == 2 and all(w is None or isinstance(w, int) for w in window):   # one (left, right)
        return [tuple(window)] * n_layers
    if len(window) != n_layers:
        raise ValueError(f"window must be None, one (left, right) pair or one entry per layer: {len(window)} entries for {n_layers} layers")
    return window


def encoder_stack_packed(x, cu_seqlens, layers, n_head: int, rope=None, window=None):
    """The encoder layer stack over a packed batch: x <- x + multi_head_attention_packed_bidir_l(x) for every (wq, wk, wv, wo) in
    ``layers``.  Per sequence it is attention_stack(causal=False) on that sequence alone.  ``window``: None, one (left, right) pair
    for every layer, or a sequence with one entry per layer, each a pair or None (global and local layers in alternation)."""
    layers = list(layers)
    for (wq, wk, wv, wo), w in zip(layers, _layer_windows(window, len(layers))):
        x = x + multi_head_attention_packed_bidir(x, cu_seqlens, wq, wk, wv, wo, n_head, rope, w)
    return x


def cross_attention_packed(x, cu_seqlens_q, memory, cu_seqlens_k, wq, wk, wv, wo, n_head: int):
    """Cross-attention over packed batches: the queries come from x (Tq, E) through wq (E, E), the keys and values from memory
    (Tk, E_mem) through wk, wv (E_mem, E), or (E_mem, Hkv * d) for grouped-query heads (d = E // n_head), read grouped.  The tokens
    of sequence b (``cu_seqlens_q``) attend all of sequence b's memory rows (``cu_seqlens_k``); a sequence without memory gives zero
    attention output.  Returns (Tq, E)."""
    Tq, E = x.shape
    d = E // n_head
    if wk.shape != wv.shape or wk.shape[1] % d or n_head % max(wk.shape[1] // d, 1):
        raise ValueError(f"wk and wv must both be (E_mem, Hkv * {d}) with Hkv a divisor of n_head = {n_head}")
    q = (x @ wq).view(Tq, n_head, d)
    k, v = ((memory @ w).view(memory.shape[0], w.shape[1] // d, d) for w in (wk, wv))
    o = device_ops.flash_attn_varlen_bidir(q, k, v, cu_seqlens_q, cu_seqlens_k)
    return o.reshape(Tq, E).to(x.dtype) @ wo


# ---- incremental generation: the inference half of the chain above ----------------------------------------------------------------
# The reference's generate() (project/run_machine_translation.py:276-292) re-runs the whole model over the full prefix for every new
# token and keeps the last row.  With a KV cache, the prompt runs once through the fused causal forward (attention_stack_prefill), and
# every further step projects only its new tokens, appends their k and v at each batch element's own length and attends to the cache
# with the decode kernels (attention_stack_step): one pass over the cached K and V per layer instead of causal attention over N tokens.
# More than 128 new tokens at once (a second turn, a long message after a cached prefix, a prompt fed in pieces) go through the
# extend kernels (attention_stack_extend, attention_stack_prefill_chunked).
# The step, fused step, extend and ragged functions (and through them chunked prefill and GraphedStep) are ONE loop, _advance, and
# every attend call in it takes the cache's features from ONE place, cache.keywords(li):
# window=W makes every call a sliding-window one (each token sees the last W positions), and a PagedKVCache gives the pages behind
# the window back through release_behind_window; with sink=S every token also keeps the first S positions (attention sinks), whose
# pages are never released.  kv_dtype=torch.float8_e4m3fn: the cache holds e4m3 bytes with one scale per (layer, kv head), the calls
# quantise on the append, and a prompt fills the cache through extend_append while its own attention stays the square forward on the
# unquantised k, v.  rope=Rotary(...): one fa_mi355x_rope_append launch per layer rotates q and the new k on their way in, then the
# attend-only call runs; the square prefill and the unfused step rotate q and k with apply_rotary.  The cache holds ROTATED keys.
# softcap=C: every call soft-caps its logits, C * tanh(score / C) (Gemma-2, Grok-1), through the family's softcap entry point; the
# prompt takes the extend route, as on a windowed cache (attention_stack(softcap=) trains under the same function).
# sink_logits=(n_layers, H) fp32: every call of layer li adds that layer's learned sink logits to its softmax (gpt-oss), through the
# family's _lsink entry point; the prompt takes the extend route likewise.

MAX_STEP_TOKENS = 128   # fa_mi355x_fwd_decode's largest Nq; longer inputs are prefill, or attention_stack_extend after a prefix


def _check_cache_window(window):
    if window is not None and (isinstance(window, bool) or not isinstance(window, int) or window < 1):
        raise ValueError("window must be None or a positive int: the positions a token sees, its own included")
    return window


def _check_cache_sink(sink, window):
    if sink is not None and (isinstance(sink, bool) or not isinstance(sink, int) or sink < 0):
        raise ValueError("sink must be None or an int >= 0: the first positions every token keeps beside its window")
    if sink and window is None:
        raise ValueError("sink tokens stand beside a sliding window: sink= needs window=")
    return sink or None


def _check_cache_rope(rope, rows, head_dim):
    """``rope`` of a cache that can hold ``rows`` rows per sequence: every row needs an angle."""
    if rope is None:
        return None
    if not isinstance(rope, Rotary):
        raise TypeError("rope must be None or a Rotary")
    if rope.max_pos < rows:
        raise ValueError(f"the rotary tables hold max_pos = {rope.max_pos} positions, the cache {rows} rows: max_pos must cover the capacity")
    if rope.rot > head_dim:
        raise ValueError(f"the rotary dimension {rope.rot} exceeds the head dim {head_dim}")
    return rope


def _check_cache_quant(kv_dtype, kv_scale, dtype, window, n_layers, n_kv_head, device):
    """(the caches' dtype, the (k, v) scales or None) of a cache built with ``kv_dtype`` / ``kv_scale``."""
    if kv_dtype is None or kv_dtype == dtype:
        if kv_scale is not None:
            raise ValueError("kv_scale belongs to an fp8 cache: give kv_dtype=torch.float8_e4m3fn")
        return dtype, None
    if kv_dtype != device_ops._FP8:
        raise ValueError("kv_dtype must be None, the compute dtype or torch.float8_e4m3fn")
    if dtype != torch.bfloat16:
        raise TypeError("an fp8 cache takes a bfloat16 stack")
    if window is not None:
        raise ValueError("a sliding window on an fp8 cache is not built")
    if kv_scale is not None:
        if len(kv_scale) != 2:
            raise ValueError("kv_scale must be a pair (k_scale, v_scale) of float32 (n_layers, n_kv_head) tensors")
        for t in kv_scale:
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (n_layers, n_kv_head):
                raise ValueError("kv_scale must be a pair (k_scale, v_scale) of float32 (n_layers, n_kv_head) tensors")
        kv_scale = tuple(t.to(device).contiguous() for t in kv_scale)
    return kv_dtype, kv_scale


def _check_cache_softcap(softcap, sink, fp8):
    """``softcap`` of a cache: None, or a finite number above 0; not beside sink tokens, not on an fp8 cache (neither is built)."""
    if softcap is None:
        return None
    if isinstance(softcap, (bool, str)) or not isinstance(softcap, numbers.Real) or not math.isfinite(softcap) or softcap <= 0:
        raise ValueError("softcap must be None or a finite number above 0: the logit cap, softcap * tanh(score / softcap)")
    if sink is not None:
        raise ValueError("softcap beside sink tokens is not built: softcap= with sink=")
    if fp8:
        raise ValueError("softcap on an fp8 cache is not built: softcap= with kv_dtype=torch.float8_e4m3fn")
    return float(softcap)


def _check_cache_sink_logits(sink_logits, sink, softcap, fp8, n_layers, n_head, device):
    """``sink_logits`` of a cache: None, or a float32 (n_layers, n_head) tensor, one learned logit per layer and QUERY head; not
    beside sink tokens, a cap or an fp8 cache (none is built).  Kept as the caller's tensor where it already lives on the cache's
    device, contiguous: a parameter updated in place is what the next call reads."""
    if sink_logits is None:
        return None
    if not isinstance(sink_logits, torch.Tensor) or sink_logits.dtype != torch.float32 or tuple(sink_logits.shape) != (n_layers, n_head):
        raise ValueError(f"sink_logits must be None or a float32 (n_layers, n_head) = ({n_layers}, {n_head}) tensor: one learned logit "
                         "per layer and query head")
    if sink is not None:
        raise ValueError("sink_logits beside sink tokens is not built: sink_logits= with sink=")
    if softcap is not None:
        raise ValueError("sink_logits beside a logit cap is not built: sink_logits= with softcap=")
    if fp8:
        raise ValueError("sink_logits on an fp8 cache is not built: sink_logits= with kv_dtype=torch.float8_e4m3fn")
    return sink_logits.detach().to(device).contiguous()


class KVCache:
    """Per-layer k and v caches of a causal attention stack: ``k[l]``, ``v[l]`` are (B, capacity, n_kv_head, dp) in the projection's
    own [B][N][H][d] layout (no permute), dp = head_dim rounded up to 32, 64 or 128 with zero columns past head_dim.  ``n_kv_head``
    (default n_head) is the number of key/value heads of a grouped-query stack: it must divide n_head, and the cache holds only those.
    ``lengths``: device int32 (B,), the valid rows per batch element (read by the decode kernels, never by the host).
    ``window`` (None, or an int >= 1): the stack's layers use SLIDING-WINDOW attention, every token sees the last ``window``
    positions, its own included (Mistral's ``sliding_window``); the stack functions pass it to every device_ops call on this cache.
    The cache still holds every row (no ring buffer): a PagedKVCache gives the memory back through release_behind_window.
    ``sink`` (None, or an int >= 0; needs ``window``): ATTENTION-SINK tokens, the first ``sink`` positions of every sequence stay
    visible to every later token beside its window (a mask on the cache's logical rows: positions are not re-assigned; learned
    sink LOGITS are ``sink_logits`` below, another thing).
    ``kv_dtype`` (None: ``dtype``, or torch.float8_e4m3fn): an FP8 cache holds e4m3 bytes, half the memory and half the bytes a step
    reads, and ``kv_scale`` (None: ones, or a pair (k_scale, v_scale) of float32 (n_layers, n_kv_head) tensors) gives every layer's
    per-head scales: a cached element is scale * e4m3.  The stack must be bfloat16; the fused step, extend and chunked-prefill
    functions and GraphedStep quantise on the append; attention_stack_step (torch indexing), attention_stack_ragged, a window
    and sink tokens are not built for it.
    ``rope`` (None, or a Rotary whose tables cover the capacity): the stack encodes positions with ROTARY embeddings; the stack
    functions rotate every q and every new k by its position (the row it is appended to), and the cache holds rotated keys.
    ``softcap`` (None, or a finite number above 0): the stack's layers SOFT-CAP their attention logits, every score becomes
    softcap * tanh(score / softcap) before the softmax (Gemma-2's ``attn_logit_softcapping``, Grok-1); the stack functions pass it
    to every device_ops call on this cache, and a prompt goes through the extend kernels (the square forward has no cap).  Works
    with a window, a paged cache and rotary embeddings; not built beside sink tokens or on an fp8 cache, and a cache has ONE window
    (Gemma-2's alternating local and global layers are not covered).  The training forward and backward have no cap.
    ``sink_logits`` (None, or a float32 (n_layers, n_head) tensor): LEARNED ATTENTION-SINK LOGITS (gpt-oss), one per layer and query
    head; layer li's row joins every softmax of that layer as a column without a value vector (device_ops.flash_attn_decode's
    ``sink_logits``).  The stack functions pass the row to every device_ops call on this cache, the kernels read it on the device
    (a GraphedStep replays with the values it holds then), and a prompt goes through the extend kernels (the square forward has no
    logit).  Works with a window, a paged cache and rotary embeddings; not built beside sink tokens, a cap or on an fp8 cache.
    The constructor, which is PagedKVCache's too, checks in this order and reports the first fault: ``window``, ``sink``,
    ``n_kv_head``, what the memory layout adds (_pool: nothing here; ``page_size``, ``capacity``, ``n_pages`` of a PagedKVCache),
    ``rope``, then ``kv_dtype`` / ``kv_scale``, then ``softcap``, then ``sink_logits``."""

    block_table = None   # (a PagedKVCache has one)

    def __init__(self, n_layers, B, capacity, n_head, head_dim, dtype, device, n_kv_head=None, window=None, kv_dtype=None, kv_scale=None,
                 sink=None, rope=None, softcap=None, sink_logits=None):
        self.window = _check_cache_window(window)
        self.sink = _check_cache_sink(sink, self.window)
        self.head_dim, self.dp = head_dim, device_ops.padded_head_dim(head_dim)
        self.capacity, self.n_head = capacity, n_head
        self.n_kv_head = n_head if n_kv_head is None else n_kv_head
        if self.n_kv_head <= 0 or n_head % self.n_kv_head:
            raise ValueError(f"n_kv_head = {n_kv_head} must divide n_head = {n_head}")
        shape, rows = self._pool(B)
        self.rope = _check_cache_rope(rope, rows, head_dim)
        dtype, self.kv_scale = _check_cache_quant(kv_dtype, kv_scale, dtype, self.window, n_layers, self.n_kv_head, device)
        self.softcap = _check_cache_softcap(softcap, self.sink, dtype == device_ops._FP8)
        self.sink_logits = _check_cache_sink_logits(sink_logits, self.sink, self.softcap, dtype == device_ops._FP8, n_layers, n_head, device)
        self.k = [torch.zeros(shape, dtype=dtype, device=device) for _ in range(n_layers)]
        self.v = [torch.zeros(shape, dtype=dtype, device=device) for _ in range(n_layers)]
        self.lengths = torch.zeros(B, dtype=torch.int32, device=device)
        self.length_bound = 0   # host-side upper bound of every length: capacity checks without a device synchronisation
        self._workspaces = {}

    def _pool(self, B):
        """(the shape of every layer's k and v, the rows a sequence can reach: the positions the rope tables must cover)."""
        return (B, self.capacity, self.n_kv_head, self.dp), self.capacity

    def keywords(self, li, rotary=True, **new):
        """Every keyword an attend call on layer ``li`` of this cache takes beside its tensors: paging, windowing, quant, rotary,
        capping and learned sink logits, and the caller's own (``new``: k_new=, v_new=).  A new cache feature adds its provider here, and every stack function
        passes it.  ``rotary=False``: the caller has rotated q and k itself (the unfused step)."""
        return {**new, **self.paging(), **self.windowing(), **self.quant(li), **(self.rotary() if rotary else {}), **self.capping(),
                **self.learned_sinks(li)}

    def learned_sinks(self, li):
        """The keyword that gives a device_ops call on layer ``li`` its learned sink logits (row li, a view: the kernels read the
        cache's own tensor): none for a cache without them."""
        return {} if self.sink_logits is None else dict(sink_logits=self.sink_logits[li])

    def capping(self):
        """The keyword that makes a device_ops call a soft-capped one: none for a cache without a cap."""
        return {} if self.softcap is None else dict(softcap=self.softcap)

    def rotary(self):
        """The keywords that make a device_ops call a roped one: none for a cache without rotary embeddings."""
        return {} if self.rope is None else self.rope.keywords()

    def paging(self):
        """The keyword that makes a device_ops call a paged one: none for this cache, block_table= for a PagedKVCache."""
        return {} if self.block_table is None else dict(block_table=self.block_table)

    def windowing(self):
        """The keywords that make a device_ops call a windowed one: none for a cache without a window (the unwindowed entry points),
        window= for a windowed one, and sink= beside it for one that keeps sink tokens."""
        if self.window is None:
            return {}
        return dict(window=self.window) if self.sink is None else dict(window=self.window, sink=self.sink)

    @property
    def fp8(self):
        return device_ops._is_fp8(self.k[0])

    def quant(self, li):
        """The keywords that give a device_ops call on layer ``li`` of an fp8 cache its scales: none for any other cache, and none
        for an fp8 cache whose scales are all ones."""
        if not self.fp8 or self.kv_scale is None:
            return {}
        return dict(k_scale=self.kv_scale[0][li], v_scale=self.kv_scale[1][li])

    def reserve(self, n_tokens, rows=None):
        """Make sure the sequences own memory for ``n_tokens`` rows: a slab cache owns its ``capacity`` rows from the start."""

    def restart(self):
        """Forget every sequence, for a new prompt: all lengths and their bound to 0 (the rows stay: the next append overwrites them)."""
        self.lengths.zero_()
        self.length_bound = 0

    def _workspace(self, family, q, *cu_seqlens_q):
        """The scratch of the ``family`` ("decode", "extend", "ragged") call with this q, sized once per key: every family splits by a
        policy of its own (and the ragged call's block map lives there), and a windowed call on its window and sink spans."""
        key = (() if family == "decode" else (family,)) + (self.window, self.sink) + tuple(q.shape)
        if key not in self._workspaces:
            size = getattr(device_ops, family + "_workspace")
            self._workspaces[key] = size(q, self.k[0], *cu_seqlens_q, "bnhd", **self.paging(), **self.windowing())
        return self._workspaces[key]

    def workspace(self, q):
        return self._workspace("decode", q)

    def extend_workspace(self, q):
        return self._workspace("extend", q)

    def ragged_workspace(self, q, cu_seqlens_q):
        return self._workspace("ragged", q, cu_seqlens_q)

    def _pad(self, t):
        return t if self.dp == self.head_dim else device_ops.pad_head_dim(t, self.dp)


class PagedKVCache(KVCache):
    """A KVCache whose memory is handed out by the page: ``k[l]``, ``v[l]`` are per-layer POOLS (n_pages, page_size, n_kv_head, dp) and
    one ``block_table`` (B, max_pages) int32 on the device, shared by the layers, names the pages of each sequence in order
    (max_pages = ceil(capacity / page_size); cache row j of sequence b is row j % page_size of page block_table[b, j // page_size]).
    ``page_size`` is a multiple of 128 rows.  ``n_pages`` defaults to B * max_pages (every sequence can reach ``capacity``) and may be
    smaller: sequences of different lengths then share what a slab cache would reserve B times over.  The host keeps a free list and
    each sequence's page list; ``lengths`` and ``length_bound`` are KVCache's.  The stack functions reserve what a call needs and pass
    ``block_table`` to the same device_ops calls; results are bit for bit those of a KVCache of capacity max_pages * page_size.
    ``window``: as in KVCache; release_behind_window then returns the pages that have fallen out of every future window to the pool,
    so a long-running sequence holds O(window) pages.  ``released[b]`` counts the leading table slots sequence b no longer owns
    (``pages[b]`` are the pages of the slots behind them).
    ``sink``: as in KVCache.  The ``sink_pages`` = ceil(sink / page_size) leading table slots hold the sink rows and are NEVER
    released.  The invariant: sequence b owns the slots 0 .. sink_pages - 1 (as many of them as it has grown into) and the slots from
    sink_pages + released[b] on; ``released[b]`` counts the released slots directly behind the sink slots, and ``pages[b]`` lists the
    owned pages in slot order, the sink pages first.  The slots in between keep stale or zero entries, which the kernels never
    read.  Without sinks sink_pages = 0 and this is the rule above."""

    def __init__(self, n_layers, B, capacity, n_head, head_dim, dtype, device, n_kv_head=None, page_size=128, n_pages=None, window=None,
                 kv_dtype=None, kv_scale=None, sink=None, rope=None, softcap=None, sink_logits=None):
        self.page_size, self.n_pages = page_size, n_pages   # (as given: _pool checks them at their place in KVCache's order)
        super().__init__(n_layers, B, capacity, n_head, head_dim, dtype, device, n_kv_head, window, kv_dtype, kv_scale, sink, rope, softcap,
                         sink_logits)
        self.block_table = torch.zeros((B, self.max_pages), dtype=torch.int32, device=device)   # (entries past a sequence's pages: never read)
        self.free = list(range(self.n_pages - 1, -1, -1))   # (handed out from the end: page 0 first)
        self.pages = [[] for _ in range(B)]                 # the pages of each sequence, in order
        self.released = [0] * B                             # table slots behind the sink slots given back by release_behind_window

    def _pool(self, B):
        if self.page_size <= 0 or self.page_size % _lib.FA_PAGE_ROWS:
            raise ValueError(f"page_size = {self.page_size} must be a positive multiple of {_lib.FA_PAGE_ROWS} rows")
        if self.capacity <= 0:
            raise ValueError("capacity must be positive")
        self.max_pages = -(-self.capacity // self.page_size)
        self.sink_pages = -(-(self.sink or 0) // self.page_size)   # leading table slots that release_behind_window keeps
        if self.n_pages is None:
            self.n_pages = B * self.max_pages
        if self.n_pages <= 0:
            raise ValueError("n_pages must be positive")
        # (the library holds the rope tables' max_pos against the table's rows, not the capacity)
        return (self.n_pages, self.page_size, self.n_kv_head, self.dp), self.max_pages * self.page_size

    def restart(self):
        """KVCache.restart; the sequences that gave leading pages back (release_behind_window) are released whole, so that each
        starts over owning row 0 again.  The others keep their pages."""
        super().restart()
        for b, gone in enumerate(self.released):
            if gone:
                self.release(b)

    def reserve(self, n_tokens, rows=None):
        """Make sure the sequences ``rows`` (default all) own pages for ``n_tokens`` cache rows each.  New pages come from the free list
        and only the table rows that changed are written to the device, in place (the table's address never changes: a captured
        graph keeps reading it).  Nothing is launched when every sequence already owns enough.  RuntimeError, naming the shortfall and
        with nothing handed out, when the pool runs out."""
        if n_tokens > self.max_pages * self.page_size:
            raise ValueError(f"{n_tokens} rows exceed the table's {self.max_pages} pages of {self.page_size}")
        need = -(-n_tokens // self.page_size)
        rows = range(len(self.pages)) if rows is None else list(rows)
        missing = sum(max(0, need - self.released[b] - len(self.pages[b])) for b in rows)
        if missing > len(self.free):
            raise RuntimeError(f"page pool exhausted: {missing} more pages needed for {n_tokens} rows per sequence, {len(self.free)} of "
                               f"{self.n_pages} free ({missing - len(self.free)} short)")
        for b in rows:
            own, gone = self.pages[b], self.released[b]   # (released slots stay unowned: the windowed kernels never read them)
            if gone + len(own) >= need:
                continue
            while gone + len(own) < need:
                own.append(self.free.pop())
            keep = self.sink_pages   # (gone > 0 only once the sequence owns every sink slot; the released slots sit behind them)
            row = own[:keep] + [0] * gone + own[keep:] + [0] * (self.max_pages - gone - len(own))
            self.block_table[b].copy_(torch.tensor(row, dtype=torch.int32))

    def release(self, b):
        """Sequence b is finished: its pages go back to the free list (the next reserve hands them out again) and its length to 0.
        Its table row keeps its stale entries, which a sequence of length 0 never reads.  ``length_bound`` stays the bound of the
        others."""
        self.free.extend(reversed(self.pages[b]))
        self.pages[b] = []
        self.released[b] = 0
        self.lengths[b] = 0

    def release_behind_window(self, lengths):
        """Give back the pages no present or future query of a windowed cache can see.  ``lengths``: a host sequence of B ints, the rows
        each sequence holds now (the caller's own bookkeeping: the cache keeps no lengths on the host, and none is read from the device
        here).  Every later query of sequence b sits at a position >= lengths[b] and admits keys above its position - window, so a
        page whose last row is <= lengths[b] - window is out of reach for good: it goes back to the free list (the next reserve may
        hand it to anyone) and its table slot is counted in ``released[b]``.  Nothing is written to the device: the windowed kernels
        start every key range at the window and never read those slots, whatever they hold.  A cache with sink tokens keeps its
        ``sink_pages`` leading slots, which every later query still reads, and releases from the slot behind them on.  Returns the
        number of pages freed."""
        if self.window is None:
            raise ValueError("release_behind_window needs a cache with a window: without one every row stays visible")
        lengths = [int(n) for n in lengths]
        if len(lengths) != len(self.pages):
            raise ValueError(f"lengths must hold one int per sequence ({len(self.pages)})")
        freed = 0
        for b, n in enumerate(lengths):
            # slot s holds rows s * page_size .. (s + 1) * page_size - 1: out of reach when (s + 1) * page_size - 1 <= n - window
            behind = max(0, n - self.window + 1) // self.page_size
            keep = self.sink_pages   # (the sink slots stay; the releasable slots are keep .. behind - 1)
            drop = min(behind - keep - self.released[b], len(self.pages[b]) - keep)
            if drop > 0:
                self.free.extend(reversed(self.pages[b][keep:keep + drop]))
                del self.pages[b][keep:keep + drop]
                self.released[b] += drop
                freed += drop
        return freed


def _project(x, wq, wk, wv, n_head):
    """q (B, N, n_head, d), k and v (B, N, Hkv, d) with d = E // n_head and Hkv read from wk's and wv's (E, Hkv * d) shape."""
    B, N, E = x.shape
    x2 = x.reshape(B * N, E)
    d = E // n_head
    if wk.shape != wv.shape or wk.shape[1] % d or n_head % max(wk.shape[1] // d, 1):
        raise ValueError(f"wk and wv must both be (E, Hkv * {d}) with Hkv a divisor of n_head = {n_head}")
    return tuple((x2 @ w).view(B, N, w.shape[1] // d, d) for w in (wq, wk, wv))


def _check_kv_heads(k, cache):
    """k (B, T, Hkv, d), or packed (T, Hkv, d): the head axis is the last but one."""
    if k.shape[-2] != cache.n_kv_head:
        raise ValueError(f"the layers project {k.shape[-2]} kv heads, the cache holds {cache.n_kv_head}")


def _check_room(cache, n_tokens):
    if cache.length_bound + n_tokens > cache.capacity:
        raise ValueError(f"cache capacity {cache.capacity} exceeded")


def attention_stack_prefill(x, layers, n_head: int, cache: KVCache):
    """attention_stack(x, layers, n_head, causal=True) over a prompt x (B, P, E) that also (re)fills ``cache`` with every layer's k and
    v of the P tokens (lengths = P).  A grouped-query stack (wk, wv of shape (E, Hkv * d)) stores its Hkv heads, and the prompt's own
    attention reads those cache-shaped k and v in place (device_ops.flash_attn_fwd_gqa: no expanded copy).  Returns the stack's
    output (B, P, E).  A WINDOWED cache does not use that square forward, which has no window: its prompt goes through the extend
    kernels as one piece (attention_stack_prefill_chunked with chunk = P), which append and attend through the window.  A cache with
    a SOFTCAP takes the same route: the square forward has no cap.  So does a cache with learned SINK LOGITS."""
    B, P, E = x.shape
    if P > cache.capacity:
        raise ValueError(f"prompt of {P} tokens exceeds the cache capacity {cache.capacity}")
    if cache.window is not None or cache.softcap is not None or cache.sink_logits is not None:
        return attention_stack_prefill_chunked(x, layers, n_head, cache, max(P, 1))
    d = E // n_head
    # an fp8 cache, slab or paged, and every paged one take the prompt through the library's append (it quantises, and it knows the
    # pages), at rows lengths[b] - P .. lengths[b] - 1 = 0 .. P - 1 of every sequence; a plain slab is filled by torch indexing
    library_append = cache.block_table is not None or cache.fp8
    cache.reserve(P)
    cache.lengths.fill_(P)
    cache.length_bound = P
    # (a grouped-query stack: the kernels read the Hkv heads in place)
    fwd = device_ops.flash_attn_fwd_bnhd if cache.n_kv_head == n_head else device_ops.flash_attn_fwd_gqa
    for li, (wq, wk, wv, wo) in enumerate(layers):
        q, k, v = _project(x, wq, wk, wv, n_head)
        _check_kv_heads(k, cache)
        if cache.rope is not None:   # (token i of the prompt sits at position i; the cache is filled with the rotated k)
            q, k = cache.rope.apply(q), cache.rope.apply(k)
        kp, vp = cache._pad(k), cache._pad(v)
        if library_append:   # (k is rotated already and an append has no window: paging and quant only; zero columns past head_dim)
            device_ops.extend_append(k, v, cache.k[li], cache.v[li], cache.lengths, "bnhd", **cache.paging(), **cache.quant(li))
        else:
            cache.k[li][:, :P] = kp
            cache.v[li][:, :P] = vp
        if cache.dp == d:   # (the prompt's own attention reads the unquantised k, v)
            o, _, _ = fwd(q, kp, vp, True, _lib.FA_VARIANT_FA2)
        else:   # zero columns add nothing to the scores; the scale keeps the caller's d
            o, _, _ = fwd(cache._pad(q), kp, vp, True, _lib.FA_VARIANT_FA2, softmax_scale=d ** -0.5)
            o = o[..., :d]
        x = x + (o.reshape(B * P, E).to(x.dtype) @ wo).view(B, P, E)
    return x


def _indexed_append(cache, x_new):
    """attention_stack_step's append, torch indexing into a slab: checks, and returns place(li, q, k, v) -> the q to attend with."""
    if cache.block_table is not None:
        raise ValueError("attention_stack_step appends with torch indexing into a slab: a PagedKVCache steps through "
                         "attention_stack_step_fused")
    if cache.fp8:
        raise ValueError("attention_stack_step appends with torch indexing, which does not quantise: an fp8 cache steps through "
                         "attention_stack_step_fused")
    (B, T, _), dev, hkv = x_new.shape, x_new.device, cache.n_kv_head
    # rows b * capacity + lengths[b] + t of the (B * capacity, Hkv, dp) view of a layer's cache: the new tokens' k and v
    rows = (cache.lengths.long() + torch.arange(B, device=dev) * cache.capacity)[:, None] + torch.arange(T, device=dev)
    rows = rows.reshape(B * T)

    def place(li, q, k, v):
        if cache.rope is not None:   # (token t of batch element b sits at position lengths[b] + t)
            q, k = cache.rope.apply(q, cache.lengths), cache.rope.apply(k, cache.lengths)
        for dst, t in ((cache.k[li], k), (cache.v[li], v)):
            dst.view(B * cache.capacity, hkv, cache.dp).index_copy_(0, rows, cache._pad(t).reshape(B * T, hkv, cache.dp))
        return q
    return place


# What tells the calls that advance a cache apart: the device_ops function that attends, the family whose workspace it takes, x_new
# packed (T, E) with per-sequence counts or batched (B, T, E), the bound on T, and the append of the one call that does its own.
_Family = collections.namedtuple("_Family", "attend workspace packed max_tokens append", defaults=(False, None, None))
_STEP = _Family(device_ops.flash_attn_decode, "decode", max_tokens=MAX_STEP_TOKENS, append=_indexed_append)
_STEP_FUSED = _Family(device_ops.flash_attn_decode, "decode", max_tokens=MAX_STEP_TOKENS)
_EXTEND = _Family(device_ops.flash_attn_extend, "extend")
_RAGGED = _Family(device_ops.flash_attn_ragged, "ragged", packed=True)


def _advance(family, x_new, layers, n_head: int, cache: KVCache, counts=None):
    """The one loop behind the step, the fused step, extend and ragged: make room for the new tokens (``counts[b]`` of sequence b in a
    packed x_new, T of every sequence otherwise), then per layer project, hand q and the new k, v to the family's attend call (it
    writes them at rows new_len[b] - n .. new_len[b] - 1, zero columns past head_dim, rotated on a roped cache, then attends) and add
    the out-projection to the residual.  Lengths grow on the device, their bound on the host.  Only the ragged family builds
    tensors on the host (counts, cu) and copies them over: GraphedStep captures the fused step, which must never."""
    packed, shape = family.packed, tuple(x_new.shape)
    T, E = shape[-2:]
    if family.max_tokens is not None and T > family.max_tokens:
        raise ValueError(f"a step takes at most {family.max_tokens} tokens; use attention_stack_prefill for longer inputs")
    grow = max(counts) if packed else T
    _check_room(cache, grow)
    place = family.append and family.append(cache, x_new)
    cache.reserve(cache.length_bound + grow, [b for b, c in enumerate(counts) if c > 0] if packed else None)
    if packed:
        cnt = torch.tensor(counts, dtype=torch.int32)
        cu = torch.cat([torch.zeros(1, dtype=torch.int32), torch.cumsum(cnt, 0, dtype=torch.int32)]).to(x_new.device)
        cu, new_len = (cu,), cache.lengths + cnt.to(x_new.device)   # (cu_seqlens_q: the ragged calls' one argument more)
    else:
        cu, new_len = (), cache.lengths + T
    x = x_new
    for li, (wq, wk, wv, wo) in enumerate(layers):
        q, k, v = _project(x[None] if packed else x, wq, wk, wv, n_head)
        if packed:
            q, k, v = q[0], k[0], v[0]   # (T, heads, d)
        _check_kv_heads(k, cache)
        if place:
            q, kw = place(li, q, k, v), cache.keywords(li, rotary=False)
        else:
            kw = cache.keywords(li, k_new=k, v_new=v)
        o, _ = family.attend(q, cache.k[li], cache.v[li], *cu, new_len, causal=True, layout="bnhd",
                             workspace=cache._workspace(family.workspace, q, *cu), **kw)
        x = x + (o.reshape(-1, E).to(x.dtype) @ wo).view(shape)
    cache.lengths.copy_(new_len)
    cache.length_bound += grow
    return x


def attention_stack_step(x_new, layers, n_head: int, cache: KVCache):
    """One generation step of the stack: x_new (B, T, E), T <= 128 new tokens that follow each batch element's cached prefix.  Every
    layer projects them, appends k and v at rows lengths[b] .. lengths[b] + T - 1 (device indexing: no host synchronisation), and
    attends causally to the cache with the decode kernels (a grouped-query stack appends its Hkv heads and its n_head query heads
    read them in place); lengths grow by T.  Returns the stack's output for the new tokens (B, T, E),
    the last T rows of attention_stack over the whole sequence."""
    return _advance(_STEP, x_new, layers, n_head, cache)


def attention_stack_step_fused(x_new, layers, n_head: int, cache: KVCache):
    """attention_stack_step with the append inside the library: every layer hands q, k and v to one fused call
    (flash_attn_decode(..., k_new=, v_new=)), which writes k and v into the cache and then attends.  No row indices, padded copies
    or index_copy_ on the caller's side; the same results and the same cache contents, bit for bit."""
    return _advance(_STEP_FUSED, x_new, layers, n_head, cache)


def attention_stack_extend(x_new, layers, n_head: int, cache: KVCache):
    """attention_stack_step_fused without its bound on T: x_new (B, T, E), any T >= 1 new tokens that follow each batch element's
    cached prefix (a second turn, a long message after a cached system prompt; from an empty cache, a prompt or its first piece).
    T <= 128 IS attention_stack_step_fused (the same bits).  Above that every layer projects the new tokens and hands q, k and v to
    one device_ops.flash_attn_extend(..., k_new=, v_new=) call, which appends k and v at rows lengths[b] .. lengths[b] + T - 1 and
    attends causally with the extend kernels (128 rows per workgroup sharing each staged tile of the cache).  Lengths grow by T on
    the device; the capacity check is the host's, through ``cache.length_bound``.  Returns the stack's output for the new tokens
    (B, T, E): the last T rows of attention_stack over the whole sequence."""
    if x_new.shape[1] <= MAX_STEP_TOKENS:
        return attention_stack_step_fused(x_new, layers, n_head, cache)
    return _advance(_EXTEND, x_new, layers, n_head, cache)


def attention_stack_ragged(x_new, counts, layers, n_head: int, cache: KVCache):
    """One step of a serving loop over a RAGGED batch: sequence b brings ``counts[b]`` new tokens (a host list of B non-negative ints:
    1 for a sequence that decodes, hundreds for one in the middle of a chunked prefill, 0 for one with nothing to do), PACKED
    sequence after sequence into x_new (T, E), sum(counts) <= T (the rows past the sum are the unused tail of a fixed-capacity buffer).
    Builds cu_seqlens_q and lengths + counts on the device and makes ONE fused device_ops.flash_attn_ragged(..., k_new=, v_new=) call
    per layer, which appends every sequence's k and v at rows lengths[b] .. lengths[b] + counts[b] - 1 and attends causally; then
    lengths grow by counts.  The capacity check is the host's: length_bound + max(counts) <= capacity, and length_bound grows by
    max(counts).  A PagedKVCache reserves pages up to that bound for the sequences with counts[b] > 0 -- more than a short sequence
    needs (page-exact reservation wants the per-sequence lengths on the host, which this layer does not keep).  Returns (T, E): for
    each sequence, attention_stack_extend's output on that sequence alone, to rounding; rows past sum(counts) are unspecified."""
    if x_new.dim() != 2:
        raise ValueError("x_new must be packed: (T, E)")
    if cache.fp8:
        raise ValueError("the ragged calls on an fp8 cache are not built: step an fp8 cache through attention_stack_step_fused / _extend")
    T, B = x_new.shape[0], cache.lengths.shape[0]
    counts = [int(c) for c in counts]
    if len(counts) != B or min(counts) < 0 or sum(counts) > T:
        raise ValueError(f"counts must be {B} non-negative ints with sum <= T = {T}")
    return _advance(_RAGGED, x_new, layers, n_head, cache, counts)


def attention_stack_prefill_chunked(x, layers, n_head: int, cache: KVCache, chunk: int):
    """attention_stack_prefill in pieces of ``chunk`` tokens: the lengths are reset, then every piece of x (B, P, E) goes through
    attention_stack_extend after the pieces before it, so the activations of a step are bounded by the piece, not the prompt.
    Returns the stack's output (B, P, E); the cache ends as attention_stack_prefill leaves it (lengths = P), to rounding."""
    if chunk < 1:
        raise ValueError("chunk must be positive")
    if x.shape[1] > cache.capacity:
        raise ValueError(f"prompt of {x.shape[1]} tokens exceeds the cache capacity {cache.capacity}")
    cache.restart()
    return torch.cat([attention_stack_extend(piece.contiguous(), layers, n_head, cache) for piece in x.split(chunk, 1)], dim=1)


class GraphedStep:
    """attention_stack_step_fused for T new tokens per call, captured once in a device graph and replayed per call: a step is a fixed launch
    sequence (projections, the library's append + decode, the output projection), and everything it reads that changes from step to
    step -- ``cache.lengths`` and the caches -- is updated by that sequence itself, so every replay advances the cache by T tokens.
    Owns a static (B, T, E) input and output; ``step`` returns the static output, which the next call overwrites.  The host-side
    capacity check and ``cache.length_bound`` stay outside the graph."""

    def __init__(self, layers, n_head: int, cache: KVCache, T: int = 1):
        if not 1 <= T <= MAX_STEP_TOKENS:
            raise ValueError(f"a step takes 1 .. {MAX_STEP_TOKENS} tokens")
        self.layers, self.n_head, self.cache, self.T = layers, n_head, cache, T
        self.graph = self.x = self.y = None

    def _capture(self, x_new):
        cache = self.cache
        self.x = torch.empty_like(x_new)
        # one eager step on a side stream first (workspaces and library handles exist before the capture); it runs on a throw-away
        # input and its effects are undone: lengths restored, and the rows it wrote are the rows the first replay writes again
        lengths, bound = cache.lengths.clone(), cache.length_bound
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self.x.zero_()
            attention_stack_step_fused(self.x, self.layers, self.n_head, cache)
            cache.lengths.copy_(lengths)
        torch.cuda.current_stream().wait_stream(side)
        cache.length_bound = bound   # (for the capture's own capacity check and reserve; step() sets the bound after the replay)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):   # (runs nothing on the device)
            self.y = attention_stack_step_fused(self.x, self.layers, self.n_head, cache)

    def step(self, x_new):
        B, T, E = x_new.shape
        if T != self.T:
            raise ValueError(f"this graph steps {self.T} tokens at a time, got {T}")
        cache, bound = self.cache, self.cache.length_bound
        _check_room(cache, T)
        # (a paged cache: the pages of this step, outside the graph; the table is edited in place, so the graph reads the new entries)
        cache.reserve(bound + T)
        if self.graph is None:
            self._capture(x_new)
        elif x_new.shape != self.x.shape or x_new.dtype != self.x.dtype:
            raise ValueError("x_new must keep the shape and dtype of the captured step")
        self.x.copy_(x_new)
        self.graph.replay()
        cache.length_bound = bound + T
        return self.y
