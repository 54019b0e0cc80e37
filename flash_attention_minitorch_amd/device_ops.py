"""Device-resident entry points: torch-ROCm tensors in, torch-ROCm tensors out, no host round trip.

This is SURVEY.md row f2 (replace the reference's per-call malloc / H2D / D2H,
``src/flash_attn_fw.cu:314-357``, with persistent device tensors) and what ``bench.py`` times.
torch is plumbing only: device memory, streams.  All arithmetic runs in the HIP kernels.

Tensors are (B, H, N, d) or (BH, N, d), contiguous, float32 or bfloat16; outputs (O, dQ, dK, dV) are
float32 (a bf16 store alone would exceed the 1e-3 max-abs bound).  Grouped-query heads (k and v with fewer
heads than q, read in place): flash_attn_fwd_gqa / flash_attn_bwd_gqa / flash_attn_gqa.

Every training entry point is one call of ``_fwd`` or ``_bwd``: the checks in one fixed order, the allocation of what the caller did not
supply, and exactly one C call.
"""
from __future__ import annotations

import ctypes
import math
import numbers
import operator

import torch

from . import _lib

_DTYPES = {torch.float32: _lib.FA_DTYPE_F32, torch.bfloat16: _lib.FA_DTYPE_BF16}
_BHND, _BNHD = _lib.FA_LAYOUT_BHND, _lib.FA_LAYOUT_BNHD
_FA1 = _lib.FA_VARIANT_FA1


def _ptr(t):   # (a plain int or None: ctypes converts either for a c_void_p parameter)
    return t.data_ptr() if t is not None else None


def _stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def _dtype_code(t):
    code = _DTYPES.get(t.dtype)
    if code is None:
        raise TypeError(f"unsupported dtype {t.dtype}: use float32 or bfloat16")
    return code


def _require_gpu(t, who):
    if not t.is_cuda:
        raise _lib.FlashAttnLibraryError(f"{who} needs GPU tensors; there is no CPU fallback")


# per-call kernel options of fa_mi355x_fwd_ex / _bwd_ex / *_guarded (include/flash_attn_mi355x.h); all give the same results
OPTS_PHASED = (4, 2, 2)          # the round-1 phased kernels instead of the MFMA-slot ones
# Where the softmax scale is applied (option 8; include/flash_attn_mi355x.h "Softmax scale and the scale guard").  The MFMA-slot
# kernels (bf16, d = 64 / 128) fold tau*log2(e) into one bf16 operand (one more 2^-9 relative rounding of q or k, worth 8-10 % of the
# step); every other kernel scales each score in fp32, as the reference does.  The default of this module is the GUARDED call: one
# device-side pass over q and k (scale_guard, no host synchronisation), then every kernel and its fp32-scaling twin are launched and
# the one on the wrong side of the budget returns at once.
OPTS_EXACT_SCALE = (0, 0, 0, 0, 0, 0, 0, 0, 2)    # fp32 scaling whatever the operands look like (no guard pass)
OPTS_FOLDED_SCALE = (0, 0, 0, 0, 0, 0, 0, 0, 1)   # the caller vouches for U(-1, 1)-sized operands: folded scale, no guard pass


def pick_opts(q, k, budget=1e-2):
    """The guard's decision on the HOST (two reductions and ONE synchronisation): OPTS_FOLDED_SCALE when one more 2^-9 rounding of q / k
    is estimated to move a score by less than ``budget`` (log2 units; 2^-9 / sqrt(3) * tau*log2(e) * max_row |q| * max_row |k|: U(-1, 1)
    gives about 6e-3 at d = 64 and 7e-3 at d = 128), else OPTS_EXACT_SCALE.  For callers that decide once per tensor family (at model
    set-up, or every few hundred steps) and then skip the per-call guard pass; the default calls need none of this."""
    if q.dtype != torch.bfloat16 or q.shape[-1] not in (64, 128):
        return None   # fp32 and d = 32 run kernels with fp32 scaling anyway
    d = q.shape[-1]
    qn = q.float().norm(dim=-1).amax()
    kn = k.float().norm(dim=-1).amax()
    est = float(qn * kn) * (1.4426950408889634 / d ** 0.5) * (2.0 ** -9) / 3.0 ** 0.5
    return OPTS_EXACT_SCALE if est > budget else OPTS_FOLDED_SCALE


def _scale_mode(opts):
    return int(opts[8]) if opts is not None and len(opts) > 8 else 0


def scale_guard(q, k, out=None):
    """The device-side evidence the folded-scale kernels run on (fa_mi355x_scale_guard): the largest squared row norms of q and k as
    partial maxima, fa_mi355x_guard_bytes() bytes.  One pass over both tensors, asynchronous, no host synchronisation.  The forward
    and the backward of one (q, k) pair take the same guard.  Any layout: a row is the last dimension."""
    if q.dtype != k.dtype or q.shape[-1] != k.shape[-1] or not q.is_cuda or not q.is_contiguous() or not k.is_contiguous():
        raise ValueError("q and k must be contiguous GPU tensors of one dtype and row length")
    if out is None:
        out = torch.empty(_lib.core().fa_mi355x_guard_bytes() // 4, dtype=torch.float32, device=q.device)
    else:
        _check_buffer(out, q.get_device(), "guard", _lib.guard_elems())
    d = q.shape[-1]
    if q.numel() != k.numel():
        raise ValueError("q and k must have the same number of rows")
    _lib.check(_lib.core().fa_mi355x_scale_guard(_ptr(q), _ptr(k), q.numel() // d, d, _dtype_code(q), _ptr(out), _stream_ptr()))
    return out


def _wants_guard(q, opts):
    """Could a folded-scale kernel run for these operands (bf16, d = 64 / 128, option 8 left at 0)?"""
    return q.dtype == torch.bfloat16 and q.shape[-1] in (64, 128) and _scale_mode(opts) == 0


def new_guard(q, opts=None):
    """An empty guard for a forward call to FILL (flash_attn_fwd(..., guard=g, produce_guard=True)) and the backward of the same
    (q, k) to read; None where no kernel of the call could fold the scale."""
    if not _wants_guard(q, opts):
        return None
    return torch.empty(_lib.core().fa_mi355x_guard_bytes() // 4, dtype=torch.float32, device=q.device)


_NATIVE_D = (32, 64, 128)


def padded_head_dim(d):
    """The row length {32, 64, 128} that a head dim d <= 128 runs at (zero columns d .. dp-1)."""
    if d > 128:
        raise ValueError("head dimension d > 128 is not supported (the reference kernels assert d <= 128, src/flash_attn_fw.cu:43)")
    return 32 if d <= 32 else (64 if d <= 64 else 128)


def pad_head_dim(t, dp):
    """(.., N, d) -> contiguous (.., N, dp) with zero columns d .. dp-1 (what fa_mi355x_*_padded and a padded KV cache expect)."""
    return torch.nn.functional.pad(t, (0, dp - t.shape[-1]))


def _unpad(tp, d, dst):
    """Columns 0 .. d-1 of a padded result: a new contiguous tensor, or copied into the caller's ``dst``."""
    if dst is None:
        return tp[..., :d].contiguous()
    dst.copy_(tp[..., :d])
    return dst


def _with_opt(opts, index, value):
    o = list(opts or ()) + [0] * (index + 1)
    o[index] = value
    return tuple(o[:max(index + 1, len(opts or ()))])


def _workspace_bytes(bh, n, d, opts=None):
    arr, cnt = _lib.opts_array(opts)
    return _lib.core().fa_mi355x_bwd_workspace_bytes_ex(bh, n, d, arr, cnt)


def _workspace(bh, n, d, device, opts=None):
    return torch.empty((_workspace_bytes(bh, n, d, opts) + 3) // 4, dtype=torch.float32, device=device)


def bwd_workspace(q, opts=None):
    """Scratch for the backward of (.., N, d) tensors, sized by the library (fa_mi355x_bwd_workspace_bytes_ex: the three
    row-constant vectors)."""
    n, d = q.shape[-2], q.shape[-1]
    return _workspace(q.numel() // (n * d), n, padded_head_dim(d), q.device, opts)


def bwd_status(workspace, q):
    """Status of a backward call that used ``workspace`` (fa_mi355x_bwd_status): 0, as no kernel of the library waits for another
    workgroup; kept for callers of the published ABI."""
    n, d = q.shape[-2], q.shape[-1]
    st = ctypes.c_int(0)
    _lib.check(_lib.core().fa_mi355x_bwd_status(_ptr(workspace), q.numel() // (n * d), n, d, ctypes.byref(st)))
    return st.value


STAGE_PREP, STAGE_DKDV, STAGE_DQ, STAGE_ALL = 1, 2, 4, 7
_F32 = torch.float32
_MASK_RANK = "a key mask needs (B, H, N, d) tensors: it is shared by the heads of a batch element"
_RANK4 = "expected (B, H, N, d)"


def _check_buffer(t, dev, name, numel):
    """A caller's float32 buffer that a kernel reads or writes as ``numel`` contiguous elements, on device index ``dev``."""
    if t.dtype is not _F32 or not t.is_contiguous() or t.get_device() != dev or t.numel() < numel:
        raise ValueError(f"{name} must be a contiguous float32 tensor on q's device with at least {numel} elements")


def _check_workspace(workspace, nbytes, dev, sizer):
    """A caller's workspace for a call that needs ``nbytes``; ``sizer``: the call that makes one, for the message."""
    if workspace.numel() * workspace.element_size() < nbytes:
        raise ValueError(f"workspace too small: size it with {sizer}")
    if not workspace.is_contiguous() or workspace.get_device() != dev or workspace.data_ptr() % 256:
        raise ValueError("workspace must be a contiguous, 256-byte aligned tensor on q's device")


def _check_out(out, q):
    """A caller's ``out`` (None: the call allocates it): fp32 in q's shape."""
    if out is not None and (out.dtype is not _F32 or out.shape != q.shape or not out.is_contiguous() or out.get_device() != q.get_device()):
        raise ValueError("out must be a contiguous float32 tensor of q's shape")


def _check_grads(grads, q, k, v):
    """A caller's ``grads`` (dq, dk, dv; None: the call allocates them): fp32 buffers for the shapes of q, k and v."""
    for g, like in zip(grads or (), (q, k, v)):
        _check_buffer(g, q.get_device(), "each of grads", like.numel())


def _new_f32(*like):
    """New fp32 tensors in the shapes of ``like``, on their device."""
    return tuple(torch.empty(t.shape, dtype=_F32, device=t.device) for t in like)


def _check_inputs(layout, ts, o, key_mask, rank4):
    """The checks every call starts with, in the order the entry points have always run them: the tensors (GPU, dtype, shared shape /
    dtype / device, contiguity, rank), the key mask, the forward's O.  ``rank4``: the message for a BHND call that needs 4-d tensors
    (key mask, dropout), else None; _MASK_RANK also requires the key mask.  Returns (B, H, N, d, dtype code) as the C entry point
    takes them: B*H and 1 for a call without mask or dropout."""
    q = ts[0]
    dev = q.get_device()
    if layout == _BNHD:
        if q.dim() != 4:
            raise ValueError("expected (B, N, H, d)")
        for t in ts:
            if not t.is_cuda or t.shape != q.shape or t.dtype != q.dtype or t.get_device() != dev or not t.is_contiguous():
                raise ValueError("q, k, v must be contiguous GPU tensors of one shape and dtype")
        B, N, H, d = q.shape
        dtype = _dtype_code(q)
    else:
        _require_gpu(q, "device_ops")
        dtype = _dtype_code(q)
        for t in ts:
            if t.shape != q.shape or t.dtype != q.dtype or t.get_device() != dev:
                raise ValueError("q, k, v (and out_grad) must share shape, dtype and device")
            if not t.is_contiguous():
                raise ValueError("tensors must be contiguous [.., N, d]")
        if q.dim() not in (3, 4):
            raise ValueError("expected (B, H, N, d) or (BH, N, d)")
        N, d = q.shape[-2], q.shape[-1]
        B, H = q.numel() // (N * d), 1
        if rank4 is not None:
            if q.dim() != 4:
                raise ValueError(rank4)
            B, H = q.shape[0], q.shape[1]
    if (key_mask is not None or rank4 is _MASK_RANK) and (key_mask is None or not key_mask.is_cuda or key_mask.dtype is not _F32
                                                          or tuple(key_mask.shape) != (B, N) or not key_mask.is_contiguous()):
        raise ValueError("key_mask must be a contiguous float32 GPU tensor of shape (B, N)")
    if o is not None and (o.dtype is not _F32 or o.shape != q.shape or not o.is_contiguous() or o.get_device() != dev):
        raise ValueError("out must be the forward's contiguous float32 output")
    return B, H, N, d, dtype


def _check_caller(dev, rows, l, m, guard):
    if l is not None:
        _check_buffer(l, dev, "l", rows)
    if m is not None:
        _check_buffer(m, dev, "m", rows)
    if isinstance(guard, torch.Tensor):
        _check_buffer(guard, dev, "guard", _lib.guard_elems())


def _dropout(rate, scale, seed):
    return float(rate), float(scale), int(seed) & 0xFFFFFFFF


def _fwd(layout, q, k, v, causal, variant, scale=None, opts=None, out_dtype=_F32, key_mask=None, dropout=None, guard="auto",
         produce=False, out=None, l=None, m=None, rank4=None):
    """Every forward: check the call, allocate what the caller did not supply, make one C call.  Returns (out, l, m)."""
    B, H, N, d, dtype = _check_inputs(layout, (q, k, v), None, key_mask, rank4)
    padded = layout == _BHND and rank4 is None and d not in _NATIVE_D
    if padded:
        if out_dtype is not _F32 or opts is not None:
            raise ValueError("per-call options and a bf16 output need a native head dim (32, 64, 128): other d run zero-padded through "
                             "fa_mi355x_fwd_padded, which takes neither")
        dp = padded_head_dim(d)
    else:
        if out_dtype is not _F32 and out_dtype is not torch.bfloat16:
            raise TypeError("out_dtype must be float32 or bfloat16")
        if out is not None and (out.dtype != out_dtype or out.shape != q.shape or not out.is_contiguous()
                                or out.get_device() != q.get_device()):
            raise ValueError("out must be a contiguous tensor of q's shape and of out_dtype")
    _check_caller(q.get_device(), B * H * N, l, m, guard)
    lib, dev, causal = _lib.core(), q.device, int(bool(causal))
    stats = (B, H, N) if layout == _BNHD else q.shape[:-2] + (N,)
    if l is None:
        l = torch.empty(stats, dtype=_F32, device=dev)
    if m is None and variant == _FA1:
        m = torch.empty(stats, dtype=_F32, device=dev)
    if padded:
        qp, kp, vp = (pad_head_dim(t, dp) for t in (q, k, v))
        outp = torch.empty(qp.shape, dtype=_F32, device=dev)
        _lib.check(lib.fa_mi355x_fwd_padded(_ptr(qp), _ptr(kp), _ptr(vp), _ptr(outp), _ptr(l), _ptr(m), B, N, d, dp, causal, variant,
                                            dtype, _stream_ptr()))
        return _unpad(outp, d, out), l, m
    if out is None:
        out = torch.empty(q.shape, dtype=out_dtype, device=dev)
    ptrs = (_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(l), _ptr(m))
    if dropout is not None:
        st = lib.fa_mi355x_fwd_dropout(*ptrs, _ptr(key_mask), *dropout, B, H, N, d, layout, causal, variant, dtype, _stream_ptr())
    elif key_mask is not None:
        st = lib.fa_mi355x_fwd_masked(*ptrs, _ptr(key_mask), B, H, N, d, layout, causal, variant, dtype, _stream_ptr())
    else:
        if out_dtype is torch.bfloat16:
            opts = _with_opt(opts, 9, 1)
        arr, cnt = _lib.opts_array(opts)
        if isinstance(guard, str):
            guard, produce = new_guard(q, opts), True
        st = lib.fa_mi355x_fwd_guarded(*ptrs, B, H, N, d, layout, float(scale or 0.0), causal, variant, dtype, arr, cnt, _ptr(guard),
                                       int(bool(produce and guard is not None)), _stream_ptr())
    _lib.check(st)
    return out, l, m


def _bwd(layout, q, k, v, o, do, l, m, causal, variant, scale=None, opts=None, key_mask=None, dropout=None, guard="auto",
         grads=None, workspace=None, stages=STAGE_ALL, rank4=None):
    """Every backward: check the call, allocate what the caller did not supply, make one C call.  Returns (dq, dk, dv)."""
    B, H, N, d, dtype = _check_inputs(layout, (q, k, v, do), o, key_mask, rank4)
    padded = layout == _BHND and rank4 is None and d not in _NATIVE_D
    if padded:
        if opts is not None or stages != STAGE_ALL or workspace is not None:
            raise ValueError("per-call options, a stage mask and a caller's workspace need a native head dim (32, 64, 128): other d run "
                             "zero-padded through fa_mi355x_bwd_padded, which takes none of them")
        dp = padded_head_dim(d)
    elif workspace is not None:
        if workspace.numel() * workspace.element_size() < _workspace_bytes(B * H, N, d, opts):
            raise ValueError("workspace too small for these options: size it with bwd_workspace(q, opts)")
        if not workspace.is_contiguous() or workspace.get_device() != q.get_device():
            raise ValueError("workspace must be a contiguous tensor on q's device")
    _check_caller(q.get_device(), B * H * N, l, m, guard)
    if grads is not None and not padded:
        for g in grads:
            _check_buffer(g, q.get_device(), "each of grads", q.numel())
    lib, dev, causal = _lib.core(), q.device, int(bool(causal))
    if padded:
        ins = [pad_head_dim(t, dp) for t in (q, k, v, o, do)]
        ws = _workspace(B, N, dp, dev)
        gp = [torch.empty(ins[0].shape, dtype=_F32, device=dev) for _ in range(3)]
        _lib.check(lib.fa_mi355x_bwd_padded(*map(_ptr, ins + gp), _ptr(l), _ptr(m), _ptr(ws), B, N, d, dp, causal, variant, dtype,
                                            _stream_ptr()))
        return tuple(_unpad(g, d, dst) for g, dst in zip(gp, grads or (None,) * 3))
    if workspace is None:   # (a BNHD call has always sized it without the options: the size does not depend on them)
        workspace = _workspace(B * H, N, d, dev, opts if layout == _BHND else None)
    dq, dk, dv = grads or (torch.empty(q.shape, dtype=_F32, device=dev) for _ in range(3))
    ptrs = (_ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(do), _ptr(dq), _ptr(dk), _ptr(dv), _ptr(l), _ptr(m))
    if dropout is not None:
        st = lib.fa_mi355x_bwd_dropout(*ptrs, _ptr(key_mask), *dropout, _ptr(workspace), B, H, N, d, layout, causal, variant, dtype,
                                       _stream_ptr())
    elif key_mask is not None:
        st = lib.fa_mi355x_bwd_masked(*ptrs, _ptr(key_mask), _ptr(workspace), B, H, N, d, layout, causal, variant, dtype, _stream_ptr())
    else:
        if isinstance(guard, str):   # "auto" on a call that only reads a guard: the separate pass over q and k
            guard = scale_guard(q, k) if _wants_guard(q, opts) else None
        arr, cnt = _lib.opts_array(opts)
        st = lib.fa_mi355x_bwd_guarded(*ptrs, _ptr(workspace), B, H, N, d, layout, float(scale or 0.0), causal, variant, dtype,
                                       int(stages), arr, cnt, _ptr(guard), _stream_ptr())
    _lib.check(st)
    return dq, dk, dv


def flash_attn_fwd(q, k, v, causal=False, variant=_lib.FA_VARIANT_FA2, out=None, l=None, m=None, opts=None, guard="auto",
                   out_dtype=torch.float32, produce_guard=False):
    """Forward.  Returns (out fp32, l, m): FA-1 -> l = sum exp(s - rowmax), m = rowmax;
    FA-2 -> l = logsumexp, m = None.  ``opts``: per-call kernel options (see OPTS_*).  ``guard``: "auto" = the call guards itself (a
    forward with the folded scale forms the row norms of q and k inside its own launch and its fp32-scaling twin redoes the call if
    they are beyond the budget); a tensor with ``produce_guard`` = the same, and the tensor (new_guard) is FILLED for the backward of
    this (q, k); a tensor without = a guard computed before (scale_guard); None = none (fp32 scaling).
    ``out_dtype`` = torch.bfloat16: the kernels store O as bf16 (one rounding of the fp32 result; option 9; native d only) -- for
    consumers that take a bf16 activation (sharded.py's gather at half the bytes); the backward needs the fp32 O.
    Any head dim d <= 128: d outside {32, 64, 128} is zero-padded to the next of them on the device (tau keeps the caller's d; the
    reference operator takes any d up to its assert, minitorch/cuda_kernel_ops.py:527-581 / src/flash_attn_fw.cu:43)."""
    return _fwd(_BHND, q, k, v, causal, variant, None, opts, out_dtype, None, None, guard, produce_guard, out, l, m)


def flash_attn_bwd(q, k, v, out, out_grad, l, m=None, causal=False, variant=_lib.FA_VARIANT_FA2,
                   workspace=None, grads=None, stages=STAGE_ALL, opts=None, guard="auto"):
    """Backward.  out: the forward's fp32 output.  Returns (dq, dk, dv) fp32.
    ``stages`` restricts the call to some of its kernels (profiling only); ``opts``: per-call kernel options (see OPTS_*);
    ``guard`` as flash_attn_fwd (pass the forward's guard tensor to save the second pass over q and k)."""
    return _bwd(_BHND, q, k, v, out, out_grad, l, m, causal, variant, None, opts, None, None, guard, grads, workspace, stages)


def flash_attn_fwd_bnhd(q, k, v, causal=False, variant=_lib.FA_VARIANT_FA2, softmax_scale=None, guard="auto", opts=None,
                        produce_guard=False):
    """Forward on (B, N, H, d) tensors -- the layout minitorch's projection writes before its
    permute(0,2,1,3).contiguous() (minitorch/modules_transfomer.py:67-89): no head-split copies.
    Returns (out (B, N, H, d) fp32, l (B, H, N), m (B, H, N) or None).
    ``softmax_scale``: P = softmax(softmax_scale * q.k) instead of the reference's sqrt(1/d) (fa_mi355x_fwd_scaled): for callers that
    fold the scale into their query projection (modules_transformer.multi_head_attention(fold_scale=True)).  With guard = "auto" the
    call guards itself even then (with softmax_scale = ln 2 the library ignores it: the folded factor is 1)."""
    return _fwd(_BNHD, q, k, v, causal, variant, softmax_scale, opts, guard=guard, produce=produce_guard)


def flash_attn_bwd_bnhd(q, k, v, out, out_grad, l, m=None, causal=False, variant=_lib.FA_VARIANT_FA2, softmax_scale=None,
                        guard="auto", opts=None):
    """Backward on (B, N, H, d) tensors; returns (dq, dk, dv) in the same layout, fp32 (``softmax_scale`` as the forward's)."""
    return _bwd(_BNHD, q, k, v, out, out_grad, l, m, causal, variant, softmax_scale, opts, guard=guard)


def flash_attn_fwd_masked(q, k, v, key_mask, causal=False, variant=_lib.FA_VARIANT_FA2):
    """Forward with an additive key mask: P = softmax_k(tau * q.k + key_mask[b, k]), the
    [batch, to_len] mask of the reference's fused softmax (src/softmax_kernel.cu:27-34; 0 keeps a key, -inf drops it).
    q, k, v: (B, H, N, d); key_mask: (B, N) float32.  Returns (out, l, m) as flash_attn_fwd."""
    return _fwd(_BHND, q, k, v, causal, variant, key_mask=key_mask, rank4=_MASK_RANK)


def flash_attn_bwd_masked(q, k, v, out, out_grad, l, m, key_mask, causal=False, variant=_lib.FA_VARIANT_FA2):
    """Backward of flash_attn_fwd_masked; returns (dq, dk, dv) fp32 (no gradient flows into the mask)."""
    return _bwd(_BHND, q, k, v, out, out_grad, l, m, causal, variant, key_mask=key_mask, rank4=_MASK_RANK)


def flash_attn_fwd_dropout(q, k, v, rate, seed, scale=1.0, key_mask=None, causal=False, variant=_lib.FA_VARIANT_FA2):
    """Forward with dropout on the attention probabilities (and an optional key mask): out = scale * (M o P) v with the
    stateless mask of include/flash_attn_mi355x.h (kept iff rate < r, minitorch/nn.py:168-186; scale = 1 is minitorch's
    convention).  q, k, v: (B, H, N, d).  Returns (out, l, m); l / m are the statistics before dropout."""
    return _fwd(_BHND, q, k, v, causal, variant, key_mask=key_mask, dropout=_dropout(rate, scale, seed), rank4=_RANK4)


def flash_attn_bwd_dropout(q, k, v, out, out_grad, l, m, rate, seed, scale=1.0, key_mask=None, causal=False,
                           variant=_lib.FA_VARIANT_FA2):
    """Backward of flash_attn_fwd_dropout (same rate, seed, scale, mask); returns (dq, dk, dv) fp32."""
    return _bwd(_BHND, q, k, v, out, out_grad, l, m, causal, variant, key_mask=key_mask, dropout=_dropout(rate, scale, seed),
                rank4=_RANK4 if key_mask is None else _MASK_RANK)


class _FlashAttnFn(torch.autograd.Function):
    """Autograd contract of the reference's Flash_Attn / Flash_Attn2 / Flash_Attn_Causal
    (minitorch/tensor_functions.py:462-497): forward returns o and saves (q, k, v, o, l, m, causal);
    backward hands them to the SAME variant's backward.  Gradients are cast to the input dtype.  ``layout``: BHND, or BNHD for
    modules_transformer's head-split-free path; ``softmax_scale`` as flash_attn_fwd_bnhd."""

    @staticmethod
    def forward(ctx, q, k, v, causal, variant, layout=_BHND, softmax_scale=None):
        # the forward fills the scale guard inside its own launch and the backward of the same (q, k) reads it; there is none when
        # the caller gives the scale (the kernels' folded factor is then exactly 1), and new_guard gives none where d is not native
        guard = new_guard(q) if softmax_scale is None else None
        o, l, m = _fwd(layout, q, k, v, causal, variant, softmax_scale, guard=guard, produce=True)
        ctx.save_for_backward(q, k, v, o, l, m, guard)   # m is None but for FA-1
        ctx.causal, ctx.variant, ctx.layout, ctx.softmax_scale = causal, variant, layout, softmax_scale
        return o

    @staticmethod
    def backward(ctx, out_grad):
        q, k, v, o, l, m, guard = ctx.saved_tensors
        dq, dk, dv = _bwd(ctx.layout, q, k, v, o, out_grad.to(q.dtype).contiguous(), l, m, ctx.causal, ctx.variant, ctx.softmax_scale,
                          guard=guard)
        return dq.to(q.dtype), dk.to(q.dtype), dv.to(q.dtype), None, None, None, None


def flash_attn(q, k, v, causal=False):        # Tensor.flash_attn, minitorch/tensor.py:422-423
    return _FlashAttnFn.apply(q, k, v, bool(causal), _lib.FA_VARIANT_FA1)


def flash_attn_causal(q, k, v, causal=True):  # Tensor.flash_attn_causal, minitorch/tensor.py:425-426
    return _FlashAttnFn.apply(q, k, v, bool(causal), _lib.FA_VARIANT_FA1)


def flash_attn2(q, k, v, causal=False):       # Tensor.flash_attn2, minitorch/tensor.py:428-429
    return _FlashAttnFn.apply(q, k, v, bool(causal), _lib.FA_VARIANT_FA2)


_DECODE_LAYOUTS = {"bnhd": _lib.FA_LAYOUT_BNHD, "bhnd": _lib.FA_LAYOUT_BHND}


# ---- grouped-query heads (GQA / MQA): fa_mi355x_fwd_gqa / _bwd_gqa ----------------------------------------------------------------
# q has H heads, k and v have Hkv (read from k's shape; H a multiple of it): query head h reads kv head h // (H // Hkv), in place --
# no expanded copy of k or v, forward or backward.  ``layout`` "bnhd": q (B, N, H, d), k and v (B, N, Hkv, d); "bhnd": (B, H, N, d) and
# (B, Hkv, N, d).  dk and dv come back in k's shape.

def _check_gqa(layout, q, k, v, o=None, do=None):
    """The checks of a grouped call, in one order.  Returns (B, H, Hkv, N, d, dtype code) as the C entry points take them."""
    if layout not in _DECODE_LAYOUTS:
        raise ValueError(f"layout must be one of {sorted(_DECODE_LAYOUTS)}")
    _require_gpu(q, "device_ops")
    dtype = _dtype_code(q)
    if q.dim() != 4 or k.dim() != 4:
        raise ValueError("expected 4-d tensors: q (B, N, H, d) and k, v (B, N, Hkv, d) for \"bnhd\", (B, H, N, d) and (B, Hkv, N, d) for \"bhnd\"")
    dev = q.get_device()
    if v.shape != k.shape:
        raise ValueError("k and v must have one shape")
    for t in (k, v):
        if not t.is_cuda or t.dtype != q.dtype or t.get_device() != dev:
            raise ValueError("q, k, v must be GPU tensors of one dtype on one device")
    if layout == "bnhd":
        (B, N, H, d), (Bk, Nk, Hkv, dk) = q.shape, k.shape
    else:
        (B, H, N, d), (Bk, Hkv, Nk, dk) = q.shape, k.shape
    if (B, N, d) != (Bk, Nk, dk):
        raise ValueError(f"q and k disagree on (B, N, d): {(B, N, d)} vs {(Bk, Nk, dk)}")
    if Hkv <= 0 or H % Hkv:
        raise ValueError(f"q's {H} heads must be a multiple of k's {Hkv}")
    if d not in _NATIVE_D:
        raise ValueError("grouped-query heads need a native head dim (32, 64, 128): pad q, k and v (pad_head_dim) and pass softmax_scale")
    if do is not None and (do.shape != q.shape or do.dtype != q.dtype or do.get_device() != dev):
        raise ValueError("out_grad must share q's shape, dtype and device")
    for t in (q, k, v) + ((do,) if do is not None else ()):
        if not t.is_contiguous():
            raise ValueError("tensors must be contiguous")
    if o is not None and (o.dtype is not _F32 or o.shape != q.shape or not o.is_contiguous() or o.get_device() != dev):
        raise ValueError("out must be the forward's contiguous float32 output")
    return B, H, Hkv, N, d, dtype


def _scale_guard_gqa(q, k):
    """scale_guard for tensors with different head counts (fa_mi355x_scale_guard_gqa: q has B*N*H rows of d elements, k B*N*Hkv)."""
    out = torch.empty(_lib.guard_elems(), dtype=_F32, device=q.device)
    d = q.shape[-1]
    _lib.check(_lib.core().fa_mi355x_scale_guard_gqa(_ptr(q), _ptr(k), q.numel() // d, k.numel() // d, d, _dtype_code(q), _ptr(out),
                                                     _stream_ptr()))
    return out


def bwd_workspace_gqa(q, k, layout="bnhd"):
    """Scratch for flash_attn_bwd_gqa with these tensors (fa_mi355x_bwd_workspace_bytes_gqa): the three row-constant vectors and, when
    k has fewer heads than q, two float32 tensors of q's shape (the dK and dV of every query head, which the group sum then adds)."""
    B, H, Hkv, N, d, _ = _check_gqa(layout, q, k, k)
    nbytes = _lib.core().fa_mi355x_bwd_workspace_bytes_gqa(B, H, Hkv, N, d)
    return torch.empty((nbytes + 3) // 4, dtype=_F32, device=q.device)


def flash_attn_fwd_gqa(q, k, v, causal=False, variant=_lib.FA_VARIANT_FA2, softmax_scale=None, layout="bnhd", guard="auto", opts=None,
                       produce_guard=False, out=None):
    """Forward with grouped-query heads.  Returns (out fp32 in q's shape, l (B, H, N), m (B, H, N) or None); ``guard``, ``opts``,
    ``produce_guard`` and ``softmax_scale`` as flash_attn_fwd / flash_attn_fwd_bnhd.  k with q's head count is the ungrouped call."""
    B, H, Hkv, N, d, dtype = _check_gqa(layout, q, k, v)
    if out is not None and (out.dtype is not _F32 or out.shape != q.shape or not out.is_contiguous() or out.get_device() != q.get_device()):
        raise ValueError("out must be a contiguous float32 tensor of q's shape")
    _check_caller(q.get_device(), B * H * N, None, None, guard)
    dev, causal = q.device, int(bool(causal))
    l = torch.empty((B, H, N), dtype=_F32, device=dev)
    m = torch.empty((B, H, N), dtype=_F32, device=dev) if variant == _FA1 else None
    if out is None:
        out = torch.empty(q.shape, dtype=_F32, device=dev)
    arr, cnt = _lib.opts_array(opts)
    if isinstance(guard, str):
        guard, produce_guard = new_guard(q, opts), True
    _lib.check(_lib.core().fa_mi355x_fwd_gqa(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(l), _ptr(m), B, H, Hkv, N, d,
                                             _DECODE_LAYOUTS[layout], float(softmax_scale or 0.0), causal, variant, dtype, arr, cnt,
                                             _ptr(guard), int(bool(produce_guard and guard is not None)), _stream_ptr()))
    return out, l, m


def flash_attn_bwd_gqa(q, k, v, out, out_grad, l, m=None, causal=False, variant=_lib.FA_VARIANT_FA2, softmax_scale=None, layout="bnhd",
                       guard="auto", opts=None, workspace=None, grads=None):
    """Backward with grouped-query heads.  Returns (dq in q's shape, dk, dv in k's shape), fp32.  The dK/dV kernels store one dK and
    one dV per query head into the workspace; one more launch adds every group's heads in ascending order (no atomics: the same bits
    on every run).  ``workspace``: bwd_workspace_gqa(q, k, layout); ``grads``: (dq, dk, dv) buffers to write into."""
    B, H, Hkv, N, d, dtype = _check_gqa(layout, q, k, v, out, out_grad)
    lib, dev = _lib.core(), q.device
    if workspace is not None:
        _check_workspace(workspace, lib.fa_mi355x_bwd_workspace_bytes_gqa(B, H, Hkv, N, d), q.get_device(), "bwd_workspace_gqa(q, k, layout)")
    _check_caller(q.get_device(), B * H * N, l, m, guard)
    if grads is not None:
        for g, like in zip(grads, (q, k, v)):
            _check_buffer(g, q.get_device(), "each of grads", like.numel())
    if workspace is None:
        workspace = bwd_workspace_gqa(q, k, layout)
    dq, dk, dv = grads or (torch.empty(t.shape, dtype=_F32, device=dev) for t in (q, k, v))
    if isinstance(guard, str):   # "auto" on a call that only reads a guard: the separate pass over q and k
        guard = _scale_guard_gqa(q, k) if _wants_guard(q, opts) else None
    arr, cnt = _lib.opts_array(opts)
    _lib.check(lib.fa_mi355x_bwd_gqa(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(out_grad), _ptr(dq), _ptr(dk), _ptr(dv), _ptr(l), _ptr(m),
                                     _ptr(workspace), B, H, Hkv, N, d, _DECODE_LAYOUTS[layout], float(softmax_scale or 0.0),
                                     int(bool(causal)), variant, dtype, STAGE_ALL, arr, cnt, _ptr(guard), _stream_ptr()))
    return dq, dk, dv


class _FlashAttnGqaFn(torch.autograd.Function):
    """flash_attn2 with grouped-query heads under autograd: the forward saves q, the UNEXPANDED k and v, o, l and the scale guard it
    filled; the backward returns k.grad and v.grad in k's shape.  Gradients are cast to the input dtype."""

    @staticmethod
    def forward(ctx, q, k, v, causal, softmax_scale, layout):
        _check_gqa(layout, q, k, v)
        guard = new_guard(q) if softmax_scale is None else None   # (as _FlashAttnFn: a caller's scale makes the folded factor 1)
        o, l, _ = flash_attn_fwd_gqa(q, k, v, causal, _lib.FA_VARIANT_FA2, softmax_scale, layout, guard, produce_guard=True)
        ctx.save_for_backward(q, k, v, o, l, guard)
        ctx.causal, ctx.softmax_scale, ctx.layout = causal, softmax_scale, layout
        return o

    @staticmethod
    def backward(ctx, out_grad):
        q, k, v, o, l, guard = ctx.saved_tensors
        dq, dk, dv = flash_attn_bwd_gqa(q, k, v, o, out_grad.to(q.dtype).contiguous(), l, None, ctx.causal, _lib.FA_VARIANT_FA2,
                                        ctx.softmax_scale, ctx.layout, guard)
        return dq.to(q.dtype), dk.to(q.dtype), dv.to(q.dtype), None, None, None


def flash_attn_gqa(q, k, v, causal=False, softmax_scale=None, layout="bnhd", window=None, sink=None, softcap=None, sink_logits=None):
    """Attention with grouped-query heads under autograd (FA-2): out fp32 in q's shape; q.grad in q's shape and dtype, k.grad and
    v.grad in k's.  ``window`` = W (with ``sink`` = S): row i admits key j iff j <= i and (j > i - W or j < S), the mask of the
    KV-cache calls, through the kernels of libflash_attn_mi355x_window.so; None or 0, W >= N or S >= N is this call without them.
    ``softcap`` = C (causal only): LOGIT SOFT-CAPPING, every score becomes C * tanh(softmax_scale * q.k / C) before the mask, the
    function of flash_attn_decode(..., softcap=), differentiated through the cap (fa_mi355x_fwd_window_softcap / _bwd_window_softcap;
    without a window the call passes W = N).  None or 0 is this call without a cap.
    ``sink_logits`` (causal only; a contiguous float32 (H,) tensor on q's device, which may require grad): LEARNED SINK LOGITS, one
    per query head, a column of every softmax without a value vector, the function of flash_attn_decode(..., sink_logits=)
    (fa_mi355x_fwd_window_lsink; dq, dk, dv through fa_mi355x_bwd_window on this forward's out and lse; ``sink_logits.grad`` float32
    (H,) through fa_mi355x_sink_logits_grad, launched only when the logits require grad).  Works with ``window``; beside
    ``causal=False``, ``softcap`` or ``sink`` it is a ValueError (not built).  None is this call without them."""
    N = q.shape[1 if layout == "bnhd" else 2] if q.dim() == 4 else 0
    if sink_logits is not None:
        if not causal:
            raise ValueError("sink_logits without the causal mask is not built: sink_logits= with causal=False")
        if _check_softcap(softcap) is not None:
            raise ValueError("sink_logits beside a logit cap is not built: sink_logits= with softcap=")
        window = _check_window(window, causal)
        if _check_sink(sink, window) is not None:
            raise ValueError("sink_logits beside sink tokens is not built: sink_logits= with sink=")
        return _lsink_fn(q, k, v, sink_logits, softmax_scale, layout, min(window or N, N) or 1)
    softcap = _check_softcap(softcap)
    if softcap is not None and not causal:
        raise ValueError("softcap without the causal mask is not built: softcap= with causal=False")
    ws = _training_window(window, sink, causal, N)
    if softcap is not None:   # (the capped kernels are the window library's: a call without a window is the one with W = N)
        return _window_fn(q, k, v, softmax_scale, layout, window or N, sink or 0, softcap)
    if ws is not None:
        return _window_fn(q, k, v, softmax_scale, layout, *ws, None)
    return _FlashAttnGqaFn.apply(q, k, v, bool(causal), softmax_scale, layout)


def _pool_dims(k_pool, layout):
    """(num_pages, page_size, Hkv, dp) of a paged cache's pool: (num_pages, page_size, Hkv, dp) for "bnhd", (num_pages, Hkv, page_size,
    dp) for "bhnd", page_size a positive multiple of 128 rows."""
    if k_pool.dim() != 4:
        raise ValueError('the pools of a paged cache are 4-d: (num_pages, page_size, Hkv, dp) for "bnhd", (num_pages, Hkv, page_size, dp) '
                         'for "bhnd"')
    num_pages, page_size, Hkv, dp = k_pool.shape
    if layout != "bnhd":
        page_size, Hkv = Hkv, page_size
    if num_pages <= 0 or page_size <= 0 or page_size % _lib.FA_PAGE_ROWS:
        raise ValueError(f"page_size = {page_size} must be a positive multiple of {_lib.FA_PAGE_ROWS} rows (and the pool hold a page)")
    return num_pages, page_size, Hkv, dp


def _check_table(block_table, B, device):
    if (not isinstance(block_table, torch.Tensor) or block_table.dtype != torch.int32 or block_table.dim() != 2
            or block_table.shape[0] != B or block_table.shape[1] < 1 or block_table.device != device
            or not block_table.is_contiguous()):
        raise ValueError("block_table must be a contiguous int32 tensor of shape (B, max_pages) on q's device")


def _max_pages(block_table, max_pages):
    """The table's second dimension, or the caller's ``max_pages`` (None: a contiguous cache)."""
    if block_table is not None:
        if not isinstance(block_table, torch.Tensor) or block_table.dim() != 2:
            raise ValueError("block_table must be a contiguous int32 tensor of shape (B, max_pages) on q's device")
        return int(block_table.shape[1])
    if max_pages is not None and max_pages < 1:
        raise ValueError("max_pages must be positive")
    return max_pages


# ---- the KV-cache calls (include/flash_attn_mi355x_decode*.h): one path for the three families ----------------------------------
# What "decode" (Nq <= 128 new tokens per sequence), "extend" (any Nq) and "ragged" (packed rows under cu_seqlens_q) do differently,
# as data; everything else is _kv_attention, _kv_append and _kv_workspace below.  ``attend`` / ``append`` / ``workspace``: the public
# names, for the messages; ``packed``: q and the new tokens are (T, H, d) with cu_seqlens_q, not (B, Nq, H, d) -- their rank and the
# messages about them follow it; ``lse``: its shape, in words; ``workspace_none``: a zero-byte workspace is None (the ragged one holds
# the block map: never); ``append_bound``: the most new tokens the append takes on the fp8 and rotary paths; ``fp8``: built for fp8
# caches; ``caches`` / ``cache_rank`` / ``kv_dtype``: the words of three messages; ``symbols``: the entry points and size queries by
# variant (_kv_symbol picks one, _lib.KV_PARAMS has its arguments).
_KV_FAMILIES = {
    "decode": dict(
        attend="flash_attn_decode", append="decode_append", workspace="decode_workspace", packed=False, lse="(B, H, Nq)",
        workspace_none=True, append_bound=128, fp8=True, caches="k_cache and v_cache must have one shape",
        cache_rank="decode expects 4-d q and caches", kv_dtype="q, k_cache and v_cache must share one dtype",
        symbols=dict(
            ungrouped="fa_mi355x_fwd_decode", attend="fa_mi355x_fwd_decode_gqa", fused="fa_mi355x_fwd_decode_append",
            paged="fa_mi355x_fwd_decode_paged", fused_paged="fa_mi355x_fwd_decode_append_paged", window="fa_mi355x_fwd_decode_window",
            sink="fa_mi355x_fwd_decode_sink", softcap="fa_mi355x_fwd_decode_softcap", lsink="fa_mi355x_fwd_decode_lsink",
            fp8="fa_mi355x_fwd_decode_fp8",
            append="fa_mi355x_decode_append",
            append_paged="fa_mi355x_decode_append_paged", append_fp8="fa_mi355x_append_fp8", rope="fa_mi355x_rope_append",
            size_ungrouped="fa_mi355x_decode_workspace_bytes", size="fa_mi355x_decode_workspace_bytes_gqa",
            size_window="fa_mi355x_decode_window_workspace_bytes", size_sink="fa_mi355x_decode_sink_workspace_bytes")),
    "extend": dict(
        attend="flash_attn_extend", append="extend_append", workspace="extend_workspace", packed=False, lse="(B, H, Nq)",
        workspace_none=True, append_bound=None, fp8=True, caches="k_cache and v_cache must have one shape",
        cache_rank="decode expects 4-d q and caches", kv_dtype="q, k_cache and v_cache must share one dtype",
        symbols=dict(
            attend="fa_mi355x_fwd_extend", fused="fa_mi355x_fwd_extend_append", paged="fa_mi355x_fwd_extend_paged",
            fused_paged="fa_mi355x_fwd_extend_append_paged", window="fa_mi355x_fwd_extend_window", sink="fa_mi355x_fwd_extend_sink",
            softcap="fa_mi355x_fwd_extend_softcap", lsink="fa_mi355x_fwd_extend_lsink", fp8="fa_mi355x_fwd_extend_fp8",
            append="fa_mi355x_extend_append",
            append_paged="fa_mi355x_extend_append_paged",
            append_fp8="fa_mi355x_append_fp8", rope="fa_mi355x_rope_append", size="fa_mi355x_extend_workspace_bytes",
            size_window="fa_mi355x_extend_window_workspace_bytes", size_sink="fa_mi355x_extend_sink_workspace_bytes")),
    "ragged": dict(
        attend="flash_attn_ragged", append="ragged_append", workspace="ragged_workspace", packed=True, lse="(H, T)",
        workspace_none=False, append_bound=None, fp8=False, caches="k_cache and v_cache must be 4-d tensors of one shape",
        cache_rank="a ragged call expects 4-d caches", kv_dtype="k_cache and v_cache must share one dtype",
        symbols=dict(
            attend="fa_mi355x_fwd_ragged", fused="fa_mi355x_fwd_ragged_append", paged="fa_mi355x_fwd_ragged_paged",
            fused_paged="fa_mi355x_fwd_ragged_append_paged", window="fa_mi355x_fwd_ragged_window", sink="fa_mi355x_fwd_ragged_sink",
            softcap="fa_mi355x_fwd_ragged_softcap", lsink="fa_mi355x_fwd_ragged_lsink", append="fa_mi355x_ragged_append",
            append_paged="fa_mi355x_ragged_append_paged",
            rope="fa_mi355x_rope_append_ragged",
            size="fa_mi355x_ragged_workspace_bytes", size_window="fa_mi355x_ragged_window_workspace_bytes",
            size_sink="fa_mi355x_ragged_sink_workspace_bytes")),
}


def _kv_symbol(fam, op, paged=False, fused=False, window=None, sink=None, fp8=False, ungrouped=False, softcap=None, lsink=False):
    """The C symbol of a call.  ``op`` "append": the append (fa_mi355x_append_fp8 takes slab and paged caches alike); "size": the size
    query; "attend": the attention -- one entry point per family on an fp8 cache, with sink tokens and with a window (null k_new /
    v_new attend only, a null table is a slab cache), otherwise the _paged and the fused _append forms.  ``window`` None takes the
    unwindowed symbols; ``ungrouped`` (Hkv = H) the ones without an Hkv, where the family has them.  ``softcap`` (not None: a cap
    above 0, never beside sink tokens or an fp8 cache) takes the family's one soft-capping entry point, windowed or not; the size
    queries do not depend on it.  ``lsink`` (learned sink logits: never beside a cap, sink tokens or an fp8 cache) takes the family's
    one _lsink entry point, likewise."""
    symbols = fam["symbols"]
    if op == "append":
        return symbols["append_fp8" if fp8 else "append_paged" if paged else "append"]
    if op == "size":
        if sink is not None:
            return symbols["size_sink"]
        if window is not None:
            return symbols["size_window"]
        return symbols["size_ungrouped"] if ungrouped and "size_ungrouped" in symbols else symbols["size"]
    if softcap is not None:
        return symbols["softcap"]
    if lsink:
        return symbols["lsink"]
    if fp8:
        return symbols["fp8"]
    if sink is not None:
        return symbols["sink"]
    if window is not None:
        return symbols["window"]
    if paged:
        return symbols["fused_paged" if fused else "paged"]
    if fused:
        return symbols["fused"]
    return symbols["ungrouped"] if ungrouped and "ungrouped" in symbols else symbols["attend"]


_KV_ARGS = {symbol: operator.itemgetter(*names) for symbol, names in _lib.KV_CALL_PARAMS.items()}   # fields -> the symbol's argument tuple


def _kv_call(symbol, fields):
    """The one place a KV-cache symbol is called: its arguments are ``fields`` in the order of the header's prototype
    (_lib.KV_PARAMS; one itemgetter per symbol, made at import, does what [fields[n] for n in names] would)."""
    return getattr(_lib.decode(), symbol)(*_KV_ARGS[symbol](fields))


def _kv_geometry(fam, k_cache, layout, max_pages, q=None, cu_seqlens_q=None):
    """(Hkv, dp, Ncap, pool, B, H, Nq, d) of a call.  The cache: (B, Ncap, Hkv, dp) for "bnhd" or (B, Hkv, Ncap, dp) for "bhnd" and
    pool None, or, with ``max_pages`` (_max_pages), a paged cache's pool (_pool_dims), Ncap = max_pages * page_size and pool =
    (num_pages, page_size, max_pages).  q (None, as the appends have none: B, H, Nq, d are None): packed (T, H, d) under cu_seqlens_q
    (B + 1,), or (B, Nq, H, d) for "bnhd" / (B, H, Nq, d) for "bhnd"; H is a multiple of Hkv (grouped-query heads: query head h reads
    cache head h // (H // Hkv)) and B the slab cache's (a pool's first dimension counts pages: the table is what B is held against)."""
    if max_pages is not None:
        num_pages, page_size, Hkv, dp = _pool_dims(k_cache, layout)
        Ncap, pool = max_pages * page_size, (num_pages, page_size, max_pages)
    else:
        if k_cache.dim() != 4:
            raise ValueError(fam["cache_rank"])
        _, Ncap, Hkv, dp = k_cache.shape
        if layout != "bnhd":
            Ncap, Hkv = Hkv, Ncap
        pool = None
    if q is None:
        return Hkv, dp, Ncap, pool, None, None, None, None
    if fam["packed"]:
        if q.dim() != 3:
            raise ValueError("a ragged call expects a 3-d packed q (T, H, d)")
        Nq, H, d = q.shape
        _check_cu(cu_seqlens_q, None if pool else k_cache.shape[0], q.device)
        B = cu_seqlens_q.shape[0] - 1
        if Nq < 1 or Hkv <= 0 or H % Hkv:
            raise ValueError(f"q has {H} heads, the cache {Hkv}: the cache's heads must divide q's (and q hold a row)")
    else:
        if q.dim() != 4:
            raise ValueError("decode expects a 4-d q" if pool else fam["cache_rank"])
        B, Nq, H, d = q.shape
        if layout != "bnhd":
            Nq, H = H, Nq
        if pool:
            if Hkv <= 0 or H % Hkv:
                raise ValueError(f"q has {H} heads, the pool {Hkv}: the pool's heads must divide q's")
        elif B != k_cache.shape[0] or Hkv <= 0 or H % Hkv:
            raise ValueError(f"q and the cache disagree on (B, H): {(B, H)} vs {(k_cache.shape[0], Hkv)} (the cache's heads must divide q's)")
    return Hkv, dp, Ncap, pool, B, H, Nq, d


def _kv_workspace_bytes(fam, B, H, Hkv, Nq, Ncap, dp, window, sink):
    """The family's size query for a call of these sizes."""
    return _kv_call(_kv_symbol(fam, "size", False, False, window, sink, False, Hkv == H),
                    {"B": B, "H": H, "Hkv": Hkv, "Nq": Nq, "Ncap": Ncap, "d": dp, "window": window, "sink": sink})


def _kv_workspace(family, q, k_cache, cu_seqlens_q, layout, block_table, max_pages, window, sink):
    """decode_workspace / extend_workspace / ragged_workspace."""
    fam = _KV_FAMILIES[family]
    if layout not in _DECODE_LAYOUTS:
        raise ValueError(f"layout must be one of {sorted(_DECODE_LAYOUTS)}")
    Hkv, dp, Ncap, _, B, H, Nq, _ = _kv_geometry(fam, k_cache, layout, _max_pages(block_table, max_pages), q, cu_seqlens_q)
    window = _check_window(window)
    nbytes = _kv_workspace_bytes(fam, B, H, Hkv, Nq, Ncap, dp, window, _check_sink(sink, window))
    return torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=q.device) if nbytes or not fam["workspace_none"] else None


def _check_int_option(value, name, counts, unset):
    """An option that counts positions (not None), as the library takes it: an int >= 0 (no bool, no float)."""
    try:
        value = None if isinstance(value, bool) else operator.index(value)
    except TypeError:
        value = None
    if value is None:
        raise ValueError(f"{name} must be None or an int: the number of {counts}")
    if value < 0:
        raise ValueError(f"{name} must not be negative (None or 0: {unset})")
    return value


def _check_window(window, causal=True):
    """``window`` as the library takes it: None stays None (the unwindowed entry points), otherwise an int >= 0 under the causal mask."""
    if window is None:
        return None
    window = _check_int_option(window, "window", "positions a token sees, its own included", "no window")
    if window and not causal:
        raise ValueError("a sliding window needs the causal mask: window= with causal=False")
    return window


def _check_sink(sink, window):
    """``sink`` as the library takes it beside a checked ``window``: None and 0 are None (today's entry points), otherwise an
    int >= 1, which needs a window."""
    if sink is None:
        return None
    sink = _check_int_option(sink, "sink", "first positions every token keeps beside its window", "no sink tokens")
    if sink and window is None:
        raise ValueError("sink tokens stand beside a sliding window: sink= needs window=")
    return sink or None


def _check_softcap(softcap):
    """``softcap`` as the library takes it: None and 0 are None (today's entry points), otherwise a finite number above 0."""
    if softcap is None:
        return None
    if isinstance(softcap, (bool, str)) or not isinstance(softcap, numbers.Real) or not math.isfinite(softcap) or softcap < 0:
        raise ValueError("softcap must be None or a finite number >= 0: the logit cap, softcap * tanh(score / softcap) (None or 0: none)")
    return float(softcap) or None


def _check_sink_logits(sink_logits, H, device):
    """``sink_logits`` of a call with H query heads whose q lives on ``device``: None, or a contiguous float32 (H,) tensor there (one
    learned logit per QUERY head, read on the device)."""
    if sink_logits is None:
        return None
    if (not isinstance(sink_logits, torch.Tensor) or sink_logits.dtype != torch.float32 or tuple(sink_logits.shape) != (H,)
            or sink_logits.device != device or not sink_logits.is_contiguous()):
        raise ValueError(f"sink_logits must be a contiguous float32 tensor of shape (H,) = ({H},) on q's device: one logit per query head")
    return sink_logits


# ---- sliding window and attention sinks in the training forward and backward: fa_mi355x_fwd_window / _bwd_window ------------------
# The mask of the KV-cache calls below with the query of row i at position i: row i admits key j iff j <= i and (j > i - W or j < S).
# Kernels of their own in a library of their own (libflash_attn_mi355x_window.so); they scale in fp32: no guard, no opts.  FA-2 side
# output (lse) only; no key mask, no dropout.

def _training_window(window, sink, causal, N):
    """(W, S) when a call over N positions is a windowed one, None when it is the unwindowed call: window None or 0, W >= N or
    S >= N."""
    window = _check_window(window, causal)
    sink = _check_sink(sink, window)
    if not window or window >= N or (sink or 0) >= N:
        return None
    return window, sink or 0


def _check_window_call(window, sink):
    """``window`` and ``sink`` of the windowed entry points themselves: W >= 1, S >= 0 (larger than N: clamped by the library)."""
    window = _check_window(window)
    sink = _check_sink(sink, window)
    if not window:
        raise ValueError("the windowed call needs window >= 1 (flash_attn_fwd_gqa is the call without a window)")
    return window, sink or 0


# ---- the training-side libraries (window / softcap, varlen, bidir, prefix, local): one path for the families ------------------------
# The NAMES by which the windowed calls here, the packed calls (flash_attn_varlen_*), the bidirectional ones
# (flash_attn_varlen_bidir_*), the causal two-array ones (flash_attn_varlen_prefix_*) and the banded ones (flash_attn_varlen_local_*, all below) differ; _side_fwd, _side_bwd and _side_workspace do the work.  What else a family has of its
# own is code, not this table: its geometry (_side_geometry, over _check_gqa or _check_packed) and its mask scalars (the public
# wrappers).  ``lib`` / ``check``: _lib's getter and status checker, looked up at call time; ``fwd`` / ``bwd``: the entry points
# (under a logit cap: their _softcap forms, the cap behind the window); ``fwd_size`` / ``bwd_size``: the workspace sizes (None: the
# call takes no workspace); ``sizer``: the public call that makes a workspace, for the message; ``wrapper`` (packed families): the
# public call that pads the head dim, likewise.  A call's arguments: the tensors, the geometry, softmax_scale, the mask scalars,
# dtype, stream.
_SIDE_FAMILIES = {
    "window": dict(lib="window", check="window_check", fwd="fa_mi355x_fwd_window", bwd="fa_mi355x_bwd_window", fwd_size=None,
                   bwd_size="fa_mi355x_bwd_window_workspace_bytes", sizer="bwd_workspace_window(q, k, layout)"),
    "varlen": dict(lib="varlen", check="varlen_check", fwd="fa_mi355x_fwd_varlen", bwd="fa_mi355x_bwd_varlen",
                   fwd_size="fa_mi355x_fwd_varlen_workspace_bytes", bwd_size="fa_mi355x_bwd_varlen_workspace_bytes",
                   sizer="varlen_workspace(q, k, cu_seqlens)", wrapper="flash_attn_varlen"),
    "bidir": dict(lib="bidir", check="bidir_check", fwd="fa_mi355x_fwd_bidir", bwd="fa_mi355x_bwd_bidir",
                  fwd_size="fa_mi355x_fwd_bidir_workspace_bytes", bwd_size="fa_mi355x_bwd_bidir_workspace_bytes",
                  sizer="bidir_workspace(q, k, cu_seqlens_q, cu_seqlens_k)", wrapper="flash_attn_varlen_bidir"),
    "prefix": dict(lib="prefix", check="prefix_check", fwd="fa_mi355x_fwd_prefix", bwd="fa_mi355x_bwd_prefix",
                   fwd_size="fa_mi355x_fwd_prefix_workspace_bytes", bwd_size="fa_mi355x_bwd_prefix_workspace_bytes",
                   sizer="prefix_workspace(q, k, cu_seqlens_q, cu_seqlens_k)", wrapper="flash_attn_varlen_prefix"),
    "local": dict(lib="local", check="local_check", fwd="fa_mi355x_fwd_local", bwd="fa_mi355x_bwd_local",
                  fwd_size="fa_mi355x_fwd_local_workspace_bytes", bwd_size="fa_mi355x_bwd_local_workspace_bytes",
                  sizer="local_workspace(q, k, cu_seqlens_q, cu_seqlens_k)", wrapper="flash_attn_varlen_local"),
}


def _side_geometry(family, q, k, v, index, layout, o=None, do=None):
    """The family's checks of its tensors (``index``: the cu_seqlens arrays of a packed call).  Returns (the geometry arguments of
    its entry points, those of its workspace sizes, lse's shape, dtype code)."""
    if family == "window":
        B, H, Hkv, N, d, dtype = _check_gqa(layout, q, k, v, o, do)
        return (B, H, Hkv, N, d, _DECODE_LAYOUTS[layout]), (B, H, Hkv, N, d), (B, H, N), dtype
    nseq, Tq, Tk, H, Hkv, d, dtype = _check_packed(q, k, v, index[0], index[-1], o, do, one_array=family == "varlen",
                                                   wrapper=_SIDE_FAMILIES[family]["wrapper"])
    geom = (nseq, Tq, H, Hkv, d) if family == "varlen" else (nseq, Tq, Tk, H, Hkv, d)
    return geom, geom, (H, Tq), dtype


def _side_buffer(fam, size, sizes, workspace, q):
    """A caller's ``workspace``, checked against the family's size query ``size``, or a new one."""
    nbytes = getattr(getattr(_lib, fam["lib"])(), fam[size])(*sizes)
    if workspace is None:
        return torch.empty((nbytes + 3) // 4, dtype=_F32, device=q.device)
    _check_workspace(workspace, nbytes, q.get_device(), fam["sizer"])
    return workspace


def _side_workspace(family, q, k, index=(), layout="bnhd", backward=True):
    _, sizes, _, _ = _side_geometry(family, q, k, k, index, layout)
    return _side_buffer(_SIDE_FAMILIES[family], "bwd_size" if backward else "fwd_size", sizes, None, q)


def _side_call(fam, op, tensors, geom, softmax_scale, mask, softcap, dtype):
    """The one place a training-side symbol is called."""
    symbol = fam[op]
    if softcap is not None:
        symbol, mask = symbol + "_softcap", (mask[0], softcap, *mask[1:])
    status = getattr(getattr(_lib, fam["lib"])(), symbol)(*map(_ptr, tensors), *geom, float(softmax_scale or 0.0), *mask, dtype, _stream_ptr())
    getattr(_lib, fam["check"])(status)


def _side_fwd(family, q, k, v, index, mask, softmax_scale, layout="bnhd", out=None, lse=None, workspace=None, softcap=None):
    """The forward of a family: the checks (out, workspace, lse), what the caller did not supply (workspace, lse, out), one C call.
    Returns (out, lse)."""
    fam = _SIDE_FAMILIES[family]
    geom, sizes, lse_shape, dtype = _side_geometry(family, q, k, v, index, layout)
    _check_out(out, q)
    workspace = () if fam["fwd_size"] is None else (_side_buffer(fam, "fwd_size", sizes, workspace, q),)
    if lse is None:
        lse = torch.empty(lse_shape, dtype=_F32, device=q.device)
    else:
        _check_buffer(lse, q.get_device(), "lse", math.prod(lse_shape))
    if out is None:
        out, = _new_f32(q)
    _side_call(fam, "fwd", (q, k, v, out, lse, *index, *workspace), geom, softmax_scale, mask, softcap, dtype)
    return out, lse


def _side_bwd(family, q, k, v, out, out_grad, lse, index, mask, softmax_scale, layout="bnhd", workspace=None, grads=None, softcap=None):
    """The backward of a family, likewise: every buffer of the caller is checked (lse, workspace, grads) before one is allocated
    (workspace, grads).  Returns (dq, dk, dv)."""
    fam = _SIDE_FAMILIES[family]
    geom, sizes, lse_shape, dtype = _side_geometry(family, q, k, v, index, layout, out, out_grad)
    _check_buffer(lse, q.get_device(), "lse", math.prod(lse_shape))
    if workspace is not None:
        _side_buffer(fam, "bwd_size", sizes, workspace, q)
    _check_grads(grads, q, k, v)
    if workspace is None:
        workspace = _side_buffer(fam, "bwd_size", sizes, None, q)
    dq, dk, dv = grads or _new_f32(q, k, v)
    _side_call(fam, "bwd", (q, k, v, out, out_grad, dq, dk, dv, lse, *index, workspace), geom, softmax_scale, mask, softcap, dtype)
    return dq, dk, dv


class _FlashAttnSideFn(torch.autograd.Function):
    """A family's public forward and backward (``fwd``, ``bwd``: flash_attn_fwd_window / _bwd_window, flash_attn_varlen_fwd / _bwd,
    flash_attn_varlen_bidir_fwd / _bwd) under autograd.  ``index``: the tensors both take behind the operands (the cu_seqlens arrays);
    ``options``: the keywords both take.  The forward saves q, the unexpanded k and v, o, lse and the index tensors; gradients are cast
    to the input dtype (k and v have q's, by the checks).  ``learned``: further DIFFERENTIABLE tensors both take behind the index (the
    learned sink logits); ``bwd`` then also takes ``wanted``, which of them need a gradient, and returns theirs (None where not
    wanted) behind dq, dk, dv."""

    @staticmethod
    def forward(ctx, fwd, bwd, q, k, v, index, options, *learned):
        o, lse = fwd(q, k, v, *index, *learned, **options)
        ctx.save_for_backward(q, k, v, o, lse, *index, *learned)
        ctx.bwd, ctx.options, ctx.n_learned = bwd, options, len(learned)
        return o

    @staticmethod
    def backward(ctx, out_grad):
        q, k, v, o, lse, *rest = ctx.saved_tensors
        more = {"wanted": tuple(ctx.needs_input_grad[7:])} if ctx.n_learned else {}
        dq, dk, dv, *dlearned = ctx.bwd(q, k, v, o, out_grad.to(q.dtype).contiguous(), lse, *rest, **ctx.options, **more)
        return (None, None, dq.to(q.dtype), dk.to(q.dtype), dv.to(q.dtype), None, None, *dlearned)


def _native_head_dim(q, k, v, softmax_scale, attend):
    """attend(q, k, v, softmax_scale) for packed tensors of any head dim: one other than 32, 64, 128 runs through zero-padded columns
    with softmax_scale = 1 / sqrt(d), and the result loses them again."""
    d = q.shape[-1] if isinstance(q, torch.Tensor) and q.dim() == 3 else 0
    if not d or d in _NATIVE_D:
        return attend(q, k, v, softmax_scale)
    dp = padded_head_dim(d)
    scale = softmax_scale if softmax_scale is not None else d ** -0.5
    return attend(pad_head_dim(q, dp), pad_head_dim(k, dp), pad_head_dim(v, dp), scale)[..., :d]


def _window_fn(q, k, v, softmax_scale, layout, window, sink, softcap):
    """flash_attn_gqa under a sliding window (and sink tokens), with or without a logit cap."""
    return _FlashAttnSideFn.apply(flash_attn_fwd_window, flash_attn_bwd_window, q, k, v, (),
                                  dict(window=window, sink=sink, softmax_scale=softmax_scale, layout=layout, softcap=softcap))


# ---- learned sink logits in training (include/flash_attn_mi355x_lsink.h; libflash_attn_mi355x_lsink.so) ------------------------------
# gpt-oss's one fp32 logit per query head, a column of every row's softmax without a value vector, under the causal (windowed) mask:
# the function flash_attn_decode(..., sink_logits=) generates with.  The forward is a kernel of its own; dq, dk and dv are
# flash_attn_bwd_window on this forward's out and lse (P = exp2(s c - lse log2 e) and delta = rowsum(dO o out) are what it computes
# from what it is given); the gradient of the logits, d a_h = -sum_{b,i} e^(a_h - lse_bhi) delta_bhi, is sink_logits_grad.

def flash_attn_fwd_window_lsink(q, k, v, window, sink_logits, softmax_scale=None, layout="bnhd", out=None):
    """Causal forward under a sliding window of ``window`` positions (>= 1; N and above: no window) with learned sink logits
    (fa_mi355x_fwd_window_lsink): ``sink_logits`` a contiguous float32 (H,) tensor on q's device, read there.  Grouped-query heads as
    flash_attn_fwd_gqa.  Returns (out fp32 in q's shape, lse (B, H, N) = ln(e^a + sum_j e^z_j))."""
    window, _ = _check_window_call(window, None)
    B, H, Hkv, N, d, dtype = _check_gqa(layout, q, k, v)
    _check_sink_logits(sink_logits, H, q.device)
    if sink_logits is None:
        raise ValueError("sink_logits must be a contiguous float32 (H,) tensor: flash_attn_fwd_window is the call without the logits")
    _check_out(out, q)
    lse = torch.empty((B, H, N), dtype=_F32, device=q.device)
    if out is None:
        out, = _new_f32(q)
    _lib.lsink_check(_lib.lsink().fa_mi355x_fwd_window_lsink(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(lse), _ptr(sink_logits), B, H, Hkv, N,
                                                            d, _DECODE_LAYOUTS[layout], float(softmax_scale or 0.0), window, dtype,
                                                            _stream_ptr()))
    return out, lse


def lsink_workspace(q, layout="bnhd"):
    """Scratch for sink_logits_grad with an out of q's shape (fa_mi355x_sink_logits_grad_workspace_bytes: one partial per head and
    slice of 512 rows)."""
    B, H, _, N, d, _ = _check_gqa(layout, q, q, q)
    nbytes = _lib.lsink().fa_mi355x_sink_logits_grad_workspace_bytes(B, H, N, d)
    return torch.empty((nbytes + 3) // 4, dtype=_F32, device=q.device)


def sink_logits_grad(out, out_grad, lse, sink_logits, layout="bnhd", workspace=None):
    """The gradient of the learned sink logits (fa_mi355x_sink_logits_grad): float32 (H,), -sum over every row of the head of
    e^(a - lse) * rowsum(out_grad o out).  ``out`` (fp32) and ``lse`` are flash_attn_fwd_window_lsink's, ``out_grad`` has out's shape
    and the forward's input dtype.  Two launches, no atomics: the same bits on every run.  ``workspace``: lsink_workspace(q, layout)."""
    B, H, _, N, d, dtype = _check_gqa(layout, out_grad, out_grad, out_grad, out)
    _check_sink_logits(sink_logits, H, out.device)
    _check_buffer(lse, out.get_device(), "lse", B * H * N)
    nbytes = _lib.lsink().fa_mi355x_sink_logits_grad_workspace_bytes(B, H, N, d)
    if workspace is None:
        workspace = torch.empty((nbytes + 3) // 4, dtype=_F32, device=out.device)
    else:
        _check_workspace(workspace, nbytes, out.get_device(), "lsink_workspace(q, layout)")
    grad = torch.empty(H, dtype=_F32, device=out.device)
    _lib.lsink_check(_lib.lsink().fa_mi355x_sink_logits_grad(_ptr(out), _ptr(out_grad), _ptr(lse), _ptr(sink_logits), _ptr(grad),
                                                            _ptr(workspace), B, H, N, d, _DECODE_LAYOUTS[layout], dtype, _stream_ptr()))
    return grad


def _lsink_fwd(q, k, v, sink_logits, window, softmax_scale, layout):
    """flash_attn_fwd_window_lsink with the learned tensor behind the operands, as _FlashAttnSideFn passes it."""
    return flash_attn_fwd_window_lsink(q, k, v, window, sink_logits, softmax_scale, layout)


def _lsink_bwd(q, k, v, out, out_grad, lse, sink_logits, window, softmax_scale, layout, wanted):
    """The backward of flash_attn_fwd_window_lsink under autograd: the EXISTING windowed backward on this forward's out and lse, and
    the logits' gradient only where it is wanted (no launch otherwise)."""
    dq, dk, dv = flash_attn_bwd_window(q, k, v, out, out_grad, lse, window, None, softmax_scale, layout)
    return dq, dk, dv, (sink_logits_grad(out, out_grad, lse, sink_logits, layout) if wanted[0] else None)


def _lsink_fn(q, k, v, sink_logits, softmax_scale, layout, window):
    """flash_attn_gqa with learned sink logits: the project's one training-side Function, the logits its one learned tensor."""
    return _FlashAttnSideFn.apply(_lsink_fwd, _lsink_bwd, q, k, v, (),
                                  dict(window=window, softmax_scale=softmax_scale, layout=layout), sink_logits)


def bwd_workspace_window(q, k, layout="bnhd"):
    """Scratch for flash_attn_bwd_window with these tensors (fa_mi355x_bwd_window_workspace_bytes): as bwd_workspace_gqa."""
    return _side_workspace("window", q, k, (), layout)


def flash_attn_fwd_window(q, k, v, window, sink=None, softmax_scale=None, layout="bnhd", out=None, softcap=None):
    """Causal forward under a sliding window of ``window`` positions and ``sink`` first positions, grouped-query heads as
    flash_attn_fwd_gqa.  Returns (out fp32 in q's shape, lse (B, H, N)).  ``softcap``: logit soft-capping, as in flash_attn_gqa
    (fa_mi355x_fwd_window_softcap; lse is taken over the capped logits); None or 0: none, today's call."""
    mask = _check_window_call(window, sink)
    return _side_fwd("window", q, k, v, (), mask, softmax_scale, layout, out, softcap=_check_softcap(softcap))


def flash_attn_bwd_window(q, k, v, out, out_grad, lse, window, sink=None, softmax_scale=None, layout="bnhd", workspace=None, grads=None,
                          softcap=None):
    """Backward of flash_attn_fwd_window.  Returns (dq in q's shape, dk, dv in k's shape), fp32; no atomics, the same bits on every
    run.  ``workspace``: bwd_workspace_window(q, k, layout); ``grads``: (dq, dk, dv) buffers to write into.  ``softcap``: the cap of
    the forward that made out and lse (fa_mi355x_bwd_window_softcap; the workspace does not depend on it)."""
    mask = _check_window_call(window, sink)
    return _side_bwd("window", q, k, v, out, out_grad, lse, (), mask, softmax_scale, layout, workspace, grads, _check_softcap(softcap))


def decode_workspace(q, k_cache, layout="bnhd", block_table=None, max_pages=None, window=None, sink=None):
    """Scratch for flash_attn_decode with these tensors (fa_mi355x_decode_workspace_bytes; one partial O, m, l per query row and key
    chunk), or None when the call runs as one split and needs none.  A pure function of the shapes: allocate once, reuse every step.
    A paged call (``k_cache`` the pool): give the block table or its ``max_pages``; the size is the contiguous call's for
    Ncap = max_pages * page_size.  ``window``: for flash_attn_decode(..., window=) (fa_mi355x_decode_window_workspace_bytes: the
    splits follow the window span, not the cache).  ``sink``: for flash_attn_decode(..., window=, sink=)
    (fa_mi355x_decode_sink_workspace_bytes).  An fp8 cache is sized as the bf16 cache of its shape is (the same splits)."""
    return _kv_workspace("decode", q, k_cache, None, layout, block_table, max_pages, window, sink)


def extend_workspace(q, k_cache, layout="bnhd", block_table=None, max_pages=None, window=None, sink=None):
    """decode_workspace for flash_attn_extend (fa_mi355x_extend_workspace_bytes: the extend call has a split policy of its own;
    ``window``: fa_mi355x_extend_window_workspace_bytes; ``sink``: fa_mi355x_extend_sink_workspace_bytes)."""
    return _kv_workspace("extend", q, k_cache, None, layout, block_table, max_pages, window, sink)


_FP8 = getattr(torch, "float8_e4m3fn", None)   # the dtype of an fp8 KV cache (include/flash_attn_mi355x_decode_fp8.h)
_RAGGED_FP8 = ("the ragged calls on an fp8 (torch.float8_e4m3fn) cache are not built: use flash_attn_decode / flash_attn_extend "
               "and decode_append / extend_append")


def _is_fp8(t):
    return _FP8 is not None and t.dtype == _FP8


def _check_scales(k_scale, v_scale, fp8, Hkv, device):
    """``k_scale`` / ``v_scale`` of an fp8 cache: None (all ones) or contiguous float32 (Hkv,) tensors on the cache's device.  Given
    with any other cache they are an error, not ignored."""
    if not fp8:
        if k_scale is not None or v_scale is not None:
            raise ValueError("k_scale and v_scale belong to an fp8 (torch.float8_e4m3fn) cache: this cache is not one")
        return
    for name, t in (("k_scale", k_scale), ("v_scale", v_scale)):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError(f"{name} must be a float32 tensor of shape (Hkv,) = ({Hkv},)")
        if tuple(t.shape) != (Hkv,) or not t.is_contiguous() or t.device != device:
            raise ValueError(f"{name} must be a contiguous float32 tensor of shape (Hkv,) = ({Hkv},) on the cache's device")


def _check_seqlens(cache_seqlens, B, device):
    if cache_seqlens is not None and (cache_seqlens.dtype != torch.int32 or tuple(cache_seqlens.shape) != (B,)
                                      or cache_seqlens.device != device or not cache_seqlens.is_contiguous()):
        raise ValueError("cache_seqlens must be a contiguous int32 tensor of shape (B,) on q's device")


def _check_new(fam, k_new, v_new, k_cache, layout, Nq, Hkv, dp, Bc):
    """(n, d_new) of the new tokens' k_new / v_new -- packed (T, Hkv, d_new), or (B, n, Hkv, d_new) for "bnhd" / (B, Hkv, n, d_new) for
    "bhnd" -- checked against the cache they are appended to (Hkv heads of dp columns, and ``Bc`` batch elements; None: a pool, whose
    first dimension counts pages) and against the caller's Nq, when given."""
    packed = fam["packed"]
    if k_new.dim() != (3 if packed else 4) or k_new.shape != v_new.shape:
        raise ValueError("k_new and v_new must be 3-d packed tensors (T, Hkv, d_new) of one shape" if packed else
                         "k_new and v_new must be 4-d tensors of one shape")
    if _is_fp8(k_cache):
        if k_new.dtype != torch.bfloat16 or v_new.dtype != torch.bfloat16:
            raise TypeError("an fp8 cache takes bfloat16 k_new and v_new (they are quantised on the device)")
    elif k_new.dtype != k_cache.dtype or v_new.dtype != k_cache.dtype:
        raise TypeError("k_new and v_new must have the cache's dtype")
    if packed:
        n, hkv, d_new = k_new.shape
        if hkv != Hkv:
            raise ValueError(f"k_new and the cache disagree on Hkv: {hkv} vs {Hkv}")
    else:
        B, n, hkv, d_new = k_new.shape if layout == "bnhd" else (k_new.shape[0], k_new.shape[2], k_new.shape[1], k_new.shape[3])
        if (B, hkv) != (B if Bc is None else Bc, Hkv):
            raise ValueError(f"k_new and the cache disagree on (B, Hkv): {(B, hkv)} vs {(B if Bc is None else Bc, Hkv)}")
    if Nq is not None and n != Nq:
        raise ValueError(f"k_new holds {n} {'packed rows' if packed else 'new tokens'}, q {Nq}")
    if (packed and n < 1) or not 1 <= d_new <= dp:
        raise ValueError(f"k_new's head dim {d_new} must be in 1 .. {dp}, the cache's row length" + " (and k_new hold a row)" * packed)
    for t in (k_new, v_new):
        if t.device != k_cache.device:
            raise ValueError("k_new and v_new must live on the cache's device")
        if not t.is_contiguous():
            raise ValueError("k_new and v_new must be contiguous")
    return n, d_new


# ---- rotary position embeddings (include/flash_attn_mi355x_decode_rope.h) ----

def rotary_table(max_pos, rot, base=10000.0, device=None):
    """The (cos, sin) tables of a rotary embedding, float32 (max_pos, rot // 2) on ``device``: the angle of position p and pair j is
    p * base ** (-2 j / rot), computed in float64 and rounded once.  Any other table (scaled, YaRN) can be built by the caller: the
    kernels only read what they are given."""
    rot, max_pos = operator.index(rot), operator.index(max_pos)
    if rot < 2 or rot % 2:
        raise ValueError("rot, the rotary dimension, must be even and at least 2")
    if max_pos < 1:
        raise ValueError("max_pos must be positive")
    inv = float(base) ** (-torch.arange(0, rot, 2, dtype=torch.float64) / rot)
    ang = torch.arange(max_pos, dtype=torch.float64)[:, None] * inv[None, :]
    return (ang.cos().to(torch.float32).to(device).contiguous(), ang.sin().to(torch.float32).to(device).contiguous())


def _check_rotary(cos, sin, device, interleaved=False):
    """``rotary_cos`` / ``rotary_sin`` as the library takes them: both None is None (no rotary: the paths without it); otherwise contiguous
    float32 (max_pos, rot / 2) tensors of one shape on ``device``, and the answer is (rot, max_pos, interleaved as 0 / 1)."""
    if cos is None and sin is None:
        return None
    if cos is None or sin is None:
        raise ValueError("rotary_cos and rotary_sin go together: give both tables or neither")
    for name, t in (("rotary_cos", cos), ("rotary_sin", sin)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError(f"{name} must be a float32 tensor of shape (max_pos, rot / 2)")
    if cos.dim() != 2 or cos.shape != sin.shape or cos.shape[0] < 1 or cos.shape[1] < 1:
        raise ValueError("rotary_cos and rotary_sin must have one shape, (max_pos, rot / 2)")
    if cos.device != device or sin.device != device:
        raise ValueError("rotary_cos and rotary_sin must live on the device of the tensors they rotate")
    if not cos.is_contiguous() or not sin.is_contiguous():
        raise ValueError("rotary_cos and rotary_sin must be contiguous")
    return 2 * cos.shape[1], cos.shape[0], int(bool(interleaved))


def _rotary_call(x, y, cos, sin, seqlen_offsets, interleaved, inverse, layout):
    B, N, H, d = x.shape if layout == "bnhd" else (x.shape[0], x.shape[2], x.shape[1], x.shape[3])
    rot, max_pos, il = _check_rotary(cos, sin, x.device, interleaved)
    _lib.decode_check(_lib.decode().fa_mi355x_rope(
        _ptr(x), _ptr(y), _ptr(cos), _ptr(sin), _ptr(seqlen_offsets), B, N, H, d, rot, max_pos, _DECODE_LAYOUTS[layout], il,
        int(bool(inverse)), _dtype_code(x), _stream_ptr()))
    return y


class _RotaryFn(torch.autograd.Function):
    """apply_rotary under autograd: a rotation is orthogonal, so the gradient is the inverse rotation of the cotangent."""

    @staticmethod
    def forward(ctx, x, cos, sin, seqlen_offsets, interleaved, inverse, layout, out):
        ctx.save_for_backward(cos, sin, seqlen_offsets)
        ctx.how = (interleaved, inverse, layout)
        if out is None:
            out = torch.empty_like(x)
        else:   # (an input that the call fills: x itself for the in-place rotation)
            ctx.mark_dirty(out)
        return _rotary_call(x, out, cos, sin, seqlen_offsets, interleaved, inverse, layout)

    @staticmethod
    def backward(ctx, g):
        cos, sin, seqlen_offsets = ctx.saved_tensors
        interleaved, inverse, layout = ctx.how
        g = g.contiguous()
        return _rotary_call(g, torch.empty_like(g), cos, sin, seqlen_offsets, interleaved, not inverse, layout), None, None, None, None, None, None, None


def apply_rotary(x, cos, sin, seqlen_offsets=None, interleaved=False, inverse=False, layout="bnhd", out=None):
    """Rotary position embedding of a tensor (fa_mi355x_rope, include/flash_attn_mi355x_decode_rope.h): x (B, N, H, d) for "bnhd" or
    (B, H, N, d) for "bhnd", float32 or bfloat16, contiguous; ``cos`` / ``sin`` contiguous float32 (max_pos, rot / 2) on x's device
    (rotary_table), rot even and <= d.  Row i of batch element b sits at position seqlen_offsets[b] + i (``seqlen_offsets``: a
    contiguous int32 (B,) tensor on x's device, read on the device; None: zeros), clamped to the table on the device.  Pair j of a
    row is (x[j], x[j + rot/2]) (NeoX / Llama) or, ``interleaved``, (x[2j], x[2j+1]) (GPT-J); with c, s the pair's table entries
    y1 = x1 c - x2 s and y2 = x2 c + x1 s in float32, rounded once to x's dtype; ``inverse`` takes -s.  Columns rot .. d-1 are
    copied.  ``out``: a contiguous tensor of x's shape and dtype, which may be x (in place).  Differentiable in x: the backward is
    the inverse rotation of the gradient."""
    if layout not in _DECODE_LAYOUTS:
        raise ValueError(f"layout must be one of {sorted(_DECODE_LAYOUTS)}")
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError("apply_rotary expects a 4-d x")
    _dtype_code(x)
    rot = _check_rotary(cos, sin, x.device)
    if rot is None:
        raise ValueError("apply_rotary needs both tables, cos and sin")
    if rot[0] > x.shape[3]:
        raise ValueError(f"the tables' rotary dimension {rot[0]} exceeds x's head dim {x.shape[3]}")
    if seqlen_offsets is not None and (not isinstance(seqlen_offsets, torch.Tensor) or seqlen_offsets.dtype != torch.int32
                                       or tuple(seqlen_offsets.shape) != (x.shape[0],) or seqlen_offsets.device != x.device
                                       or not seqlen_offsets.is_contiguous()):
        raise ValueError("seqlen_offsets must be a contiguous int32 tensor of shape (B,) on x's device")
    if not x.is_contiguous():
        raise ValueError("x must be contiguous")
    if out is not None and (out.shape != x.shape or out.dtype != x.dtype or out.device != x.device or not out.is_contiguous()):
        raise ValueError("out must be a contiguous tensor of x's shape, dtype and device")
    _require_gpu(x, "apply_rotary")
    return _RotaryFn.apply(x, cos, sin, seqlen_offsets, bool(interleaved), bool(inverse), layout, out)


def _rope_append(fam, fields, rotary, fp8=False):
    """The roped append in front of an attend-only call (the family's ``rope`` symbol): the q of ``fields`` -> its q_rot,
    k_new -> the K cache, both rotated at the positions the append gives the tokens, v_new -> the V cache; q / q_rot or k_new / v_new
    may be null."""
    cos, sin, (rot, max_pos, interleaved) = rotary
    _lib.decode_check(_kv_call(fam["symbols"]["rope"], dict(fields, cos=_ptr(cos), sin=_ptr(sin), rot=rot, max_pos=max_pos,
                                                            interleaved=interleaved, cache_fp8=int(bool(fp8)))))


def _rotary_of(rotary_cos, rotary_sin, rotary_interleaved, device):
    """None (no rotary), or (cos, sin, (rot, max_pos, interleaved)) of checked tables."""
    if rotary_cos is None and rotary_sin is None:
        return None
    dims = _check_rotary(rotary_cos, rotary_sin, device, rotary_interleaved)
    return None if dims is None else (rotary_cos, rotary_sin, dims)


def _check_rot(rotary, d, d_new=None):
    rot = rotary[2][0]
    if rot > d or (d_new is not None and rot > d_new):
        raise ValueError(f"the tables' rotary dimension {rot} exceeds the head dim of the rows it rotates ({d if d_new is None else min(d, d_new)})")


def _q_rot_buffer(q_rot, q, qp):
    """The tensor the rotated (padded) q goes into: the caller's ``q_rot`` where it fits as it is, otherwise a new one."""
    if q_rot is not None and (not isinstance(q_rot, torch.Tensor) or q_rot.shape != q.shape or q_rot.dtype != q.dtype
                              or q_rot.device != q.device or not q_rot.is_contiguous()):
        raise ValueError("q_rot must be a contiguous tensor of q's shape, dtype and device")
    if q_rot is None:
        return torch.empty_like(qp)
    return q_rot if qp is q else pad_head_dim(q_rot, qp.shape[-1])   # (padded: rows a ragged call does not own come back as they were)


def _kv_append(family, k_new, v_new, k_cache, v_cache, cu_seqlens_q, cache_seqlens, layout, block_table, k_scale, v_scale, rotary_cos,
               rotary_sin, rotary_interleaved, q_rot):
    """decode_append / extend_append / ragged_append: the checks, then the family's append (its _paged form when there is a block
    table; for an fp8 cache fa_mi355x_append_fp8, which quantises; with rotary tables the roped append without a q, one entry point
    for any Nq, slab or paged, fp8 or not)."""
    fam = _KV_FAMILIES[family]
    rotary = _rotary_of(rotary_cos, rotary_sin, rotary_interleaved, k_cache.device)
    if q_rot is not None:
        raise ValueError("q_rot belongs to a call that has a q: an append rotates k_new only")
    if layout not in _DECODE_LAYOUTS:
        raise ValueError(f"layout must be one of {sorted(_DECODE_LAYOUTS)}")
    if k_cache.dim() != 4 or k_cache.shape != v_cache.shape:
        raise ValueError("k_cache and v_cache must be 4-d tensors of one shape")
    if v_cache.dtype != k_cache.dtype:
        raise TypeError("k_cache and v_cache must share one dtype")
    fp8 = _is_fp8(k_cache)
    if fp8 and not fam["fp8"]:
        raise TypeError(_RAGGED_FP8)
    dtype = _lib.FA_DTYPE_BF16 if fp8 else _dtype_code(k_cache)
    Hkv, dp, Ncap, pool, *_ = _kv_geometry(fam, k_cache, layout, None if block_table is None else _max_pages(block_table, None))
    Bc = None if pool else k_cache.shape[0]
    Nq, d_new = _check_new(fam, k_new, v_new, k_cache, layout, None, Hkv, dp, Bc)
    if fam["packed"]:
        _check_cu(cu_seqlens_q, Bc, k_cache.device)
    B = cu_seqlens_q.shape[0] - 1 if fam["packed"] else k_new.shape[0]
    _check_scales(k_scale, v_scale, fp8, Hkv, k_cache.device)
    _check_seqlens(cache_seqlens, B, k_cache.device)
    if pool:
        _check_table(block_table, B, k_cache.device)
    for t in (k_cache, v_cache):
        if t.device != k_cache.device or not t.is_contiguous():
            raise ValueError("k_cache and v_cache must be contiguous and live on one device")
        _require_gpu(t, fam["append"])
    if (fp8 or rotary) and fam["append_bound"] and Nq > fam["append_bound"]:
        raise ValueError(f"{fam['append']} takes at most {fam['append_bound']} new tokens per call: use extend_append")
    num_pages, page_size, max_pages = pool or (0, 0, 0)
    fields = {   # what the family's appends take, by the names of the prototypes (a paged cache goes without an Ncap)
        "q": None, "q_rot": None, "k_new": k_new.data_ptr(), "v_new": v_new.data_ptr(), "k_cache": k_cache.data_ptr(),
        "v_cache": v_cache.data_ptr(), "k_scale": _ptr(k_scale), "v_scale": _ptr(v_scale), "cu_seqlens_q": _ptr(cu_seqlens_q),
        "cache_seqlens": _ptr(cache_seqlens), "block_table": _ptr(block_table), "B": B, "H": Hkv, "Hkv": Hkv, "Nq": Nq,
        "Ncap": 0 if pool else Ncap, "num_pages": num_pages, "page_size": page_size, "max_pages": max_pages, "d_new": d_new, "d": dp,
        "layout": _DECODE_LAYOUTS[layout], "dtype": dtype, "stream": _stream_ptr()}
    if rotary:   # (no q, so k_new alone is rotated)
        _check_rot(rotary, dp, d_new)
        _rope_append(fam, fields, rotary, fp8)
    else:
        _lib.decode_check(_kv_call(_kv_symbol(fam, "append", paged=pool is not None, fp8=fp8), fields))


def decode_append(k_new, v_new, k_cache, v_cache, cache_seqlens=None, layout="bnhd", block_table=None, k_scale=None, v_scale=None,
                  rotary_cos=None, rotary_sin=None, rotary_interleaved=False, q_rot=None):
    """Write the Nq <= 128 new tokens' k and v into the caches on the device (fa_mi355x_decode_append): k_new, v_new (B, Nq, Hkv,
    d_new) for "bnhd" or (B, Hkv, Nq, d_new) for "bhnd", 1 <= d_new <= dp, into caches (B, Ncap, Hkv, dp) / (B, Hkv, Ncap, dp).
    ``cache_seqlens`` COUNTS the new tokens, as flash_attn_decode reads it: token i goes to row clamp(len_b, 0, Ncap) - Nq + i when
    that is >= 0 (None: the last Nq rows), with zeros in columns d_new .. dp-1; every other row keeps its contents.  k_new and v_new
    must not alias the caches.  In place, no host synchronisation.  ``block_table`` (int32 (B, max_pages)): the caches are the pools
    of a paged cache (flash_attn_decode), row r of batch element b is row r % page_size of page block_table[b, r // page_size], and
    Ncap = max_pages * page_size; a page that two sequences share is written by both (the caller keeps appends off shared pages).
    An FP8 cache (torch.float8_e4m3fn caches, bfloat16 k_new / v_new; fa_mi355x_append_fp8): every element x of kv head h is stored
    as the e4m3 code of clamp(x * (1 / scale[h]), -448, 448), rounded to nearest even (overflow saturates to +-448, a NaN stores the
    NaN code 0x7F), with ``k_scale`` / ``v_scale`` contiguous float32 (Hkv,) on the cache's device (None: ones); columns d_new .. dp-1
    are zero bytes.  Scales with any other cache are an error.
    ``rotary_cos`` / ``rotary_sin`` (both or neither; rotary_table): k_new is ROTATED on its way into the K cache
    (fa_mi355x_rope_append without a q): token i of batch element b at position clamp(len_b, 0, Ncap) - Nq + i, the row it is
    written to; ``rotary_interleaved`` picks GPT-J pairs.  The tables must cover the cache (max_pos >= Ncap).  v_new is never
    rotated.  ``q_rot`` must stay None here (an append has no q)."""
    _kv_append("decode", k_new, v_new, k_cache, v_cache, None, cache_seqlens, layout, block_table, k_scale, v_scale, rotary_cos, rotary_sin,
               rotary_interleaved, q_rot)


def extend_append(k_new, v_new, k_cache, v_cache, cache_seqlens=None, layout="bnhd", block_table=None, k_scale=None, v_scale=None,
                  rotary_cos=None, rotary_sin=None, rotary_interleaved=False, q_rot=None):
    """decode_append for any number of new tokens (fa_mi355x_extend_append: the same kernel, placement and checks, no bound on Nq)."""
    _kv_append("extend", k_new, v_new, k_cache, v_cache, None, cache_seqlens, layout, block_table, k_scale, v_scale, rotary_cos, rotary_sin,
               rotary_interleaved, q_rot)


def _kv_attention(family, q, k_cache, v_cache, cu_seqlens_q, cache_seqlens, causal, softmax_scale, layout, out, lse, workspace, k_new, v_new,
                  block_table, max_pages, window, k_scale, v_scale, sink, rotary_cos, rotary_sin, rotary_interleaved, q_rot, softcap=None,
                  sink_logits=None):
    """flash_attn_decode / flash_attn_extend / flash_attn_ragged: the checks in one order (the options; the caches and their dtypes; the
    geometry; q, the lengths, the table, the new tokens; devices and strides; out, lse, the workspace's size; the GPU; the tables' rotary
    dimension and q_rot), the head-dim padding, the buffers the caller did not supply, then the entry point _kv_symbol picks.  With
    rotary tables: the roped append (q -> q_rot, the rotated k_new and v_new into the caches), then the ATTEND-ONLY form of the same
    choice on q_rot.  ``softcap``: the family's soft-capping entry point (a window rides along, 0 without one); refused beside sink
    tokens and on an fp8 cache before any library call.  ``sink_logits``: the family's _lsink entry point (a window rides along
    likewise); refused beside sink tokens, beside a cap and on an fp8 cache before any library call."""
    fam = _KV_FAMILIES[family]
    packed = fam["packed"]
    window = _check_window(window, causal)
    sink = _check_sink(sink, window)
    softcap = _check_softcap(softcap)
    if softcap is not None and sink is not None:
        raise ValueError("softcap beside sink tokens is not built: softcap= with sink=")
    if sink_logits is not None and sink is not None:
        raise ValueError("sink_logits beside sink tokens is not built: sink_logits= with sink=")
    if sink_logits is not None and softcap is not None:
        raise ValueError("sink_logits beside a logit cap is not built: sink_logits= with softcap=")
    rotary = _rotary_of(rotary_cos, rotary_sin, rotary_interleaved, q.device)
    if rotary is None and q_rot is not None:
        raise ValueError("q_rot is where a roped call leaves the rotated q: it needs rotary_cos and rotary_sin")
    if (k_new is None) != (v_new is None):
        raise ValueError("k_new and v_new go together: give both (fused append) or neither")
    if layout not in _DECODE_LAYOUTS:
        raise ValueError(f"layout must be one of {sorted(_DECODE_LAYOUTS)}")
    if (packed and k_cache.dim() != 4) or k_cache.shape != v_cache.shape:
        raise ValueError(fam["caches"])
    dtype = _dtype_code(q)
    fp8 = _is_fp8(k_cache) or _is_fp8(v_cache)
    if k_cache.dtype != v_cache.dtype:
        raise TypeError("k_cache and v_cache must share one dtype" if fp8 else fam["kv_dtype"])
    if fp8:
        if not fam["fp8"]:
            raise TypeError(_RAGGED_FP8)
        if q.dtype != torch.bfloat16:
            raise TypeError("an fp8 cache takes bfloat16 queries")
        if window is not None:   # (sink tokens need a window, so this refuses them on an fp8 cache as well)
            raise ValueError("a sliding window on an fp8 cache is not built: window= with torch.float8_e4m3fn caches")
        if softcap is not None:
            raise ValueError("softcap on an fp8 cache is not built: softcap= with torch.float8_e4m3fn caches")
        if sink_logits is not None:
            raise ValueError("sink_logits on an fp8 cache is not built: sink_logits= with torch.float8_e4m3fn caches")
    elif k_cache.dtype != q.dtype:
        raise TypeError("q, k_cache and v_cache must share one dtype")
    mp = None if block_table is None else _max_pages(block_table, None)
    if max_pages is not None and max_pages != mp:   # (the caller's own figure, e.g. the one a workspace was sized with: held against the table)
        raise ValueError(f"max_pages = {max_pages} is not the block_table's second dimension ({mp}; a contiguous cache has none)")
    Hkv, dp, Ncap, pool, B, H, Nq, d = _kv_geometry(fam, k_cache, layout, mp, q, cu_seqlens_q)
    if d > dp:
        raise ValueError(f"q's head dim {d} exceeds the cache's row length {dp}")
    _check_scales(k_scale, v_scale, fp8, Hkv, q.device)
    _check_sink_logits(sink_logits, H, q.device)
    _check_seqlens(cache_seqlens, B, q.device)
    if pool:
        _check_table(block_table, B, q.device)
    d_new = dp
    if k_new is not None:
        _, d_new = _check_new(fam, k_new, v_new, k_cache, layout, Nq, Hkv, dp, None if pool else B)
        if not packed and k_new.shape[0] != B:
            raise ValueError(f"k_new holds {k_new.shape[0]} batch elements, q {B}")
    for t in (q, k_cache, v_cache):
        if t.device != q.device:
            raise ValueError("q, k_cache and v_cache must live on one device")
        if not t.is_contiguous():
            raise ValueError("q, k_cache and v_cache must be contiguous")
    if out is not None and (out.shape != q.shape or out.dtype != torch.float32 or not out.is_contiguous()):
        raise ValueError("out must be a contiguous float32 tensor of q's shape")
    lse_shape = (H, Nq) if packed else (B, H, Nq)
    if lse is not None and (tuple(lse.shape) != lse_shape or lse.dtype != torch.float32 or not lse.is_contiguous()):
        raise ValueError(f"lse must be a contiguous float32 tensor of shape {fam['lse']}")
    if workspace is not None and workspace.numel() * workspace.element_size() < _kv_workspace_bytes(fam, B, H, Hkv, Nq, Ncap, dp, window, sink):
        raise ValueError(f"workspace too small: size it with {fam['workspace']}()")
    _require_gpu(q, fam["attend"])   # (the caches live on q's device)
    if rotary:
        _check_rot(rotary, d, d_new if k_new is not None else None)
    if softmax_scale is None:
        softmax_scale = 0.0 if d == dp else d ** -0.5
    qp = pad_head_dim(q, dp) if d < dp else q
    qr = _q_rot_buffer(q_rot, q, qp) if rotary else None
    if out is not None and d == dp:
        outp = out
    elif out is not None and packed:   # (padded: the rows of the unused tail must come back as the caller's out held them)
        outp = pad_head_dim(out, dp)
    else:
        outp = torch.empty(qp.shape, dtype=torch.float32, device=q.device)
    if lse is None:
        lse = torch.empty(lse_shape, dtype=torch.float32, device=q.device)
    if workspace is None:
        nbytes = _kv_workspace_bytes(fam, B, H, Hkv, Nq, Ncap, dp, window, sink)
        if nbytes or not fam["workspace_none"]:
            workspace = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=q.device)
    num_pages, page_size, table_pages = pool or (0, 0, 0)
    fields = {   # what the family's entry points take, by the names of the prototypes (a paged cache goes without an Ncap).  Written
                 # out and not gathered in a loop: this is on the path of every launch-bound decode step.
        "q": qp.data_ptr(), "q_rot": None if qr is None else qr.data_ptr(), "k_new": None if k_new is None else k_new.data_ptr(),
        "v_new": None if v_new is None else v_new.data_ptr(), "k_cache": k_cache.data_ptr(), "v_cache": v_cache.data_ptr(),
        "k_scale": None if k_scale is None else k_scale.data_ptr(), "v_scale": None if v_scale is None else v_scale.data_ptr(),
        "out": outp.data_ptr(), "lse": lse.data_ptr(), "cu_seqlens_q": None if cu_seqlens_q is None else cu_seqlens_q.data_ptr(),
        "cache_seqlens": None if cache_seqlens is None else cache_seqlens.data_ptr(),
        "block_table": None if block_table is None else block_table.data_ptr(),
        "workspace": None if workspace is None else workspace.data_ptr(), "B": B, "H": H, "Hkv": Hkv, "Nq": Nq,
        "Ncap": 0 if pool else Ncap, "num_pages": num_pages, "page_size": page_size, "max_pages": table_pages, "d_new": d_new, "d": dp,
        "layout": _DECODE_LAYOUTS[layout], "softmax_scale": float(softmax_scale), "causal": int(bool(causal)),
        # (the softcap and lsink entry points take a window: 0 is none)
        "window": 0 if window is None and (softcap is not None or sink_logits is not None) else window,
        "sink": sink, "softcap": softcap, "sink_logits": None if sink_logits is None else sink_logits.data_ptr(), "dtype": dtype,
        "stream": _stream_ptr()}
    if rotary:   # (the roped append, then the attend-only form of whatever follows, on the rotated q)
        _rope_append(fam, fields, rotary, fp8)
        if q_rot is not None and qr is not q_rot:
            q_rot.copy_(qr[..., :d])
        fields.update(q=_ptr(qr), k_new=None, v_new=None, d_new=dp)
        k_new = None
    symbol = _kv_symbol(fam, "attend", pool is not None, k_new is not None, window, sink, fp8, Hkv == H, softcap, sink_logits is not None)
    _lib.decode_check(_kv_call(symbol, fields))
    return (_unpad(outp, d, out) if d < dp else outp), lse


def flash_attn_decode(q, k_cache, v_cache, cache_seqlens=None, causal=True, softmax_scale=None, layout="bnhd", out=None, lse=None,
                      workspace=None, k_new=None, v_new=None, block_table=None, window=None, k_scale=None, v_scale=None, sink=None,
                      rotary_cos=None, rotary_sin=None, rotary_interleaved=False, q_rot=None, softcap=None, sink_logits=None):
    """Attention of Nq <= 128 new queries against a KV cache (fa_mi355x_fwd_decode / _gqa, include/flash_attn_mi355x_decode.h).
    ``layout`` "bnhd": q (B, Nq, H, d), caches (B, Ncap, Hkv, dp); "bhnd": q (B, H, Nq, d), caches (B, Hkv, Ncap, dp).  Hkv is the
    cache's own head count and must divide H: Hkv < H is a grouped-query (Hkv = 1: multi-query) cache, query head h reads cache head
    h // (H // Hkv), and the group's heads share one pass over it (no expansion of the cache).  dp in {32, 64, 128};
    a q with fewer columns (d < dp) is zero-padded to the cache's row length (the cache itself holds zero columns d .. dp-1) and the
    default scale is then 1/sqrt(d).  ``cache_seqlens``: int32 (B,) on q's device, the valid cache rows per batch element counting the
    new tokens (None: all Ncap); clamped to [0, Ncap] on the device, no host synchronisation.  ``causal``: the queries are the last Nq
    positions.  ``k_new``, ``v_new`` (both or neither; shapes and placement as decode_append): the new tokens' k and v, written into
    the caches on the device in front of the attention (fa_mi355x_fwd_decode_append: decode_append, then this call, one library call).
    ``block_table`` (contiguous int32 (B, max_pages) on q's device): a PAGED cache.  k_cache and v_cache are then the pools,
    (num_pages, page_size, Hkv, dp) for "bnhd" or (num_pages, Hkv, page_size, dp) for "bhnd" with page_size a multiple of 128, cache
    row j of batch element b is row j % page_size of page block_table[b, j // page_size], Ncap = max_pages * page_size, and entries
    past a sequence's last page are never read (fa_mi355x_fwd_decode_paged; ids are clamped to the pool on the device).  The result
    is bit for bit the contiguous call's on the gathered cache; size a workspace with decode_workspace(..., block_table=).
    ``window`` (None, or an int >= 0; causal only): SLIDING-WINDOW attention (fa_mi355x_fwd_decode_window,
    include/flash_attn_mi355x_decode_window.h).  The query at position p admits the W keys p - W < j <= p, its own position
    included (Mistral's ``sliding_window``); lse covers the admitted keys.  The kernels start each row block's key range at its
    window, so the work and the bytes read follow W and not the cache's length, and cache rows (and the pages of a paged cache) wholly
    below the window are never read.  None takes the unwindowed entry points above; 0, and any W >= Ncap, is the unwindowed call
    through the windowed entry point (the same launches and bits).  Size a workspace with decode_workspace(..., window=).
    ``sink`` (None, or an int >= 0; needs ``window``): ATTENTION-SINK tokens (fa_mi355x_fwd_decode_sink,
    include/flash_attn_mi355x_decode_sink.h).  The first S positions of every sequence stay admitted beside the window: the query at
    p admits j <= p with j > p - W or j < S, a key in both counted once.  None and 0 take the paths above exactly; S >= Ncap, and
    window 0 or >= Ncap, is the unwindowed call.  A block reads ceil(S / 128) sink tiles beside its window's; the pages of a paged
    cache that hold the first S rows must stay.  Size a workspace with decode_workspace(..., window=, sink=).
    FP8 caches (k_cache and v_cache of dtype torch.float8_e4m3fn, slab or paged; fa_mi355x_fwd_decode_fp8,
    include/flash_attn_mi355x_decode_fp8.h): the caches hold e4m3 bytes and the value of an element of cache head h is
    scale[h] * e4m3, with ``k_scale`` / ``v_scale`` contiguous float32 (Hkv,) tensors on q's device (None: ones; read on the device).
    q, k_new and v_new are bfloat16; k_new / v_new are quantised as decode_append does.  Half the bytes per cached row; with
    power-of-two scales the result is bit for bit the bf16 call's on the cache cast to bfloat16 with softmax_scale * k_scale,
    times v_scale.  The workspace is the bf16 call's (decode_workspace takes the fp8 cache).  No ``window`` or ``sink`` on an fp8 cache, and
    scales with any other cache are an error.
    ``rotary_cos`` / ``rotary_sin`` (both or neither: contiguous float32 (max_pos, rot / 2) on q's device, rotary_table; rot even,
    <= d and <= d_new, max_pos >= Ncap): ROTARY position embeddings (include/flash_attn_mi355x_decode_rope.h).  One launch
    (fa_mi355x_rope_append) rotates q into ``q_rot`` (a contiguous tensor of q's shape and dtype, which may be q; None: allocated),
    rotates k_new on its way into the K cache and copies v_new into the V cache; the attention is then the ATTEND-ONLY form of
    whichever entry point the other arguments select, on q_rot.  New token i of batch element b, and its query, sit at position
    clamp(len_b, 0, Ncap) - Nq + i; ``rotary_interleaved`` picks GPT-J pairs (x[2j], x[2j+1]) instead of NeoX ones
    (x[j], x[j + rot/2]).  Bit for bit the call without the tables on apply_rotary(q) and apply_rotary(k_new) at those positions.
    Works with every cache feature above (paged, window, sink, fp8).  Without k_new / v_new only q is rotated.
    ``softcap`` (None, or a finite number >= 0): LOGIT SOFT-CAPPING (fa_mi355x_fwd_decode_softcap,
    include/flash_attn_mi355x_decode_softcap.h; Gemma-2's attn_logit_softcapping, Grok-1).  Every score becomes
    softcap * tanh(softmax_scale * q.k / softcap) before the masks and the softmax; lse is taken over the capped logits.  None and 0
    take the paths above exactly.  Works with a paged cache, a window (the one entry point takes both), the fused append, rotary
    tables and causal=False; beside ``sink`` and on an fp8 cache it is a ValueError (not built).  The workspace does not depend on
    the cap: decode_workspace(..., window=) sizes it.
    ``sink_logits`` (None, or a contiguous float32 (H,) tensor of FINITE values on q's device): LEARNED ATTENTION-SINK LOGITS
    (fa_mi355x_fwd_decode_lsink, include/flash_attn_mi355x_decode_lsink.h; gpt-oss's ``sinks``).  The logit a of a query head joins
    every row's softmax as one more column that has no value vector: lse = ln(e^a + sum_j e^z_j) over the admitted keys j,
    P_j = e^(z_j - lse), out = P . V, which is out0 * sigmoid(lse0 - a) and lse0 + softplus(a - lse0) of the call without it.  The
    logit is not scaled, not rotated and not masked.  The kernels read the tensor on the device, so a captured call replays with the
    values it holds then.  A row with no admissible key gives out = 0 and lse = a.  None takes the paths above exactly.  Works with
    a paged cache, a window, the fused append, rotary tables and causal=False, in as many launches as the call without it; beside
    ``sink``, beside ``softcap`` and on an fp8 cache it is a ValueError (not built).  The workspace does not depend on it.
    Returns (out fp32 in q's shape, lse fp32 (B, H, Nq)): rows with no admissible key give out = 0, lse = -inf."""
    return _kv_attention("decode", q, k_cache, v_cache, None, cache_seqlens, causal, softmax_scale, layout, out, lse, workspace, k_new, v_new,
                         block_table, None, window, k_scale, v_scale, sink, rotary_cos, rotary_sin, rotary_interleaved, q_rot, softcap,
                         sink_logits)


def flash_attn_extend(q, k_cache, v_cache, cache_seqlens=None, causal=True, softmax_scale=None, layout="bnhd", out=None, lse=None,
                      workspace=None, k_new=None, v_new=None, block_table=None, window=None, k_scale=None, v_scale=None, sink=None,
                      rotary_cos=None, rotary_sin=None, rotary_interleaved=False, q_rot=None, softcap=None, sink_logits=None):
    """flash_attn_decode for ANY number Nq >= 1 of new queries (fa_mi355x_fwd_extend / fa_mi355x_fwd_extend_append): a long input that
    follows a cached prefix, or one piece of a chunked prefill (the same call, from an empty cache on).  Every argument, check, the
    head-dim padding (the default scale keeps the caller's 1/sqrt(d)) and the return value are flash_attn_decode's; ``workspace`` is
    sized by extend_workspace (the extend call has its own split policy), ``k_new`` / ``v_new`` are appended as by extend_append.
    Always the extend kernels, whatever Nq: a workgroup owns 128 rows of a kv head's G * Nq and shares each staged K / V tile among
    them, and a causal call loads no tile above a block's last position.  For Nq <= 128 the result agrees with flash_attn_decode to
    rounding, not bit for bit.  ``block_table``: a paged cache, as in flash_attn_decode (fa_mi355x_fwd_extend_paged).  ``window``:
    sliding-window attention, as in flash_attn_decode (fa_mi355x_fwd_extend_window): every 128-row block walks its own W + 128
    positions' worth of keys wherever it sits in a long input; size a workspace with extend_workspace(..., window=).  ``k_scale`` /
    ``v_scale``: an fp8 cache, as in flash_attn_decode (fa_mi355x_fwd_extend_fp8).  ``sink``: attention-sink tokens beside the
    window, as in flash_attn_decode (fa_mi355x_fwd_extend_sink; extend_workspace(..., window=, sink=)).  ``rotary_cos`` /
    ``rotary_sin`` / ``rotary_interleaved`` / ``q_rot``: rotary embeddings, as in flash_attn_decode (fa_mi355x_rope_append, then the
    attend-only extend call on q_rot).  ``softcap``: logit soft-capping, as in flash_attn_decode (fa_mi355x_fwd_extend_softcap).
    ``sink_logits``: learned sink logits, as in flash_attn_decode (fa_mi355x_fwd_extend_lsink)."""
    return _kv_attention("extend", q, k_cache, v_cache, None, cache_seqlens, causal, softmax_scale, layout, out, lse, workspace, k_new, v_new,
                         block_table, None, window, k_scale, v_scale, sink, rotary_cos, rotary_sin, rotary_interleaved, q_rot, softcap,
                         sink_logits)


# ---- ragged batches: every sequence brings its own number of new tokens (include/flash_attn_mi355x_decode_ragged.h) ----

def _check_cu(cu_seqlens_q, B, device):
    if (not isinstance(cu_seqlens_q, torch.Tensor) or cu_seqlens_q.dtype != torch.int32 or cu_seqlens_q.dim() != 1
            or (B is not None and cu_seqlens_q.shape[0] != B + 1) or cu_seqlens_q.shape[0] < 2 or cu_seqlens_q.device != device
            or not cu_seqlens_q.is_contiguous()):
        raise ValueError("cu_seqlens_q must be a contiguous int32 tensor of shape (B + 1,) on q's device")


def ragged_workspace(q, k_cache, cu_seqlens_q, layout="bnhd", block_table=None, max_pages=None, window=None, sink=None):
    """Scratch for flash_attn_ragged with these tensors (fa_mi355x_ragged_workspace_bytes): the block map and one partial O, m, l per
    packed row and key chunk.  Never None: the map lives there, so every ragged call needs one.  A pure function of the SHAPES
    (cu_seqlens_q's contents are not read): allocate once, reuse every step.  A paged call (``k_cache`` the pool): give the block
    table or its ``max_pages``; the size is the contiguous call's for Ncap = max_pages * page_size.  ``window``: for
    flash_attn_ragged(..., window=) (fa_mi355x_ragged_window_workspace_bytes); ``sink``: for flash_attn_ragged(..., window=, sink=)
    (fa_mi355x_ragged_sink_workspace_bytes)."""
    return _kv_workspace("ragged", q, k_cache, cu_seqlens_q, layout, block_table, max_pages, window, sink)


def ragged_append(k_new, v_new, k_cache, v_cache, cu_seqlens_q, cache_seqlens=None, layout="bnhd", block_table=None, rotary_cos=None,
                  rotary_sin=None, rotary_interleaved=False, q_rot=None):
    """Write the packed new tokens' k and v into the caches on the device (fa_mi355x_ragged_append): k_new, v_new (T, Hkv, d_new),
    1 <= d_new <= dp, sequence b's rows cu_seqlens_q[b] .. cu_seqlens_q[b + 1] - 1 (clamped on the device so that no row leaves the
    buffers; a sequence may own none), into caches (B, Ncap, Hkv, dp) / (B, Hkv, Ncap, dp) (``layout`` names the caches' layout only:
    the packed buffers are token-major).  ``cache_seqlens`` COUNTS the new tokens: token i of sequence b goes to row
    clamp(len_b, 0, Ncap) - nq_b + i when that is >= 0, with zeros in columns d_new .. dp-1; every other cache row, and every packed
    row past the last sequence, is left alone.  In place, no host synchronisation.  ``block_table``: the caches are a paged cache's
    pools, as in decode_append.  ``rotary_cos`` / ``rotary_sin`` / ``rotary_interleaved``: k_new is rotated on its way into the K
    cache, as in decode_append (fa_mi355x_rope_append_ragged without a q; token i of sequence b at position
    clamp(len_b, 0, Ncap) - nq_b + i); ``q_rot`` must stay None."""
    _kv_append("ragged", k_new, v_new, k_cache, v_cache, cu_seqlens_q, cache_seqlens, layout, block_table, None, None, rotary_cos, rotary_sin,
               rotary_interleaved, q_rot)


def flash_attn_ragged(q, k_cache, v_cache, cu_seqlens_q, cache_seqlens=None, causal=True, softmax_scale=None, layout="bnhd", out=None,
                      lse=None, workspace=None, k_new=None, v_new=None, block_table=None, max_pages=None, window=None, sink=None,
                      rotary_cos=None, rotary_sin=None, rotary_interleaved=False, q_rot=None, softcap=None, sink_logits=None):
    """One attention call over a RAGGED batch (fa_mi355x_fwd_ragged / _fwd_ragged_append and their _paged forms): every sequence
    brings its own number of new tokens -- some decode one, one is part-way through a chunked prefill, some have none.  ``q`` is
    PACKED, (T, H, d): sequence b owns rows cu_seqlens_q[b] .. cu_seqlens_q[b + 1] - 1 (``cu_seqlens_q`` contiguous int32 (B + 1,) on
    q's device, read and clamped on the device: no host synchronisation, no access outside the T rows whatever it holds; T may exceed
    cu_seqlens_q[B], the rows past it are the unused tail of a fixed-capacity buffer and are neither read nor written).  The caches,
    ``cache_seqlens`` (counting the new tokens), ``causal`` (token i of sequence b sits at len_b - nq_b + i), the head-dim padding
    and the default scale are flash_attn_extend's; ``layout`` names the caches' layout only.  ``k_new``, ``v_new`` (both or neither,
    (T, Hkv, d_new) packed like q): appended as by ragged_append in front of the attention, one library call.  ``block_table``: a
    paged cache, as in flash_attn_decode; ``max_pages``, when given, must be the table's second dimension (the figure a workspace
    was sized with through ragged_workspace(..., max_pages=): a mismatch is an error here, not a workspace of the wrong size).
    ``workspace``: from ragged_workspace (always needed: it holds the block map).  Per sequence the result is flash_attn_extend's
    on that sequence alone (bit for bit where both run as one split).  A step in which EVERY sequence decodes one token is faster
    through flash_attn_decode (measured, profiles/ragged_bench.txt: 1.10x in bf16, 2.4x in fp32 at B = 32, length 4096).
    ``window``: sliding-window attention, as in flash_attn_decode (fa_mi355x_fwd_ragged_window; token i of sequence b sits at
    len_b - nq_b + i and admits the W keys up to its own position); size a workspace with ragged_workspace(..., window=).
    ``sink``: attention-sink tokens beside the window, as in flash_attn_decode (fa_mi355x_fwd_ragged_sink: the first S positions of
    each sequence; ragged_workspace(..., window=, sink=)).
    ``rotary_cos`` / ``rotary_sin`` / ``rotary_interleaved`` / ``q_rot``: rotary embeddings, as in flash_attn_decode
    (fa_mi355x_rope_append_ragged, then the attend-only ragged call on q_rot; token i of sequence b sits at
    clamp(len_b, 0, Ncap) - nq_b + i; the rows of q_rot that no sequence owns keep what they held).
    ``softcap``: logit soft-capping, as in flash_attn_decode (fa_mi355x_fwd_ragged_softcap).
    ``sink_logits``: learned sink logits, as in flash_attn_decode (fa_mi355x_fwd_ragged_lsink); a sequence's row with no admissible
    key gives out = 0 and lse = its head's logit.
    Returns (out fp32 (T, H, d), lse fp32 (H, T)): rows with no admissible key give out = 0, lse = -inf; rows of the unused tail
    keep what they held."""
    return _kv_attention("ragged", q, k_cache, v_cache, cu_seqlens_q, cache_seqlens, causal, softmax_scale, layout, out, lse, workspace, k_new,
                         v_new, block_table, max_pages, window, None, None, sink, rotary_cos, rotary_sin, rotary_interleaved, q_rot, softcap,
                         sink_logits)


# ---- packed variable-length batches in the training forward and backward (include/flash_attn_mi355x_varlen.h) ----------------------
# q (T, H, d), k and v (T, Hkv, d), token-major as in the ragged calls above; sequence b owns the packed rows cu_seqlens[b] ..
# cu_seqlens[b + 1] - 1 (clamped on the device; never read on the host).  Row i of a sequence sits at position i and admits key j of
# the same sequence iff j <= i and (j > i - W or j < S).  Causal only.  The kernels are the window library's, run per (sequence,
# block) off a device-side block map (libflash_attn_mi355x_varlen.so): per sequence the result is, bit for bit,
# flash_attn_fwd_window / flash_attn_bwd_window on that sequence alone.  Rows no sequence owns come back as zeros.

def _check_packed(q, k, v, cu_q, cu_k, o=None, do=None, *, one_array, wrapper):
    """What _check_gqa checks, for packed 3-d tensors.  ``one_array``: the causal packed calls, where one cu_seqlens serves queries
    and keys and q and k agree on (T, d); otherwise the two-array ones (bidirectional, or causal behind a prefix), with a row count and
    an array for either side.  ``wrapper``: the public call that pads the head dim, for the message.  Returns (nseq, Tq, Tk, H, Hkv,
    d, dtype code)."""
    tq, tk = ("T", "T") if one_array else ("Tq", "Tk")
    _require_gpu(q, "device_ops")
    dtype = _dtype_code(q)
    if q.dim() != 3 or k.dim() != 3:
        raise ValueError(f"expected packed 3-d tensors: q ({tq}, H, d) and k, v ({tk}, Hkv, d)")
    dev = q.get_device()
    if v.shape != k.shape:
        raise ValueError("k and v must have one shape")
    for t in (k, v):
        if not t.is_cuda or t.dtype != q.dtype or t.get_device() != dev:
            raise ValueError("q, k, v must be GPU tensors of one dtype on one device")
    (Tq, H, d), (Tk, Hkv, dk) = q.shape, k.shape
    if one_array:
        if (Tq, d) != (Tk, dk):
            raise ValueError(f"q and k disagree on (T, d): {(Tq, d)} vs {(Tk, dk)} (one cu_seqlens serves queries and keys)")
        if Tq < 1:
            raise ValueError("the packed batch is empty: T must be at least 1")
    else:
        if d != dk:
            raise ValueError(f"q and k disagree on the head dim: {d} vs {dk}")
        if Tq < 1 or Tk < 1:
            raise ValueError("the packed batch is empty: Tq and Tk must be at least 1")
    if Hkv <= 0 or H % Hkv:
        raise ValueError(f"q's {H} heads must be a multiple of k's {Hkv}")
    if d not in _NATIVE_D:
        raise ValueError(f"the packed calls need a native head dim (32, 64, 128): {wrapper} pads, or pad q, k and v "
                         "(pad_head_dim) and pass softmax_scale")
    _check_cu(cu_q, None, q.device)
    if cu_k is not cu_q:
        _check_cu(cu_k, None, q.device)
        if cu_k.shape != cu_q.shape:
            raise ValueError("cu_seqlens_q and cu_seqlens_k must have one length: the same sequences, counted in q and in k")
    if do is not None and (do.shape != q.shape or do.dtype != q.dtype or do.get_device() != dev):
        raise ValueError("out_grad must share q's shape, dtype and device")
    for t in (q, k, v) + ((do,) if do is not None else ()):
        if not t.is_contiguous():
            raise ValueError("tensors must be contiguous")
    if o is not None and (o.dtype is not _F32 or o.shape != q.shape or not o.is_contiguous() or o.get_device() != dev):
        raise ValueError("out must be the forward's contiguous float32 output")
    return cu_q.shape[0] - 1, Tq, Tk, H, Hkv, d, dtype


def _check_varlen_mask(window, sink):
    """(W, S) as the packed entry points take them: 0 for None (no window: every j <= i); a sink needs a window."""
    window = _check_window(window)
    sink = _check_sink(sink, window)
    if sink and not window:
        raise ValueError("sink tokens stand beside a sliding window: sink= needs window >= 1")
    return window or 0, sink or 0


def varlen_workspace(q, k, cu_seqlens, backward=True):
    """Scratch for flash_attn_varlen_bwd (``backward=False``: for flash_attn_varlen_fwd alone) with these tensors
    (fa_mi355x_bwd_varlen_workspace_bytes / _fwd_): the block maps, the row constants and, when k has fewer heads than q, the dK and
    dV of every query head.  Never empty: the maps live there.  A pure function of the SHAPES (cu_seqlens's contents are not read):
    allocate once, reuse every step.  A backward workspace also serves the forward."""
    return _side_workspace("varlen", q, k, (cu_seqlens,), backward=backward)


def flash_attn_varlen_fwd(q, k, v, cu_seqlens, window=None, sink=None, softmax_scale=None, out=None, workspace=None, lse=None):
    """Causal forward over a packed batch (fa_mi355x_fwd_varlen): q (T, H, d), k and v (T, Hkv, d), ``cu_seqlens`` contiguous int32
    (nseq + 1,) on q's device.  ``window`` = W, ``sink`` = S: the sliding-window mask within every sequence (None or 0: none).
    Returns (out fp32 (T, H, d), lse (H, T)); rows no sequence owns are zero in both.  ``out``, ``lse``: buffers to write into;
    ``workspace``: varlen_workspace(q, k, cu_seqlens) (with all three given the call allocates nothing: it can be captured in a graph)."""
    mask = _check_varlen_mask(window, sink)
    return _side_fwd("varlen", q, k, v, (cu_seqlens,), mask, softmax_scale, out=out, lse=lse, workspace=workspace)


def flash_attn_varlen_bwd(q, k, v, out, out_grad, lse, cu_seqlens, window=None, sink=None, softmax_scale=None, workspace=None, grads=None):
    """Backward of flash_attn_varlen_fwd (fa_mi355x_bwd_varlen).  Returns (dq in q's shape, dk, dv in k's shape), fp32, zero in the
    rows no sequence owns; no atomics, the same bits on every run.  ``workspace``: varlen_workspace(q, k, cu_seqlens); ``grads``:
    (dq, dk, dv) buffers to write into."""
    mask = _check_varlen_mask(window, sink)
    return _side_bwd("varlen", q, k, v, out, out_grad, lse, (cu_seqlens,), mask, softmax_scale, workspace=workspace, grads=grads)


def flash_attn_varlen(q, k, v, cu_seqlens, causal=True, softmax_scale=None, window=None, sink=None):
    """Causal attention over a packed batch of sequences of different lengths, under autograd: q (T, H, d), k and v (T, Hkv, d),
    ``cu_seqlens`` int32 (nseq + 1,) on q's device.  out fp32 (T, H, d); q.grad in q's shape and dtype, k.grad and v.grad in k's.
    ``window``, ``sink``: as flash_attn_gqa, within every sequence.  A head dim other than 32, 64, 128 runs through zero-padded
    columns with softmax_scale = 1 / sqrt(d).  Rows no sequence owns give zeros and take a zero gradient."""
    if not causal:
        raise ValueError("non-causal packed attention is not built: flash_attn_varlen is causal only (causal=False); "
                         "flash_attn_varlen_bidir is the bidirectional packed call")
    window, sink = _check_varlen_mask(window, sink)
    return _native_head_dim(q, k, v, softmax_scale, lambda q, k, v, scale: _FlashAttnSideFn.apply(
        flash_attn_varlen_fwd, flash_attn_varlen_bwd, q, k, v, (cu_seqlens,), dict(window=window, sink=sink, softmax_scale=scale)))


def _rotary_varlen_call(x, y, cos, sin, cu_seqlens, interleaved, inverse):
    T, H, d = x.shape
    rot, max_pos, il = _check_rotary(cos, sin, x.device, interleaved)
    _lib.varlen_check(_lib.varlen().fa_mi355x_rope_varlen(
        _ptr(x), _ptr(y), _ptr(cos), _ptr(sin), _ptr(cu_seqlens), cu_seqlens.shape[0] - 1, T, H, d, rot, max_pos, il, int(bool(inverse)),
        _dtype_code(x), _stream_ptr()))
    return y


class _RotaryVarlenFn(torch.autograd.Function):
    """apply_rotary_varlen under autograd: as _RotaryFn, the gradient is the inverse rotation of the cotangent."""

    @staticmethod
    def forward(ctx, x, cos, sin, cu_seqlens, interleaved, inverse, out):
        ctx.save_for_backward(cos, sin, cu_seqlens)
        ctx.how = (interleaved, inverse)
        if out is None:
            out = torch.empty_like(x)
        else:
            ctx.mark_dirty(out)
        return _rotary_varlen_call(x, out, cos, sin, cu_seqlens, interleaved, inverse)

    @staticmethod
    def backward(ctx, g):
        cos, sin, cu_seqlens = ctx.saved_tensors
        interleaved, inverse = ctx.how
        g = g.contiguous()
        return _rotary_varlen_call(g, torch.empty_like(g), cos, sin, cu_seqlens, interleaved, not inverse), None, None, None, None, None, None


def apply_rotary_varlen(x, cos, sin, cu_seqlens, interleaved=False, inverse=False, out=None):
    """Rotary position embedding of a packed tensor (fa_mi355x_rope_varlen): x (T, H, d), float32 or bfloat16, contiguous; packed
    row t of sequence b sits at position t - cu_seqlens[b], so positions restart at every sequence (clamped to the table on the
    device); a row no sequence owns is copied.  Tables, pairs, arithmetic, ``inverse`` and ``out`` as apply_rotary: per sequence the
    result is apply_rotary's on that sequence alone, bit for bit.  Differentiable in x by the inverse rotation."""
    if not isinstance(x, torch.Tensor) or x.dim() != 3:
        raise ValueError("apply_rotary_varlen expects a packed 3-d x, (T, H, d)")
    _dtype_code(x)
    rot = _check_rotary(cos, sin, x.device)
    if rot is None:
        raise ValueError("apply_rotary_varlen needs both tables, cos and sin")
    if rot[0] > x.shape[2]:
        raise ValueError(f"the tables' rotary dimension {rot[0]} exceeds x's head dim {x.shape[2]}")
    _check_cu(cu_seqlens, None, x.device)
    if not x.is_contiguous():
        raise ValueError("x must be contiguous")
    if out is not None and (out.shape != x.shape or out.dtype != x.dtype or out.device != x.device or not out.is_contiguous()):
        raise ValueError("out must be a contiguous tensor of x's shape, dtype and device")
    _require_gpu(x, "apply_rotary_varlen")
    return _RotaryVarlenFn.apply(x, cos, sin, cu_seqlens, bool(interleaved), bool(inverse), out)


# ---- bidirectional packed attention with one cu_seqlens for q and one for k (include/flash_attn_mi355x_bidir.h) ---------------------
# q (Tq, H, d), k and v (Tk, Hkv, d); sequence b owns the rows cu_seqlens_q[b] .. cu_seqlens_q[b + 1] - 1 of q and the rows
# cu_seqlens_k[b] .. cu_seqlens_k[b + 1] - 1 of k and v (each clamped on the device against its own T; never read on the host), and
# every query of a sequence admits every key of it: encoders on packed documents (one array for both) and cross-attention.  Kernels
# of their own (libflash_attn_mi355x_bidir.so).  Query rows of a keyless sequence and rows no sequence owns come back as zeros.

def _self_cu(q, k, cu_seqlens_q, cu_seqlens_k):
    """cu_seqlens_k=None: self-attention, one array for both buffers, and k has q's rows."""
    if cu_seqlens_k is not None:
        return cu_seqlens_k
    if isinstance(q, torch.Tensor) and isinstance(k, torch.Tensor) and q.dim() == 3 and k.dim() == 3 and q.shape[0] != k.shape[0]:
        raise ValueError(f"cu_seqlens_k=None means self-attention: k must have q's {q.shape[0]} rows, not {k.shape[0]}")
    return cu_seqlens_q


def bidir_workspace(q, k, cu_seqlens_q, cu_seqlens_k=None, backward=True):
    """Scratch for flash_attn_varlen_bidir_bwd (``backward=False``: for flash_attn_varlen_bidir_fwd alone) with these tensors
    (fa_mi355x_bwd_bidir_workspace_bytes / _fwd_): the two block maps, the row constants and, when k has fewer heads than q, the dK
    and dV of every query head.  Never empty: the maps live there.  A pure function of the SHAPES (the arrays' contents are not
    read): allocate once, reuse every step.  A backward workspace also serves the forward."""
    return _side_workspace("bidir", q, k, (cu_seqlens_q, _self_cu(q, k, cu_seqlens_q, cu_seqlens_k)), backward=backward)


def flash_attn_varlen_bidir_fwd(q, k, v, cu_seqlens_q, cu_seqlens_k=None, softmax_scale=None, out=None, workspace=None, lse=None):
    """Bidirectional forward over a packed batch (fa_mi355x_fwd_bidir): q (Tq, H, d), k and v (Tk, Hkv, d), the two arrays contiguous
    int32 (nseq + 1,) on q's device (``cu_seqlens_k=None``: self-attention, the same array).  Returns (out fp32 (Tq, H, d), lse
    (H, Tq)); query rows of a keyless sequence and rows no sequence owns are zero in both.  ``out``, ``lse``: buffers to write into;
    ``workspace``: bidir_workspace(...) (with all three given the call allocates nothing: it can be captured in a graph)."""
    index = (cu_seqlens_q, _self_cu(q, k, cu_seqlens_q, cu_seqlens_k))
    return _side_fwd("bidir", q, k, v, index, (), softmax_scale, out=out, lse=lse, workspace=workspace)


def flash_attn_varlen_bidir_bwd(q, k, v, out, out_grad, lse, cu_seqlens_q, cu_seqlens_k=None, softmax_scale=None, workspace=None,
                                grads=None):
    """Backward of flash_attn_varlen_bidir_fwd (fa_mi355x_bwd_bidir).  Returns (dq in q's shape, dk, dv in k's shape), fp32; zero in
    the query rows of a keyless sequence, the key rows of a sequence without queries and the rows no sequence owns; no atomics, the
    same bits on every run.  ``workspace``: bidir_workspace(...); ``grads``: (dq, dk, dv) buffers to write into."""
    index = (cu_seqlens_q, _self_cu(q, k, cu_seqlens_q, cu_seqlens_k))
    return _side_bwd("bidir", q, k, v, out, out_grad, lse, index, (), softmax_scale, workspace=workspace, grads=grads)


def flash_attn_varlen_bidir(q, k, v, cu_seqlens_q, cu_seqlens_k=None, softmax_scale=None):
    """Bidirectional attention over a packed batch, under autograd: q (Tq, H, d), k and v (Tk, Hkv, d); sequence b's queries
    (``cu_seqlens_q``) admit every key of sequence b (``cu_seqlens_k``; None: self-attention, the same array, and k has Tq rows).
    out fp32 (Tq, H, d); q.grad in q's shape and dtype, k.grad and v.grad in k's.  A head dim other than 32, 64, 128 runs through
    zero-padded columns with softmax_scale = 1 / sqrt(d).  Query rows of a keyless sequence and rows no sequence owns give zeros and
    take a zero gradient."""
    index = (cu_seqlens_q, _self_cu(q, k, cu_seqlens_q, cu_seqlens_k))
    return _native_head_dim(q, k, v, softmax_scale, lambda q, k, v, scale: _FlashAttnSideFn.apply(
        flash_attn_varlen_bidir_fwd, flash_attn_varlen_bidir_bwd, q, k, v, index, dict(softmax_scale=scale)))


def _batched_two_array(name, attend, q, k, v, softmax_scale):
    """``attend`` (a packed two-array call under autograd) on batched tensors: q (B, Nq, H, d), k and v (B, Nk, Hkv, d) are viewed as
    packed ((B * Nq, H, d), (B * Nk, Hkv, d)) and the two cu_seqlens are built on the device.  out fp32 (B, Nq, H, d)."""
    if not isinstance(q, torch.Tensor) or not isinstance(k, torch.Tensor) or not isinstance(v, torch.Tensor) or q.dim() != 4 or k.dim() != 4:
        raise ValueError(f"{name} expects 4-d tensors: q (B, Nq, H, d) and k, v (B, Nk, Hkv, d)")
    if v.shape != k.shape:
        raise ValueError("k and v must have one shape")
    (B, Nq, H, d), (Bk, Nk, Hkv, _) = q.shape, k.shape
    if B != Bk:
        raise ValueError(f"q and k disagree on the batch: {B} vs {Bk}")
    if not (q.is_contiguous() and k.is_contiguous() and v.is_contiguous()):
        raise ValueError("tensors must be contiguous")
    steps = torch.arange(B + 1, dtype=torch.int32, device=q.device)
    cu_q, cu_k = steps * Nq, steps * Nk
    o = attend(q.view(B * Nq, H, d), k.view(B * Nk, Hkv, d), v.view(B * Nk, Hkv, d), cu_q, cu_k, softmax_scale)
    return o.view(B, Nq, H, o.shape[-1])


def flash_attn_cross(q, k, v, softmax_scale=None):
    """Batched cross-attention under autograd: q (B, Nq, H, d), k and v (B, Nk, Hkv, d), contiguous; every query of batch element b
    admits every key of it, Nq and Nk independent.  The tensors are viewed as packed ((B * Nq, H, d), (B * Nk, Hkv, d)) and the two
    cu_seqlens are built on the device: flash_attn_varlen_bidir does the rest.  out fp32 (B, Nq, H, d)."""
    return _batched_two_array("flash_attn_cross", flash_attn_varlen_bidir, q, k, v, softmax_scale)


# ---- causal packed attention with one cu_seqlens for q and one for k: a cached prefix (include/flash_attn_mi355x_prefix.h) ----------
# The tensors and the two arrays of the bidirectional calls above; the queries of sequence b are the LAST n_q positions of its n_k
# keys, so with D = n_k - n_q row i admits the keys 0 .. i + D (the bottom-right alignment of flash-attn >= 2.1, the mask
# flash_attn_extend generates with).  Kernels of their own (libflash_attn_mi355x_prefix.so).  Rows that admit no key (i + D < 0, a
# keyless sequence) and rows no sequence owns come back as zeros.

def prefix_workspace(q, k, cu_seqlens_q, cu_seqlens_k=None, backward=True):
    """Scratch for flash_attn_varlen_prefix_bwd (``backward=False``: for flash_attn_varlen_prefix_fwd alone) with these tensors
    (fa_mi355x_bwd_prefix_workspace_bytes / _fwd_): as bidir_workspace, a pure function of the SHAPES."""
    return _side_workspace("prefix", q, k, (cu_seqlens_q, _self_cu(q, k, cu_seqlens_q, cu_seqlens_k)), backward=backward)


def flash_attn_varlen_prefix_fwd(q, k, v, cu_seqlens_q, cu_seqlens_k=None, softmax_scale=None, out=None, workspace=None, lse=None):
    """Causal forward over a packed batch whose sequences have n_q queries behind n_k - n_q earlier keys (fa_mi355x_fwd_prefix): q
    (Tq, H, d), k and v (Tk, Hkv, d), the two arrays contiguous int32 (nseq + 1,) on q's device (``cu_seqlens_k=None``: causal
    self-attention, the same array).  Returns (out fp32 (Tq, H, d), lse (H, Tq)); rows that admit no key and rows no sequence owns
    are zero in both.  ``out``, ``lse``: buffers to write into; ``workspace``: prefix_workspace(...) (with all three given the call
    allocates nothing: it can be captured in a graph)."""
    index = (cu_seqlens_q, _self_cu(q, k, cu_seqlens_q, cu_seqlens_k))
    return _side_fwd("prefix", q, k, v, index, (), softmax_scale, out=out, lse=lse, workspace=workspace)


def flash_attn_varlen_prefix_bwd(q, k, v, out, out_grad, lse, cu_seqlens_q, cu_seqlens_k=None, softmax_scale=None, workspace=None,
                                 grads=None):
    """Backward of flash_attn_varlen_prefix_fwd (fa_mi355x_bwd_prefix).  Returns (dq in q's shape, dk, dv in k's shape), fp32; zero in
    the query rows that admit no key, the key rows of a sequence without queries and the rows no sequence owns; no atomics, the same
    bits on every run.  ``workspace``: prefix_workspace(...); ``grads``: (dq, dk, dv) buffers to write into."""
    index = (cu_seqlens_q, _self_cu(q, k, cu_seqlens_q, cu_seqlens_k))
    return _side_bwd("prefix", q, k, v, out, out_grad, lse, index, (), softmax_scale, workspace=workspace, grads=grads)


def flash_attn_varlen_prefix(q, k, v, cu_seqlens_q, cu_seqlens_k=None, softmax_scale=None):
    """Causal attention over a packed batch with a cached prefix, under autograd: q (Tq, H, d), k and v (Tk, Hkv, d); sequence b's
    queries (``cu_seqlens_q``) are the last positions of sequence b's keys (``cu_seqlens_k``; None: causal self-attention, the same
    array, and k has Tq rows), and row i admits the keys 0 .. i + n_k - n_q.  out fp32 (Tq, H, d); q.grad in q's shape and dtype,
    k.grad and v.grad in k's, the prefix rows included.  A head dim other than 32, 64, 128 runs through zero-padded columns with
    softmax_scale = 1 / sqrt(d).  Rows that admit no key and rows no sequence owns give zeros and take a zero gradient."""
    index = (cu_seqlens_q, _self_cu(q, k, cu_seqlens_q, cu_seqlens_k))
    return _native_head_dim(q, k, v, softmax_scale, lambda q, k, v, scale: _FlashAttnSideFn.apply(
        flash_attn_varlen_prefix_fwd, flash_attn_varlen_prefix_bwd, q, k, v, index, dict(softmax_scale=scale)))


def flash_attn_prefix(q, k, v, softmax_scale=None):
    """Batched causal attention behind a prefix, under autograd: q (B, Nq, H, d) are the last Nq positions of k and v (B, Nk, Hkv, d),
    contiguous: the differentiable counterpart of flash_attn_extend on a slab cache that holds the same keys.  Built as
    flash_attn_cross, over flash_attn_varlen_prefix.  out fp32 (B, Nq, H, d)."""
    return _batched_two_array("flash_attn_prefix", flash_attn_varlen_prefix, q, k, v, softmax_scale)


# ---- packed attention under a two-sided sliding window, a band (include/flash_attn_mi355x_local.h) ---------------------------------
# The tensors, the two arrays and the bottom-right alignment of the causal calls above: row i of a sequence sits at key position
# p = i + n_k - n_q and, under window = (L, R), admits the keys max(0, p - L) .. min(n_k - 1, p + R); a side of -1 (or None) is
# unbounded.  Kernels of their own (libflash_attn_mi355x_local.so), which walk only the tiles that meet the band.  (-1, -1) IS the
# bidirectional call and (-1, 0) the causal one: those two windows go to the functions above, launches and bits unchanged.  Rows that
# admit no key, keys no row admits and rows no sequence owns come back as zeros.

def _check_band(window):
    """``window`` of the banded calls as the library takes it: (left, right), each an int >= -1 (None, for a side or for the pair:
    -1, unbounded)."""
    if window is None:
        return -1, -1
    sides = None
    if not isinstance(window, (str, bytes, torch.Tensor)):
        try:
            sides = tuple(window)
        except TypeError:
            sides = None
    if sides is None or len(sides) != 2:
        raise ValueError("window must be a pair (left, right): the positions a token sees before and behind its own, each an int >= -1 "
                         "(-1 or None: unbounded)")
    pair = []
    for side in sides:
        if side is None:
            side = -1
        try:
            side = None if isinstance(side, bool) else operator.index(side)
        except TypeError:
            side = None
        if side is None or side < -1:
            raise ValueError("window must be a pair (left, right) of ints >= -1 (-1 or None: unbounded on that side)")
        pair.append(side)
    return tuple(pair)


_BAND_ROUTES = {(-1, -1): "bidir", (-1, 0): "prefix"}   # the windows that are an existing call


def local_workspace(q, k, cu_seqlens_q, cu_seqlens_k=None, backward=True):
    """Scratch for flash_attn_varlen_local_bwd (``backward=False``: for flash_attn_varlen_local_fwd alone) with these tensors
    (fa_mi355x_bwd_local_workspace_bytes / _fwd_): as bidir_workspace, a pure function of the SHAPES, the same for every window (the
    sizes are those of bidir_workspace and prefix_workspace, so it also serves the two windows that run as those calls)."""
    return _side_workspace("local", q, k, (cu_seqlens_q, _self_cu(q, k, cu_seqlens_q, cu_seqlens_k)), backward=backward)


def flash_attn_varlen_local_fwd(q, k, v, cu_seqlens_q, cu_seqlens_k=None, window=(-1, -1), softmax_scale=None, out=None, workspace=None,
                                lse=None):
    """Forward under a two-sided sliding window over a packed batch (fa_mi355x_fwd_local): q (Tq, H, d), k and v (Tk, Hkv, d), the two
    arrays contiguous int32 (nseq + 1,) on q's device (``cu_seqlens_k=None``: self-attention, the same array); ``window`` = (left,
    right), ints >= -1.  Returns (out fp32 (Tq, H, d), lse (H, Tq)); rows that admit no key and rows no sequence owns are zero in
    both.  (-1, -1) is flash_attn_varlen_bidir_fwd and (-1, 0) flash_attn_varlen_prefix_fwd, and runs as them.  ``out``, ``lse``:
    buffers to write into; ``workspace``: local_workspace(...) (with all three given the call allocates nothing: it can be captured
    in a graph)."""
    window = _check_band(window)
    index = (cu_seqlens_q, _self_cu(q, k, cu_seqlens_q, cu_seqlens_k))
    family = _BAND_ROUTES.get(window, "local")
    return _side_fwd(family, q, k, v, index, window if family == "local" else (), softmax_scale, out=out, lse=lse, workspace=workspace)


def flash_attn_varlen_local_bwd(q, k, v, out, out_grad, lse, cu_seqlens_q, cu_seqlens_k=None, window=(-1, -1), softmax_scale=None,
                                workspace=None, grads=None):
    """Backward of flash_attn_varlen_local_fwd (fa_mi355x_bwd_local) under the same ``window``.  Returns (dq in q's shape, dk, dv in
    k's shape), fp32; zero in the query rows that admit no key, the key rows no query admits and the rows no sequence owns; no
    atomics, the same bits on every run.  ``workspace``: local_workspace(...); ``grads``: (dq, dk, dv) buffers to write into."""
    window = _check_band(window)
    index = (cu_seqlens_q, _self_cu(q, k, cu_seqlens_q, cu_seqlens_k))
    family = _BAND_ROUTES.get(window, "local")
    return _side_bwd(family, q, k, v, out, out_grad, lse, index, window if family == "local" else (), softmax_scale,
                     workspace=workspace, grads=grads)


def flash_attn_varlen_local(q, k, v, cu_seqlens_q, cu_seqlens_k=None, window=(-1, -1), softmax_scale=None):
    """Attention under a two-sided sliding window over a packed batch, under autograd: q (Tq, H, d), k and v (Tk, Hkv, d); sequence
    b's queries (``cu_seqlens_q``) are the last positions of sequence b's keys (``cu_seqlens_k``; None: self-attention, the same
    array, and k has Tq rows), and the row at position p admits the keys p - left .. p + right of its sequence (``window`` = (left,
    right), ints >= -1; -1 or None: unbounded on that side).  out fp32 (Tq, H, d); q.grad in q's shape and dtype, k.grad and v.grad
    in k's.  A head dim other than 32, 64, 128 runs through zero-padded columns with softmax_scale = 1 / sqrt(d).  Rows that admit no
    key and rows no sequence owns give zeros and take a zero gradient.  (-1, -1) is flash_attn_varlen_bidir and (-1, 0)
    flash_attn_varlen_prefix: the same launches and bits."""
    window = _check_band(window)
    index = (cu_seqlens_q, _self_cu(q, k, cu_seqlens_q, cu_seqlens_k))
    return _native_head_dim(q, k, v, softmax_scale, lambda q, k, v, scale: _FlashAttnSideFn.apply(
        flash_attn_varlen_local_fwd, flash_attn_varlen_local_bwd, q, k, v, index, dict(window=window, softmax_scale=scale)))


def flash_attn_local(q, k, v, window, softmax_scale=None):
    """Batched attention under a two-sided sliding window, under autograd: q (B, Nq, H, d) are the last Nq positions of k and v
    (B, Nk, Hkv, d), contiguous; ``window`` = (left, right) as flash_attn_varlen_local.  Built as flash_attn_cross, over
    flash_attn_varlen_local.  out fp32 (B, Nq, H, d)."""
    window = _check_band(window)
    return _batched_two_array("flash_attn_local", lambda q, k, v, cu_q, cu_k, scale: flash_attn_varlen_local(
        q, k, v, cu_q, cu_k, window, scale), q, k, v, softmax_scale)
