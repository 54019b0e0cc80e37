"""MLA prefill without a GPU (include/flash_attn_mi355x_mla_prefill.h, csrc/fa_mla_prefill.h): the fp64 reference, the C ABI against
the header, every refusal in front of a HIP call, the Python checks, the workspace law, the kernels' registers, and the inputs of
tests/test_gpu_mla_prefill.py, which must tell a right kernel from one that drops k_pe and from one that aligns the mask top-left."""
import functools
import re

import numpy as np
import pytest
import torch

from test_abi_cpu import _device_kernels
from test_decode_cpu import built  # noqa: F401  (the module-scoped build fixture)

HEADER = "flash_attn_mi355x_mla_prefill.h"
TOL, SCALE, BAD_ARG = 1e-3, 192 ** -0.5, 1   # TOL: the project's bf16 figure, max-abs on out and lse
# The packed batches of the GPU tests: rows in front of sequence 0 that no sequence owns, then (n_q, n_k) per sequence.  A is
# self-attention (one array: D = 0 throughout), B a prefix behind every sequence (D > 0), C more queries than keys and empty sides.
CASES = {"A": (1, ((1, 1), (63, 63), (129, 129), (0, 0), (200, 200))), "B": (0, ((1, 300), (65, 129), (128, 192), (3, 64))),
         "C": (0, ((70, 5), (5, 0), (130, 130)))}


@functools.lru_cache(maxsize=None)
def inputs(case, H, seed=5):
    """q (Tq, H, 192), kv (Tk, H, 256) = k_nope | v per head, k_pe (Tk, 64): U(-1, 1) rounded to bf16; cu_q, cu_k int32."""
    lead, lens = CASES[case]
    cu_q, cu_k = (torch.tensor(np.concatenate([[0], np.cumsum([n[s] for n in lens])]) + lead, dtype=torch.int32) for s in (0, 1))
    g = torch.Generator().manual_seed(seed)
    u = lambda *shape: (torch.rand(*shape, generator=g) * 2 - 1).to(torch.bfloat16)
    return u(int(cu_q[-1]), H, 192), u(int(cu_k[-1]), H, 256), u(int(cu_k[-1]), 64), cu_q, cu_k


def reference(q, k_nope, k_pe, v, cu_q, cu_k, scale=SCALE, pe=True, top_left=False):
    """fp64, a plain loop over the sequences: head h scores q . [k_nope_h | k_pe], row i admits key j iff j <= i + n_k - n_q
    (``top_left``: j <= i; ``pe`` False: the 64 k_pe columns dropped).  Returns out (Tq, H, 128), lse (H, Tq), zeros where a row admits
    no key or no sequence owns it, and the mask (Tq,) of the rows that admit a key."""
    q, k_nope, k_pe, v = (t.double().numpy() for t in (q, k_nope, k_pe, v))
    (Tq, H, _), cols = q.shape, 192 if pe else 128
    out, lse, live = np.zeros((Tq, H, 128)), np.zeros((H, Tq)), np.zeros(Tq, dtype=bool)
    for b in range(len(cu_q) - 1):
        (sq, eq), (sk, ek) = (int(cu_q[b]), int(cu_q[b + 1])), (int(cu_k[b]), int(cu_k[b + 1]))
        admit = np.arange(ek - sk)[None, :] <= np.arange(eq - sq)[:, None] + (0 if top_left else (ek - sk) - (eq - sq))
        live[sq:eq] = rows = admit.any(-1)
        for h in range(H if rows.any() else 0):
            k =np.concatenate([k_nope[sk:ek, h], k_pe[sk:ek]], -1)
            z = np.where(admit, scale * q[sq:eq, h, :cols] @ k[:, :cols].T, -np.inf)[rows]
            mx = z.max(-1, keepdims=True)
            e = np.exp(z - mx)
            out[sq:eq, h][rows], lse[h, sq:eq][rows] = e / e.sum(-1, keepdims=True) @ v[sk:ek, h], (mx + np.log(e.sum(-1, keepdims=True)))[:, 0]
    return torch.from_numpy(out), torch.from_numpy(lse), torch.from_numpy(live)


@functools.lru_cache(maxsize=None)
def expected(case, H):
    q, kv, k_pe, cu_q, cu_k = inputs(case, H)
    return reference(q, kv[..., :128], k_pe, kv[..., 128:], cu_q, cu_k)


@pytest.mark.parametrize("case,wrong", [("A", "pe"), ("B", "pe"), ("C", "pe"), ("B", "top_left"), ("C", "top_left")])
def test_gpu_inputs_tell_a_right_kernel_from_a_likely_wrong_one(case, wrong):
    """(Batch A is self-attention under one array: D = 0 in every sequence, where the two alignments are one mask.)"""
    q, kv, k_pe, cu_q, cu_k = inputs(case, 2)
    _, lse, live = expected(case, 2)
    other = reference(q, kv[..., :128], k_pe, kv[..., 128:], cu_q, cu_k, **{"pe": {"pe": False}, "top_left": {"top_left": True}}[wrong])[1]
    assert (lse - other)[:, live].abs().max().item() >= 10 * TOL


def test_abi_table_matches_the_header_and_the_library(built):
    from test_lib_cpu import _ctypes_kind, _prototypes
    protos, lib = _prototypes(HEADER), built.mla_prefill()
    assert sorted(protos) == sorted(built.MLA_PREFILL_ABI)
    for s, (res, args) in built.MLA_PREFILL_ABI.items():
        ret, kinds = protos[s]
        assert [_ctypes_kind(x) for x in args] == kinds and _ctypes_kind(res) == ret, s
        assert getattr(lib, s).argtypes == args and getattr(lib, s).restype is res, s


def test_every_kernel_runs_without_scratch(built):
    kernels = _device_kernels(built.lib_path(built.MLA_PREFILL_NAME))
    names = " ".join(k[0] for k in kernels)
    assert "mla_prefill_fwd_kernel" in names and "bidir_schedule_kernel" in names
    for name, scratch, vgpr in kernels:
        assert scratch == 0 and vgpr <= 512, (name, scratch, vgpr)


# ---- refusals, before any HIP call (this machine has no GPU: a HIP call would answer FA_ERR_HIP) ----
_GOOD = dict(q=256, k_nope=512, k_pe=768, v=1024, out=1280, lse=1536, cu_q=1792, cu_k=1792, ws=2048, nseq=3, Tq=300, Tk=400, H=4, k_ld=1024,
             k_hs=256, v_ld=1024, v_hs=256, scale=0.0)
_BAD = [
    (dict(nseq=0), "positive"), (dict(Tq=0), "positive"), (dict(Tk=-1), "positive"), (dict(H=0), "positive"), (dict(q=0), "null pointer"),
    (dict(k_pe=0), "null pointer"), (dict(v=0), "null pointer"), (dict(lse=0), "null pointer"), (dict(cu_k=0), "null pointer"),
    (dict(ws=0), "null pointer"), (dict(scale=-1.0), "softmax_scale"), (dict(scale=float("inf")), "softmax_scale"),
    (dict(scale=float("nan")), "softmax_scale"), (dict(k_ld=1028), "k_nope: row stride and head stride must be multiples of 8"),
    (dict(v_hs=260), "v: row stride and head stride must be multiples of 8"), (dict(k_hs=120), "k_nope: head stride below"),
    (dict(v_ld=512), "v: row stride below"), (dict(k_ld=1 << 22, Tk=128), "k_nope: byte offsets"), (dict(Tk=1 << 20), "k_nope: byte offsets"),
    (dict(Tq=1 << 21), "q: byte offsets"), (dict(Tq=1 << 20), "out: byte offsets"), (dict(k_nope=520), "16-byte aligned"),
    (dict(out=1288), "16-byte aligned"), (dict(ws=2176), "256-byte aligned"),
]


@pytest.mark.parametrize("over,msg", _BAD, ids=[",".join(f"{k}={v}" for k, v in o.items()) for o, _ in _BAD])
def test_call_rejects_each_bad_argument_before_any_hip_call(built, over, msg):
    a, lib = dict(_GOOD, **over), built.mla_prefill()
    rc = lib.fa_mi355x_fwd_mla_prefill(*[a[n] or None for n in ("q", "k_nope", "k_pe", "v", "out", "lse", "cu_q", "cu_k", "ws")],
                                       *[a[n] for n in ("nseq", "Tq", "Tk", "H", "k_ld", "k_hs", "v_ld", "v_hs", "scale")], None)
    err = lib.fa_mi355x_mla_prefill_last_error().decode()
    assert rc == BAD_ARG and msg in err, (rc, err)


def test_python_checks_name_the_operand_before_the_library_is_called(monkeypatch):
    from flash_attention_minitorch_amd import _lib, device_ops as ops
    monkeypatch.setattr(_lib, "mla_prefill", lambda: pytest.fail("the library was called"))
    z = lambda *shape, dtype=torch.bfloat16: torch.zeros(*shape, dtype=dtype)
    q, kv, k_pe, cu = z(10, 2, 192), z(10, 2, 256), z(10, 64), torch.tensor([0, 10], dtype=torch.int32)
    k, v = kv[..., :128], kv[..., 128:]
    for bad, exc, msg in [
        (lambda: ops.flash_attn_mla_prefill(z(10, 2, 128), k, k_pe, v, cu), ValueError, "q must be"),
        (lambda: ops.flash_attn_mla_prefill(q, z(10, 2, 192), k_pe, v, cu), ValueError, "k_nope must be"),
        (lambda: ops.flash_attn_mla_prefill(q, k, z(10, 2, 64), v, cu), ValueError, "k_pe must be"),
        (lambda: ops.flash_attn_mla_prefill(q, k, k_pe, z(10, 2, 64), cu), ValueError, "v must be"),
        (lambda: ops.flash_attn_mla_prefill(q, k.float(), k_pe, v, cu), TypeError, "k_nope must be bfloat16"),
        (lambda: ops.flash_attn_mla_prefill(q, k, z(9, 64), v, cu), ValueError, "k_pe must have k_nope's 10 rows"),
        (lambda: ops.flash_attn_mla_prefill(q, z(12, 2, 128), z(12, 64), z(12, 2, 128), cu), ValueError, "cu_seqlens_k=None means self-attention"),
        (lambda: ops.flash_attn_mla_prefill(q, k, k_pe, z(10, 3, 128), cu), ValueError, "v must be (Tk, H, 128)"),
        (lambda: ops.flash_attn_mla_prefill(q, k, k_pe, z(10, 128, 2).transpose(1, 2), cu), ValueError, "v may be a view, but its last dimension"),
        (lambda: ops.flash_attn_mla_prefill(q, z(10, 2, 132)[..., 4:], k_pe, v, cu), ValueError, "k_nope may be a view"),
        (lambda: ops.flash_attn_mla_prefill(q, k, k_pe, v, cu, softmax_scale=-1.0), ValueError, "softmax_scale must be"),
        (lambda: ops.mla_prefill_workspace(z(10, 2, 128), k, cu), ValueError, "q must be"),
    ]:
        with pytest.raises(exc, match=re.escape(msg)):
            bad()


@pytest.mark.parametrize("nseq,Tq,Tk,H", [(5, 394, 394, 2), (4, 197, 685, 5), (1, 1, 1, 1), (16, 16384, 16384, 128), (3, 127, 9, 2)])
def test_workspace_is_the_query_block_map(built, nseq, Tq, Tk, H):
    ws = built.mla_prefill().fa_mi355x_fwd_mla_prefill_workspace_bytes
    assert ws(nseq, Tq, Tk, H) == -(-32 * (Tq // 128 + nseq) // 256) * 256
    assert ws(0, Tq, Tk, H) == ws(nseq, 0, Tk, H) == ws(nseq, Tq, 0, H) == ws(nseq, Tq, Tk, 0) == 0
