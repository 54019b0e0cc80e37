"""Sparse MLA decode without a GPU (include/flash_attn_mi355x_mla_sparse.h, csrc/fa_mla_sparse.h): the fp64 definition, the index
lists of tests/test_gpu_mla_sparse.py and what they must tell apart, the C ABI against the header, the new refusals in front of a HIP
call, the size queries' laws and the Python operand checks."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from test_decode_cpu import built  # noqa: F401  (the module-scoped build fixture)
from test_mla_cpu import BAD_ARG, DQK, DV, NCAP, ROOT, SCALE, SEED, TOL, inputs, reference

HEADER = "flash_attn_mi355x_mla_sparse.h"
# The GPU cases: (H, Nq, topk) -> the two sequences' lengths.  In the first, query (0, 0) is -1 throughout.
CASES = {(5, 1, 64): (63, 768), (16, 3, 128): (65, 300), (72, 2, 256): (129, 768), (128, 1, 768): (768, 300), (128, 2, 768): (768, 0)}
EMPTY_QUERY = (5, 1, 64)


def sparse_reference(q, kv, lens, indices, scale, causal):
    """fp64 sparse MLA decode, the header's definition: query (b, i) attends the entries j of indices[b, i] with 0 <= j < len_b (and
    j <= len_b - Nq + i under causal), each a key of its own.  (out (B, Nq, H, 512), lse (B, H, Nq)); no admitted entry: 0, -inf."""
    q, kv, idx = q.double().numpy(), kv.double().numpy(), indices.numpy()
    (B, Nq, H, _), Ncap = q.shape, kv.shape[1]
    out, lse = np.zeros((B, Nq, H, DV)), np.full((B, H, Nq), -np.inf)
    for b in range(B):
        n = min(max(int(lens[b]), 0), Ncap)
        for i in range(Nq):
            j = idx[b, i]
            j = j[(j >= 0) & (j < n) & ((j <= n - Nq + i) | (not causal))]
            if j.size:
                z = scale * q[b, i] @ kv[b, j].T   # (H, admitted)
                mx = z.max(-1, keepdims=True)
                e = np.exp(z - mx)
                out[b, i], lse[b, :, i] = e / e.sum(-1, keepdims=True) @ kv[b, j, :DV], (mx + np.log(e.sum(-1, keepdims=True)))[:, 0]
    return torch.from_numpy(out), torch.from_numpy(lse)


def indices(seed, B, Nq, topk, lens, empty_query=False):
    """int32 (B, Nq, topk): per query a random draw of the whole capacity (many entries fall >= len_b), about a quarter -1 at random,
    entries 64..127 all -1 (a whole empty tile) when topk >= 192, entry 1 = entry 0 (a duplicate), entry 2 = len_b - 1 (admitted for
    the last query only, under causal), entries 3, 4, 5 = len_b, NCAP + 5, -7 (never admitted)."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.stack([torch.stack([torch.randperm(NCAP, generator=g)[:topk] for _ in range(Nq)]) for _ in range(B)]).int()
    idx[torch.rand(B, Nq, topk, generator=g) < 0.25] = -1
    if topk >= 192:
        idx[:, :, 64:128] = -1
    idx[:, :, 1] = idx[:, :, 0]
    for b in range(B):
        idx[b, :, 2:6] = torch.tensor([lens[b] - 1, lens[b], NCAP + 5, -7], dtype=torch.int32)
    if empty_query:
        idx[0, 0] = -1
    return idx


@functools.lru_cache(maxsize=None)
def case(H, Nq, topk, causal):
    """(q, kv, lens, indices, (out, lse)) of a GPU case, computed once and shared."""
    (q, kv), lens = inputs(SEED, 2, NCAP, H, Nq), CASES[H, Nq, topk]
    idx = indices(SEED, 2, Nq, topk, lens, (H, Nq, topk) == EMPTY_QUERY)
    return q, kv, lens, idx, sparse_reference(q, kv, lens, idx, SCALE, causal)


@pytest.mark.parametrize("H,Nq,topk", list(CASES))
def test_gpu_inputs_tell_the_lists_and_the_mask_from_their_absence(H, Nq, topk):
    """A kernel that ignores the lists, or the causal bound, cannot pass the GPU cases.  (Nq = 1: the one query is the last position,
    so the causal bound j <= len_b - 1 IS j < len_b and the two references must agree; they must differ wherever Nq > 1.)"""
    q, kv, lens, idx, (out_c, lse_c) = case(H, Nq, topk, True)
    out_n, lse_n = case(H, Nq, topk, False)[4]
    assert torch.equal(lse_c, lse_n) == (Nq == 1)
    for causal, (out, lse) in ((True, (out_c, lse_c)), (False, (out_n, lse_n))):
        dense = reference(q, kv, lens, SCALE, causal)[1]
        for b, n in enumerate(lens):
            live = ~torch.isneginf(lse[b])
            if n == 0 or ((H, Nq, topk) == EMPTY_QUERY and b == 0):   # the length-0 sequence, the all -1 query
                assert not live[:, 0].any() and not out[b, 0].any()
            if n >= 63 and live.any():
                assert (lse[b] - dense[b])[live].abs().min().item() >= 10 * TOL
    assert torch.isneginf(lse_n).any() == ((H, Nq, topk) == EMPTY_QUERY or 0 in lens)


# ---- the C ABI ----
def test_sparse_abi_table_matches_the_header_and_the_library(built):
    from test_lib_cpu import _ctypes_kind, _prototypes
    protos, lib = _prototypes(HEADER), built.mla()
    assert sorted(protos) == sorted(built.MLA_SPARSE_ABI) and not set(protos) & set(built.MLA_ABI)
    for s, (res, args) in built.MLA_SPARSE_ABI.items():
        assert ([_ctypes_kind(x) for x in args], _ctypes_kind(res)) == (protos[s][1], protos[s][0]), s
        assert getattr(lib, s).argtypes == args and getattr(lib, s).restype is res, s
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)
    params = re.search(r"fa_mi355x_fwd_decode_mla_sparse\s*\(([^()]*)\)", text).group(1)
    assert [re.findall(r"\w+", p)[-1] for p in params.split(",")] == (
        "q kv_new kv_cache indices out lse cache_seqlens block_table workspace B H Nq topk Ncap num_pages page_size max_pages "
        "softmax_scale causal stream").split()


# ---- refusals, before any HIP call (this machine has no GPU: a HIP call would answer FA_ERR_HIP) ----
_GOOD = dict(q=32, kv_new=0, kv=64, idx=160, out=96, lse=0, lens=128, table=0, ws=256, B=2, H=16, Nq=1, topk=768, Ncap=768, num_pages=0,
             page_size=0, max_pages=0, scale=SCALE, causal=1)
_PAGED = dict(table=512, num_pages=12, page_size=128, max_pages=6)
_BAD = [(dict(idx=0), "null pointer argument: indices"), (dict(idx=162), "indices must be 4-byte aligned"), (dict(topk=0), "multiple of 64"),
        (dict(topk=-64), "multiple of 64"), (dict(topk=100), "multiple of 64"), (dict(Nq=128, topk=1 << 23), "2^31"),
        (dict(_PAGED, num_pages=1 << 24), "pool's rows"), (dict(ws=0), "null workspace"), (dict(q=0), "null pointer"), (dict(Nq=129), "Nq > 128")]


@pytest.mark.parametrize("over,msg", _BAD, ids=[",".join(f"{k}={v}" for k, v in o.items()) for o, _ in _BAD])
def test_sparse_call_rejects_each_bad_argument_before_any_hip_call(built, over, msg):
    a, lib = dict(_GOOD, **over), built.mla()
    rc = lib.fa_mi355x_fwd_decode_mla_sparse(*[a[n] or None for n in ("q", "kv_new", "kv", "idx", "out", "lse", "lens", "table", "ws")],
                                             *[a[n] for n in ("B", "H", "Nq", "topk", "Ncap", "num_pages", "page_size", "max_pages", "scale",
                                                              "causal")], None)
    err = lib.fa_mi355x_mla_last_error().decode()
    assert rc == BAD_ARG and msg in err, (rc, err)


# ---- the size queries: the dense rule on the index list, restated ----
@pytest.mark.parametrize("B,H,Nq,topk", [(2,) + k for k in CASES] + [(32, 128, 1, 2048), (32, 16, 2, 2048), (1, 1, 1, 64), (64, 128, 2, 4096)])
def test_sparse_size_queries_follow_the_rule(built, B, H, Nq, topk):
    lib = built.mla()
    n, ws = lib.fa_mi355x_decode_mla_sparse_splits(B, H, Nq, topk), lib.fa_mi355x_decode_mla_sparse_workspace_bytes(B, H, Nq, topk)
    groups = B * Nq * -(-H // 64)
    chunk = max(256, -(-(-(-topk // max(1, -(-512 // groups)))) // 128) * 128)   # two rounds of 256 CUs, whole 128-entry multiples
    assert n == -(-topk // chunk) and ws == (0 if n == 1 else B * H * n * Nq * (DV + 2) * 4)
    assert (n > 1) == (topk >= 768) if B == 2 else True   # the GPU cases: topk = 768 splits, topk <= 256 does not
    for zero in ((0, H, Nq, topk), (B, 0, Nq, topk), (B, H, 0, topk), (B, H, Nq, 0), (B, H, Nq, -64)):
        assert lib.fa_mi355x_decode_mla_sparse_splits(*zero) == 0 and lib.fa_mi355x_decode_mla_sparse_workspace_bytes(*zero) == 0


def test_python_checks_name_the_indices_before_the_library_is_called(monkeypatch):
    from flash_attention_minitorch_amd import _lib, device_ops as ops
    monkeypatch.setattr(_lib, "mla", lambda: pytest.fail("the library was called"))
    z = lambda *shape, dtype=torch.int32, **kw: torch.zeros(*shape, dtype=dtype, **kw)
    lens, q, kv = z(2), z(2, 1, 4, DQK, dtype=torch.bfloat16), z(2, 128, DQK, dtype=torch.bfloat16)
    for idx, exc, msg in [(z(2, 1, 64, dtype=torch.int64), TypeError, "indices must be an int32 tensor"), ([[0] * 64], TypeError, "int32 tensor"),
                          (z(2, 2, 64), ValueError, "indices must be (B, Nq, topk)"), (z(2, 64), ValueError, "indices must be (B, Nq, topk)"),
                          (z(2, 1, 100), ValueError, "multiple of 64"), (z(2, 1, 0), ValueError, "multiple of 64"),
                          (z(2, 1, 128)[:, :, ::2], ValueError, "contiguous"), (z(2, 1, 64, device="meta"), ValueError, "on the cache's device")]:
        with pytest.raises(exc, match=re.escape(msg)):
            ops.flash_attn_decode_mla(q, kv, lens, SCALE, indices=idx)
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.mla_workspace(q, kv, topk=100)
