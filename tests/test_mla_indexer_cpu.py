"""The lightning indexer of sparse MLA decode without a GPU (include/flash_attn_mi355x_mla_indexer.h, csrc/fa_mla_indexer.h): the fp64
definitions that tests/test_gpu_mla_indexer.py compares with, how sharp its cases are, the C ABI against the header, every new
refusal in front of a HIP call and the Python operand checks."""
import functools
import re

import numpy as np
import pytest
import torch

from test_decode_cpu import built  # noqa: F401  (the module-scoped build fixture)
from test_mla_cpu import BAD_ARG, SEED

HEADER = "flash_attn_mi355x_mla_indexer.h"
DI, NCAP = 128, 1024
# The GPU score cases: (HI, Nq) x the two sequences' lengths (2 < Nq for Nq = 3 and 5; 1000 reaches the second 512-key chunk).
HEADS, LENS = [(64, 1), (64, 3), (20, 2), (128, 5)], [(300, 2), (1000, 129)]
FUSED = (64, 3, (1000, 129), 64)   # (HI, Nq, lengths, topk) of the fused call: every row but those of length 2 has to choose


def index_inputs(seed, B, Ncap, HI, Nq):
    """q_idx (B, Nq, HI, 128) and the index keys (B, Ncap, 128), U(-1, 1) rounded to bf16; weights (B, Nq, HI) fp32, U(-1, 1)."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *shape: torch.rand(*shape, generator=g) * 2 - 1
    return u(B, Nq, HI, DI).to(torch.bfloat16), u(B, Nq, HI), u(B, Ncap, DI).to(torch.bfloat16)


def index_scores_reference(q_idx, weights, kidx, lens, causal):
    """fp64 (score, bound), both (B, Nq, Ncap): score[b, i, s] = sum_h w[b, i, h] max(0, q[b, i, h] . k[b, s]) where s is admitted
    (s < len_b, and s <= len_b - Nq + i under causal), -inf elsewhere; bound = (128 + HI + 2) 2^-24 sum_h |w_h| sum_c |q_hc| |k_c|: the
    products of bf16 values are exact in fp32, which leaves the fp32 sums of 128 terms per dot and HI per head sum and two roundings."""
    q, w, k = q_idx.double().numpy(), weights.double().numpy(), kidx.double().numpy()
    (B, Nq, HI, _), Ncap = q.shape, k.shape[1]
    score = np.einsum("bih,bihs->bis", w, np.maximum(np.einsum("bihc,bsc->bihs", q, k), 0))
    bound = (DI + HI + 2) * 2.0 ** -24 * np.einsum("bih,bihs->bis", np.abs(w), np.einsum("bihc,bsc->bihs", np.abs(q), np.abs(k)))
    s, i = np.arange(Ncap)[None, None, :], np.arange(Nq)[None, :, None]
    n = np.clip(np.asarray(lens), 0, Ncap)[:, None, None]
    score[~((s < n) & ((s <= n - Nq + i) | (not causal)))] = -np.inf
    return torch.from_numpy(score), torch.from_numpy(bound)


def topk_reference(scores, lens, topk):
    """int32 (B, Nq, topk): per row the entries of scores[b, i, :len_b] that are neither -inf nor NaN in a stable descending sort (equal
    values, -0 = +0, by position ascending), the first topk of them, sorted ascending, then -1."""
    x = scores.double().numpy()
    out = np.full(x.shape[:2] + (topk,), -1, dtype=np.int32)
    for b, i in np.ndindex(*x.shape[:2]):
        row = x[b, i, :min(max(int(lens[b]), 0), x.shape[2])]
        pos = np.flatnonzero(~np.isnan(row) & ~np.isneginf(row))
        pick = np.sort(pos[np.argsort(-row[pos], kind="stable")[:topk]])
        out[b, i, :pick.size] = pick
    return torch.from_numpy(out)


@functools.lru_cache(maxsize=None)
def score_case(HI, Nq, lens, causal):
    """(q_idx, weights, kidx, (score, bound)) of a GPU case, computed once and shared."""
    q, w, k = index_inputs(SEED, 2, NCAP, HI, Nq)
    return q, w, k, index_scores_reference(q, w, k, lens, causal)


def test_references_on_a_case_small_enough_to_read():
    q, w, k = torch.zeros(1, 2, 1, DI), torch.tensor([[[2.0], [-1.0]]]), torch.zeros(1, 4, DI)
    q[..., 0], k[:, :, 0] = 1.0, torch.tensor([3.0, -5.0, 1.0, 7.0])
    score, bound = index_scores_reference(q, w, k, (3,), True)
    ninf = -np.inf
    assert score[0].tolist() == [[6.0, 0.0, ninf, ninf], [-3.0, -0.0, -1.0, ninf]] and bound[0, 0, 0].item() == 131 * 2.0 ** -24 * 6
    x = torch.tensor([[[1.0, float("nan"), 1.0, -0.0, 0.0, -np.inf, 2.0, 9.0]]])
    assert topk_reference(x, (7,), 4)[0, 0].tolist() == [0, 2, 3, 6] and topk_reference(x, (2,), 4)[0, 0].tolist() == [0, -1, -1, -1]


def test_the_fused_case_is_sharp_and_its_masks_matter():
    """With t a row's k-th reference score and eps = 2 x the bound there, the band |score - t| <= eps, inside which the GPU test lets
    a position go either way, holds at most 1 % of the row's admitted entries; and the causal lists differ from the non-causal ones."""
    HI, Nq, lens, topk = FUSED
    lists = {}
    for causal in (True, False):
        score, bound = score_case(HI, Nq, lens, causal)[3]
        lists[causal] = topk_reference(score, lens, topk)
        for b, i in np.ndindex(2, Nq):
            row = score[b, i][~torch.isneginf(score[b, i])]
            if row.numel() > topk:
                kth = lists[causal][b, i].long()[score[b, i][lists[causal][b, i].long()].argmin()]
                band = ((row - score[b, i, kth]).abs() <= 2 * bound[b, i, kth]).sum().item()
                print(f"b {b} i {i} causal {causal}: band {band} of {row.numel()}")
                assert band <= 0.01 * row.numel()
    assert not torch.equal(lists[True], lists[False])
    assert torch.equal(lists[True][:, -1], lists[False][:, -1])   # (the last token sees everything either way)


# ---- the C ABI ----
def test_indexer_abi_table_matches_the_header_and_the_library(built):
    from test_lib_cpu import _ctypes_kind, _prototypes
    protos, lib = _prototypes(HEADER), built.mla()
    assert sorted(protos) == sorted(built.MLA_INDEXER_ABI) and not set(protos) & (set(built.MLA_ABI) | set(built.MLA_SPARSE_ABI))
    for s, (res, args) in built.MLA_INDEXER_ABI.items():
        assert ([_ctypes_kind(x) for x in args], _ctypes_kind(res)) == (protos[s][1], protos[s][0]), s
        assert getattr(lib, s).argtypes == args and getattr(lib, s).restype is res, s
    assert lib.fa_mi355x_mla_indexer_scores_bytes(2, 3, 1000) == 24000 and lib.fa_mi355x_mla_indexer_scores_bytes(2, 0, 1000) == 0
    # the chunk policy: the GPU cases cut a sequence in two, the benchmark's into 1024-key chunks; a token group holds 64 KB of Q
    assert [lib.fa_mi355x_mla_index_chunks(2, HI, Nq, NCAP) for HI, Nq in HEADS] == [2] * 4
    assert lib.fa_mi355x_mla_index_chunks(32, 64, 1, 32768) == 32 and lib.fa_mi355x_mla_index_chunks(32, 64, 8, 32768) == 16
    assert lib.fa_mi355x_mla_index_chunks(0, 64, 1, 1024) == 0


# ---- refusals, before any HIP call (this machine has no GPU: a HIP call would answer FA_ERR_HIP) ----
_GOOD = dict(q=32, w=64, new=0, kidx=96, scores=128, idx=160, lens=192, table=0, B=2, HI=64, Nq=1, topk=128, Ncap=1024, num_pages=0,
             page_size=0, max_pages=0, causal=1)
_PAGED = dict(table=512, num_pages=16, page_size=128, max_pages=8)
_BAD = [(dict(q=0), "null pointer argument: q_idx"), (dict(w=0), "null pointer argument: q_idx and weights"), (dict(w=68), "16-byte aligned"),
        (dict(kidx=0), "null pointer argument: kidx_cache"), (dict(new=8), "16-byte aligned"), (dict(scores=0), "null pointer argument: scores"),
        (dict(scores=132), "scores must be 16-byte aligned"), (dict(idx=0), "null pointer argument: indices"), (dict(idx=162), "4-byte aligned"),
        (dict(lens=194), "4-byte aligned"), (dict(HI=0), "positive"), (dict(HI=129), "HI must be in 1 .. 128"), (dict(Nq=129), "Nq > 128"),
        (dict(topk=0), "multiple of 64"), (dict(topk=100), "multiple of 64"), (dict(Nq=128, topk=1 << 23), "2^30"),
        (dict(_PAGED, page_size=192), "multiple of 128"), (dict(_PAGED, max_pages=1 << 25), "fit an int"), (dict(Ncap=0), "Ncap"),
        (dict(Ncap=1 << 23), "2 GiB")]


@pytest.mark.parametrize("over,msg", _BAD, ids=[",".join(f"{k}={v}" for k, v in o.items()) for o, _ in _BAD])
def test_indexer_rejects_each_bad_argument_before_any_hip_call(built, over, msg):
    a, lib = dict(_GOOD, **over), built.mla()
    rc = lib.fa_mi355x_mla_indexer(*[a[n] or None for n in ("q", "w", "new", "kidx", "scores", "idx", "lens", "table")],
                                   *[a[n] for n in ("B", "HI", "Nq", "topk", "Ncap", "num_pages", "page_size", "max_pages", "causal")], None)
    err = lib.fa_mi355x_mla_last_error().decode()
    assert rc == BAD_ARG and msg in err, (rc, err)


def test_the_separate_entry_points_refuse_their_own_arguments(built):
    lib, err = built.mla(), lambda: built.mla().fa_mi355x_mla_last_error().decode()
    assert lib.fa_mi355x_mla_index_scores(32, 64, None, 96, None, 192, None, 2, 64, 1, 1024, 0, 0, 0, 1, None) == BAD_ARG and "scores" in err()
    assert lib.fa_mi355x_mla_index_topk(128, 160, 192, 2, 1, 1024, 96, None) == BAD_ARG and "multiple of 64" in err()
    assert lib.fa_mi355x_mla_index_topk(128, 160, 192, 2, 1, 1 << 30, 64, None) == BAD_ARG and "2^30" in err()
    assert lib.fa_mi355x_mla_index_append(None, 96, 192, None, 2, 1, 1024, 0, 0, 0, None) == BAD_ARG and "kidx_new" in err()
    assert lib.fa_mi355x_mla_index_append(32, 96, 192, 512, 2, 1, 0, 16, 64, 8, None) == BAD_ARG and "multiple of 128" in err()


def test_python_checks_name_the_operand_before_the_library_is_called(monkeypatch):
    from flash_attention_minitorch_amd import _lib, device_ops as ops, modules_transformer as mt
    monkeypatch.setattr(_lib, "mla", lambda: pytest.fail("the library was called"))
    z = lambda *shape, dtype=torch.bfloat16, **kw: torch.zeros(*shape, dtype=dtype, **kw)
    f32, i32 = torch.float32, torch.int32
    lens, q, w, k, s = z(2, dtype=i32), z(2, 1, 4, DI), z(2, 1, 4, dtype=f32), z(2, 256, DI), z(2, 1, 256, dtype=f32)
    for bad, exc, msg in [
        (lambda: ops.mla_indexer(z(2, 4, DI), w, k, lens, 64), ValueError, "q_idx must be (B, Nq, HI, 128)"),
        (lambda: ops.mla_indexer(z(2, 1, 4, 64), w, k, lens, 64), ValueError, "q_idx must be"),
        (lambda: ops.mla_indexer(q.float(), w, k, lens, 64), TypeError, "q_idx must be bfloat16"),
        (lambda: ops.mla_indexer(z(2, 1, 129, DI), z(2, 1, 129, dtype=f32), k, lens, 64), ValueError, "HI in 1 .. 128"),
        (lambda: ops.mla_indexer(q, w.bfloat16(), k, lens, 64), TypeError, "weights must be float32"),
        (lambda: ops.mla_indexer(q, z(2, 1, 5, dtype=f32), k, lens, 64), ValueError, "weights must be (B, Nq, HI)"),
        (lambda: ops.mla_indexer(q, w, z(2, 256, 576), lens, 64), ValueError, "kidx_cache must be"),
        (lambda: ops.mla_indexer(q, w, k.float(), lens, 64), TypeError, "kidx_cache must be bfloat16"),
        (lambda: ops.mla_indexer(z(2, 1, 4, DI, device="meta"), w, k, lens, 64), ValueError, "q_idx must be contiguous and on the cache's device"),
        (lambda: ops.mla_indexer(q, w, k, lens, 100), ValueError, "multiple of 64"),
        (lambda: ops.mla_indexer(q, w, k, lens, 64, kidx_new=z(2, 2, DI)), ValueError, "kidx_new must be"),
        (lambda: ops.mla_indexer(q, w, z(4, 100, DI), lens, 64, block_table=z(2, 2, dtype=i32)), ValueError, "multiple of 128"),
        (lambda: ops.mla_index_scores(q, w, k, lens, scores=z(2, 1, 255, dtype=f32)), ValueError, "scores must be a contiguous float32"),
        (lambda: ops.mla_index_topk(s.double(), lens, 64), TypeError, "scores must be float32"),
        (lambda: ops.mla_index_topk(s[0], lens, 64), ValueError, "scores must be (B, Nq, Ncap)"),
        (lambda: ops.mla_index_topk(s, lens, 96), ValueError, "multiple of 64"),
        (lambda: ops.mla_index_topk(s, lens, 64, indices=z(2, 1, 64, dtype=torch.int64)), ValueError, "indices must be a contiguous int32"),
        (lambda: ops.mla_index_append(z(2, 129, DI), k, lens), ValueError, "Nq must be in 1 .. 128"),
        (lambda: ops.mla_index_append(z(2, 1, 64), k, lens), ValueError, "kidx_new must be"),
        (lambda: mt.mla_attention_step(z(2, 1, 8), mt.LatentKVCache(1, 2, 128, "cpu", index_keys=True), 0, None, 1, None, indices=s,
                                       indexer=mt.IndexerWeights(None, None, None), topk=64), ValueError, "indexer and indices exclude"),
        (lambda: mt.mla_attention_step(z(2, 1, 8), mt.LatentKVCache(1, 2, 128, "cpu"), 0, None, 1, None,
                                       indexer=mt.IndexerWeights(None, None, None), topk=64), ValueError, "index_keys=True"),
    ]:
        with pytest.raises(exc, match=re.escape(msg)):
            bad()
