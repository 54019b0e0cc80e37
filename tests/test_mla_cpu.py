"""Multi-head latent attention decode without a GPU (include/flash_attn_mi355x_mla.h, csrc/fa_mla.h): the fp64 reference and the
absorption identity it stands on, the C ABI against the header, every refusal in front of a HIP call, the size queries' laws, the
kernels' registers, and the inputs of tests/test_gpu_mla.py (which must tell a kernel that drops the rope columns from a right one)."""
import os
import re

import numpy as np
import pytest
import torch

from test_abi_cpu import _device_kernels
from test_decode_cpu import built  # noqa: F401  (the module-scoped build fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "flash_attn_mi355x_mla.h"
DQK, DV, TOL, SCALE = 576, 512, 1e-3, 192 ** -0.5   # TOL: the project's bf16 figure, max-abs on out and lse
BAD_ARG = 1

# The GPU cases (tests/test_gpu_mla.py): (H, Nq) -> the two sequences' lengths.  Every length of {1, 63, 64, 65, 128, 129, 300, 768}
# appears, and one sequence of length 0.
NCAP, SEED = 768, 11
CASES = {(5, 1): (1, 768), (16, 3): (63, 300), (40, 2): (64, 129), (128, 1): (65, 128), (128, 2): (300, 0)}


def inputs(seed, B, Ncap, H, Nq):
    """q (B, Nq, H, 576) and the latent cache (B, Ncap, 576): U(-1, 1) rounded to bf16."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *shape: (torch.rand(*shape, generator=g) * 2 - 1).to(torch.bfloat16)
    return u(B, Nq, H, DQK), u(B, Ncap, DQK)


def reference(q, kv, lens, scale, causal, score_cols=DQK):
    """fp64 MLA decode: q (B, Nq, H, 576), kv (B, Ncap, 576), lens valid rows (clamped to [0, Ncap]).  Scores over the first
    ``score_cols`` columns (576: all of them), values from columns 0..511, query i at position len - Nq + i (causal: keys j <= it).
    Returns (out (B, Nq, H, 512), lse (B, H, Nq)) as torch fp64; rows with no admissible key: 0, -inf."""
    q, kv = (np.asarray(t.double() if isinstance(t, torch.Tensor) else t, dtype=np.float64) for t in (q, kv))
    (B, Nq, H, _), Ncap = q.shape, kv.shape[1]
    out, lse = np.zeros((B, Nq, H, DV)), np.full((B, H, Nq), -np.inf)
    for b in range(B):
        n = min(max(int(lens[b]), 0), Ncap)
        for i in range(Nq):
            m = min(n, n - Nq + i + 1) if causal else n
            if m <= 0:
                continue
            z = scale * q[b, i, :, :score_cols] @ kv[b, :m, :score_cols].T   # (H, m)
            mx = z.max(-1, keepdims=True)
            e = np.exp(z - mx)
            l = e.sum(-1, keepdims=True)
            out[b, i], lse[b, :, i] = (e / l) @ kv[b, :m, :DV], (mx + np.log(l))[:, 0]
    return torch.from_numpy(out), torch.from_numpy(lse)


def test_reference_is_unabsorbed_multi_head_attention():
    """The absorption identity mla_attention_step relies on, in fp64: attention of head h on k_h = [c W_UK[h]^T | k_pe] and
    v_h = c W_UV[h] equals the latent reference on q = [q_nope W_UK[h] | q_pe] followed by W_UV[h]."""
    rng = np.random.default_rng(0)
    B, Nq, H, n, dn, dv, lens = 2, 2, 3, 9, 5, 4, (9, 4)
    q_nope, q_pe = rng.standard_normal((B, Nq, H, dn)), rng.standard_normal((B, Nq, H, 64))
    kv, w_uk, w_uv = rng.standard_normal((B, n, DQK)), rng.standard_normal((H, dn, DV)), rng.standard_normal((H, DV, dv))
    q_abs = np.concatenate([np.einsum("bthn,hnc->bthc", q_nope, w_uk), q_pe], -1)
    out, lse = reference(q_abs, kv, lens, 0.3, True)
    got = np.einsum("bthc,hcv->bthv", out.numpy(), w_uv)
    for b in range(B):
        for h in range(H):
            k_h = np.concatenate([kv[b, :, :DV] @ w_uk[h].T, kv[b, :, DV:]], -1)   # (n, dn + 64)
            v_h = kv[b, :, :DV] @ w_uv[h]
            for i in range(Nq):
                m = lens[b] - Nq + i + 1
                z = 0.3 * np.concatenate([q_nope[b, i, h], q_pe[b, i, h]]) @ k_h[:m].T
                p = np.exp(z - z.max())
                assert np.allclose(got[b, i, h], p / p.sum() @ v_h[:m], rtol=1e-10, atol=1e-10)
                assert np.isclose(lse[b, h, i].item(), z.max() + np.log(p.sum()), rtol=1e-12)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("H,Nq", list(CASES))
def test_gpu_inputs_tell_the_rope_columns_from_their_absence(H, Nq, causal):
    q, kv = inputs(SEED, 2, NCAP, H, Nq)
    full, nope = reference(q, kv, CASES[H, Nq], SCALE, causal)[1], reference(q, kv, CASES[H, Nq], SCALE, causal, DV)[1]
    live = ~torch.isneginf(full)
    assert (full - nope)[live].abs().max().item() >= 10 * TOL


# ---- the C ABI ----
def test_mla_abi_table_matches_the_header_and_the_library(built):
    from test_lib_cpu import _ctypes_kind, _prototypes
    protos = _prototypes(HEADER)
    lib = built.mla()
    assert sorted(protos) == sorted(built.MLA_ABI)
    for s, (res, args) in built.MLA_ABI.items():
        ret, kinds = protos[s]
        assert [_ctypes_kind(x) for x in args] == kinds and _ctypes_kind(res) == ret, s
        assert getattr(lib, s).argtypes == args and getattr(lib, s).restype is res, s
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)
    names = {s: [re.findall(r"\w+", p)[-1] for p in ps.split(",")] for s, ps in re.findall(r"\b(fa_mi355x_\w+)\s*\(([^()]*)\)\s*;", text)}
    assert names["fa_mi355x_fwd_decode_mla"] == ("q kv_new kv_cache out lse cache_seqlens block_table workspace B H Nq Ncap num_pages "
                                                 "page_size max_pages softmax_scale causal stream").split()
    assert names["fa_mi355x_mla_append"] == "kv_new kv_cache cache_seqlens block_table B Nq Ncap num_pages page_size max_pages stream".split()


def test_every_mla_kernel_runs_without_scratch(built):
    kernels = _device_kernels(built.lib_path(built.MLA_NAME))
    names = " ".join(k[0] for k in kernels)
    assert names.count("mla_decode_split_kernel") == 2 and "mla_decode_combine_kernel" in names and "mla_append_kernel" in names
    for name, scratch, vgpr in kernels:
        assert scratch == 0 and vgpr <= 512, (name, scratch, vgpr)


# ---- refusals, before any HIP call (this machine has no GPU: a HIP call would answer FA_ERR_HIP) ----
_GOOD = dict(q=32, kv_new=0, kv=64, out=96, lse=0, lens=128, table=0, ws=256, B=2, H=16, Nq=1, Ncap=768, num_pages=0, page_size=0, max_pages=0,
             scale=SCALE, causal=1)
_PAGED = dict(table=512, num_pages=12, page_size=128, max_pages=6)
_BAD = [
    (dict(Nq=0), "positive"), (dict(Nq=129), "Nq > 128"), (dict(B=0), "positive"), (dict(H=0), "positive"), (dict(Ncap=0), "Ncap"),
    (dict(q=0), "null pointer"), (dict(kv=0), "null pointer"), (dict(out=0), "null pointer"), (dict(ws=0), "null workspace"),
    (dict(q=8), "aligned"), (dict(kv_new=8), "aligned"), (dict(scale=0.0), "softmax_scale"), (dict(scale=-1.0), "softmax_scale"),
    (dict(scale=float("nan")), "softmax_scale"), (dict(_PAGED, page_size=100), "multiple of 128"), (dict(_PAGED, num_pages=0), "positive"),
    (dict(Ncap=1 << 21), "2 GiB"),
]


@pytest.mark.parametrize("over,msg", _BAD, ids=[",".join(f"{k}={v}" for k, v in o.items()) for o, _ in _BAD])
def test_mla_call_rejects_each_bad_argument_before_any_hip_call(built, over, msg):
    a, lib = dict(_GOOD, **over), built.mla()
    rc = lib.fa_mi355x_fwd_decode_mla(*[a[n] or None for n in ("q", "kv_new", "kv", "out", "lse", "lens", "table", "ws")], a["B"], a["H"],
                                      a["Nq"], a["Ncap"], a["num_pages"], a["page_size"], a["max_pages"], a["scale"], a["causal"], None)
    err = lib.fa_mi355x_mla_last_error().decode()
    assert rc == BAD_ARG and msg in err, (rc, err)


@pytest.mark.parametrize("over,msg", [(dict(kv_new=0), "null pointer"), (dict(kv=0), "null pointer"), (dict(Nq=129), "Nq > 128"),
                                      (dict(Nq=0), "positive"), (dict(_PAGED, page_size=64), "multiple of 128")])
def test_mla_append_rejects_each_bad_argument_before_any_hip_call(built, over, msg):
    a, lib = dict(dict(_GOOD, kv_new=32), **over), built.mla()
    rc = lib.fa_mi355x_mla_append(*[a[n] or None for n in ("kv_new", "kv", "lens", "table")], a["B"], a["Nq"], a["Ncap"], a["num_pages"],
                                  a["page_size"], a["max_pages"], None)
    assert rc == BAD_ARG and msg in lib.fa_mi355x_mla_last_error().decode()


def test_python_checks_name_the_operand_before_the_library_is_called(monkeypatch):
    from flash_attention_minitorch_amd import _lib, device_ops as ops
    monkeypatch.setattr(_lib, "mla", lambda: pytest.fail("the library was called"))
    z = lambda *shape, dtype=torch.bfloat16: torch.zeros(*shape, dtype=dtype)
    lens, q, kv = torch.zeros(2, dtype=torch.int32), z(2, 1, 4, DQK), z(2, 128, DQK)
    for bad, exc, msg in [
        (lambda: ops.flash_attn_decode_mla(z(2, 1, 4, 512), kv, lens, SCALE), ValueError, "q must be"),
        (lambda: ops.flash_attn_decode_mla(q, z(2, 128, 512), lens, SCALE), ValueError, "kv_cache must be"),
        (lambda: ops.flash_attn_decode_mla(q, kv, lens, SCALE, kv_new=z(2, 1, 512)), ValueError, "kv_new must be"),
        (lambda: ops.flash_attn_decode_mla(q.float(), kv, lens, SCALE), TypeError, "q must be bfloat16"),
        (lambda: ops.flash_attn_decode_mla(q, kv.float(), lens, SCALE), TypeError, "kv_cache must be bfloat16"),
        (lambda: ops.flash_attn_decode_mla(z(2, 0, 4, DQK), kv, lens, SCALE), ValueError, "Nq in 1 .. 128"),
        (lambda: ops.flash_attn_decode_mla(z(2, 129, 4, DQK), kv, lens, SCALE), ValueError, "Nq in 1 .. 128"),
        (lambda: ops.flash_attn_decode_mla(q, kv, lens, None), ValueError, "softmax_scale is required"),
        (lambda: ops.flash_attn_decode_mla(q, z(4, 100, DQK), lens, SCALE, block_table=torch.zeros(2, 2, dtype=torch.int32)), ValueError,
         "multiple of 128"),
        (lambda: ops.mla_append(z(2, 129, DQK), kv, lens), ValueError, "Nq must be in 1 .. 128"),
        (lambda: ops.mla_append(z(2, 1, 512), kv, lens), ValueError, "kv_new must be"),
        (lambda: ops.mla_workspace(z(2, 1, 4, 512), kv), ValueError, "q must be"),
    ]:
        with pytest.raises(exc, match=re.escape(msg)):
            bad()


# ---- the size queries ----
@pytest.mark.parametrize("B,H,Nq,Ncap", [(2, 5, 1, 768), (2, 128, 2, 768), (2, 16, 3, 128), (32, 128, 1, 32768), (1, 1, 1, 1), (64, 128, 2, 4096)])
def test_size_queries_are_consistent(built, B, H, Nq, Ncap):
    lib = built.mla()
    n, ws = lib.fa_mi355x_decode_mla_splits(B, H, Nq, Ncap), lib.fa_mi355x_decode_mla_workspace_bytes(B, H, Nq, Ncap)
    assert n >= 1 and ws == (0 if n == 1 else B * H * n * Nq * (DV + 2) * 4)
    assert n > 1 if Ncap == 768 else n == 1 if Ncap <= 128 else True   # the GPU cases at Ncap = 768 split, the one-split case (128) does not
    assert lib.fa_mi355x_decode_mla_splits(0, H, Nq, Ncap) == 0 and lib.fa_mi355x_decode_mla_workspace_bytes(B, H, 0, Ncap) == 0
