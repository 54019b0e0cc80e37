"""CPU-side checks of the KV-cache decode library (include/flash_attn_mi355x_decode.h): exported symbols, the gfx950 code object
without scratch, argument validation before any HIP call, the split policy (with the split counts that the shapes of
tests/test_gpu_decode_edges.py rely on), the Python entry point's checks, and this file's fp64 decode reference (used by
tests/test_gpu_decode.py) against the dense oracle."""
import ctypes
import os
import re

import numpy as np
import pytest

import oracle
from test_abi_cpu import _device_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "flash_attn_mi355x_decode.h")


def decode_reference(q, k, v, lens, causal, scale):
    """fp64 decode attention: q (BH, Nq, d), k / v (BH, Ncap, d), lens (BH,) valid rows (clamped to [0, Ncap]).  Query i sits at position
    len - Nq + i (causal: sees keys j <= that).  Returns (out (BH, Nq, d), lse (BH, Nq)); rows with no admissible key: 0, -inf."""
    BH, Nq, d = q.shape
    Ncap = k.shape[1]
    out = np.zeros((BH, Nq, v.shape[2]))
    lse = np.full((BH, Nq), -np.inf)
    for b in range(BH):
        n = int(min(max(int(lens[b]), 0), Ncap))
        if n == 0:
            continue
        s = scale * (q[b].astype(np.float64) @ k[b, :n].astype(np.float64).T)   # (Nq, n)
        if causal:
            pos = n - Nq + np.arange(Nq)
            s = np.where(np.arange(n)[None, :] <= pos[:, None], s, -np.inf)
        m = s.max(axis=1)
        ok = np.isfinite(m)
        e = np.exp(s - np.where(ok, m, 0)[:, None])
        e[~ok] = 0
        l = e.sum(axis=1)
        out[b][ok] = (e[ok] @ v[b, :n].astype(np.float64)) / l[ok, None]
        lse[b][ok] = m[ok] + np.log(l[ok])
    return out, lse


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from flash_attention_minitorch_amd import _lib
    return _lib


def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(fa_mi355x_\w+)\s*\(", text)))


def test_decode_library_exports_every_declared_symbol(built):
    syms = _declared()
    assert {"fa_mi355x_fwd_decode", "fa_mi355x_decode_workspace_bytes", "fa_mi355x_decode_splits",
            "fa_mi355x_decode_last_error"} <= set(syms)
    lib = built.decode()
    for s in syms:
        assert hasattr(lib, s), s


def test_decode_code_object_is_gfx950_without_scratch(built):
    kernels = _device_kernels(built.lib_path(built.DECODE_NAME))
    names = " ".join(k[0] for k in kernels)
    assert "decode_split_kernel" in names and "decode_combine_kernel" in names
    for name, scratch, vgpr in kernels:
        assert scratch == 0, (name, scratch)
        assert vgpr <= 512


# one valid call (fake non-null device pointers: a launch would fail, so a code other than the expected one shows a HIP call)
_ONE = 16
_GOOD = dict(q=_ONE, k=_ONE, v=_ONE, out=_ONE, lse=_ONE, lens=_ONE, ws=_ONE, B=1, H=2, Nq=1, Ncap=4096, d=64, layout=1, scale=0.0,
             causal=1, dtype=1)
_BAD = [
    ("q", 0, 1, "null"), ("k", 0, 1, "null"), ("v", 0, 1, "null"), ("out", 0, 1, "null"),
    ("B", 0, 1, "positive"), ("H", -1, 1, "positive"), ("Nq", 0, 1, "positive"), ("Ncap", 0, 1, "positive"), ("d", 0, 1, "positive"),
    ("Nq", 129, 1, "fa_mi355x_fwd_layout"),
    ("layout", 2, 1, "layout"), ("dtype", 5, 1, "dtype"),
    ("d", 48, 2, "32, 64, 128"), ("d", 256, 2, "32, 64, 128"),
    ("scale", -1.0, 1, "softmax_scale"), ("scale", float("nan"), 1, "softmax_scale"), ("scale", float("inf"), 1, "softmax_scale"),
    ("ws", 0, 1, "workspace"),
    ("Ncap", 1 << 24, 1, "2 GiB"),
]


def _call(lib, **over):
    a = dict(_GOOD, **over)
    vp = lambda x: ctypes.c_void_p(x)
    return lib.fa_mi355x_fwd_decode(vp(a["q"]), vp(a["k"]), vp(a["v"]), vp(a["out"]), vp(a["lse"]), vp(a["lens"]), vp(a["ws"]), a["B"],
                                    a["H"], a["Nq"], a["Ncap"], a["d"], a["layout"], a["scale"], a["causal"], a["dtype"], None)


@pytest.mark.parametrize("field,value,code,msg", _BAD, ids=[f"{f}={v}" for f, v, _, _ in _BAD])
def test_decode_rejects_each_bad_argument_before_any_hip_call(built, field, value, code, msg):
    lib = built.decode()
    assert lib.fa_mi355x_decode_splits(1, 2, 1, 4096, 64, 1) > 1   # (so the null workspace case needs one)
    assert _call(lib, **{field: value}) == code
    err = lib.fa_mi355x_decode_last_error().decode()
    assert err and msg in err, err


def test_decode_optional_pointers_are_not_required(built):
    lib = built.decode()
    # lse and cache_seqlens may be NULL, and a one-split call needs no workspace: all three pass validation and reach the launch,
    # which fails on the fake pointers (or, with a device, on the launch itself) -- never with a validation code
    ns = lib.fa_mi355x_decode_splits(64, 32, 1, 256, 64, 1)
    assert ns == 1 and lib.fa_mi355x_decode_workspace_bytes(64, 32, 1, 256, 64) == 0


_SHAPES = [(1, 8, 1, 4096, 128), (1, 8, 1, 65536, 128), (32, 32, 1, 4096, 128), (8, 8, 1, 4096, 64), (8, 8, 1, 1024, 32),
           (8, 8, 4, 1024, 64), (8, 8, 64, 1024, 64), (1, 2, 1, 65536, 128), (2, 3, 33, 300, 32), (4, 2, 128, 512, 128),
           (64, 32, 1, 256, 64), (1, 1, 1, 1, 32)]


def test_split_policy_is_pure_and_sizes_the_workspace(built):
    lib = built.decode()
    seen = set()
    for B, H, Nq, Ncap, d in _SHAPES:
        ns = [lib.fa_mi355x_decode_splits(B, H, Nq, Ncap, d, dt) for dt in (0, 1)]
        ws = [lib.fa_mi355x_decode_workspace_bytes(B, H, Nq, Ncap, d) for _ in range(2)]
        assert ns[0] == ns[1] == lib.fa_mi355x_decode_splits(B, H, Nq, Ncap, d, 1) >= 1
        assert ws[0] == ws[1]
        ns = ns[0]
        seen.add(ns > 1)
        # at least 256 keys per chunk; the chunks cover Ncap
        assert ns == 1 or Ncap / ns >= 128
        need = 0 if ns == 1 else B * H * ns * Nq * (d + 2) * 4
        assert ws[0] == need, (B, H, Nq, Ncap, d, ns, ws[0])
    assert seen == {True, False}
    assert lib.fa_mi355x_decode_splits(1, 2, 1, 65536, 128, 1) > 1
    assert lib.fa_mi355x_decode_splits(32, 32, 1, 4096, 128, 1) == 1
    assert lib.fa_mi355x_decode_splits(0, 2, 1, 65536, 128, 1) == 0
    assert lib.fa_mi355x_decode_workspace_bytes(1, 2, 0, 65536, 128) == 0


def test_split_counts_that_the_gpu_edge_cases_rely_on(built):
    """tests/test_gpu_decode_edges.py picks its shapes for the path the policy sends them down; the same counts, checked wherever
    the library builds.  (B, H, Hkv, Nq, Ncap, d) -> splits."""
    lib = built.decode()
    want = [((3, 2, 2, 33, 256, 64), 1),            # a cache of one chunk
            ((128, 8, 8, 1, 700, 64), 1),           # 1024 workgroups without splitting: one chunk of six super tiles
            ((128, 8, 8, 3, 700, 128), 1),
            ((128, 32, 8, 1, 700, 64), 1),          # the same, four heads per kv head
            ((16, 8, 8, 1, 8192, 128), 8),          # chunks of 1024 keys
            ((16, 8, 8, 5, 8192, 64), 8),
            ((40, 2, 2, 1, 1300, 64), 6),           # chunks of 256 keys, one and two row blocks
            ((40, 2, 2, 33, 1300, 64), 6),
            ((1, 8, 8, 1, 1048447, 128), 128),      # the largest batch element the 2 GiB check admits: chunks of 8192 keys
            ((2, 71, 1, 1, 520, 64), 3),            # one query's 71 heads: three row blocks
            ((6, 71, 1, 11, 520, 128), 3),
            ((6, 28, 4, 128, 520, 64), 2),          # 28 row blocks per kv head: 672 workgroups per split, chunks of 512
            ((1, 4096, 1, 128, 64, 32), 1)]
    for (B, H, Hkv, Nq, Ncap, d), ns in want:
        for dt in (0, 1):
            assert lib.fa_mi355x_decode_splits_gqa(B, H, Hkv, Nq, Ncap, d, dt) == ns, (B, H, Hkv, Nq, Ncap, d)
            if H == Hkv:
                assert lib.fa_mi355x_decode_splits(B, H, Nq, Ncap, d, dt) == ns, (B, H, Nq, Ncap, d)
        assert lib.fa_mi355x_decode_workspace_bytes_gqa(B, H, Hkv, Nq, Ncap, d) == (0 if ns == 1 else B * H * ns * Nq * (d + 2) * 4)
    # one row more and the 2 GiB check refuses the cache before any HIP call
    assert _call(lib, B=1, H=8, Nq=1, Ncap=1048447 + 1, d=128, ws=_ONE) == 1
    assert "2 GiB" in lib.fa_mi355x_decode_last_error().decode()


def test_flash_attn_decode_python_checks(built):
    import torch
    from flash_attention_minitorch_amd import device_ops

    q = torch.zeros(2, 1, 4, 64)
    kc = torch.zeros(2, 256, 4, 64)
    with pytest.raises(built.FlashAttnLibraryError, match="GPU"):
        device_ops.flash_attn_decode(q, kc, kc.clone())
    with pytest.raises(TypeError, match="dtype"):
        device_ops.flash_attn_decode(q, kc.bfloat16(), kc.bfloat16())
    with pytest.raises(TypeError, match="dtype"):
        device_ops.flash_attn_decode(q.double(), kc.double(), kc.double())
    for bad in (torch.zeros(3, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)):
        with pytest.raises(ValueError, match="cache_seqlens"):
            device_ops.flash_attn_decode(q, kc, kc.clone(), cache_seqlens=bad)
    with pytest.raises(ValueError, match=r"\(B, H\)"):
        device_ops.flash_attn_decode(q, torch.zeros(2, 256, 8, 64), torch.zeros(2, 256, 8, 64))
    with pytest.raises(ValueError, match="layout"):
        device_ops.flash_attn_decode(q, kc, kc.clone(), layout="nbhd")
    with pytest.raises(ValueError, match="row length"):
        device_ops.flash_attn_decode(torch.zeros(2, 1, 4, 80), kc, kc.clone())


@pytest.mark.parametrize("causal", [False, True])
def test_decode_reference_agrees_with_dense_oracle_when_nq_equals_len(causal):
    rng = np.random.default_rng(3)
    BH, N, d = 3, 37, 32
    q, k, v = (rng.uniform(-1, 1, (BH, N, d)) for _ in range(3))
    pad = np.full((BH, 11, d), np.nan)   # rows past len must not matter
    out, lse = decode_reference(q, np.concatenate([k, pad], 1), np.concatenate([v, pad], 1), np.full(BH, N), causal, d ** -0.5)
    ro, rL, _, _ = oracle.dense_attention_fw(q, k, v, causal)
    assert np.max(np.abs(out - ro)) < 1e-12 and np.max(np.abs(lse - rL)) < 1e-12
    # len = 0 and lengths beyond Ncap clamp; a causal row below position 0 is empty
    out, lse = decode_reference(q[:, :4], k, v, np.array([0, N + 7, 2]), causal, d ** -0.5)
    assert np.all(out[0] == 0) and np.all(np.isneginf(lse[0]))
    full, fl = decode_reference(q[:, :4], k, v, np.array([0, N, 2]), causal, d ** -0.5)
    assert np.array_equal(out[1], full[1])
    if causal:
        assert np.all(np.isneginf(lse[2, :2])) and np.all(np.isfinite(lse[2, 2:]))
