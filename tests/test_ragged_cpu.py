"""CPU-side checks of the ragged-batch entry points (include/flash_attn_mi355x_decode_ragged.h: packed new tokens, a per-sequence
count of them in cu_seqlens_q on the device, contiguous or paged caches): the eight symbols declared in their own header, exported
and bound; every bad argument answered with its code and a message that names it before any HIP call (fake non-null pointers, as in
tests/test_extend_cpu.py: a launch would fail with another code); the split policy (pure, sizing the workspace, with the counts
tests/test_gpu_ragged.py relies on); this file's fp64 ragged reference and append reference (loops of the uniform references over
the sequences) on hand-made cases; the Python checks of the three device_ops functions; and the model layer's calls under the
recorder."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_decode_append_cpu import append_reference
from test_decode_cpu import _declared, built, decode_reference  # noqa: F401  (built: the module-scoped build fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "flash_attn_mi355x_decode_ragged.h")
RAGGED = ["fa_mi355x_ragged_splits", "fa_mi355x_ragged_workspace_bytes", "fa_mi355x_fwd_ragged", "fa_mi355x_ragged_append",
          "fa_mi355x_fwd_ragged_append", "fa_mi355x_fwd_ragged_paged", "fa_mi355x_ragged_append_paged",
          "fa_mi355x_fwd_ragged_append_paged"]
CALLS = RAGGED[2:]


# ---- the references (used by tests/test_gpu_ragged.py) ----

def seq_rows(cu, T, b):
    """(s_b, e_b) of sequence b in buffers of T packed rows: the clamp the header defines."""
    s = min(max(int(cu[b]), 0), T)
    return s, min(max(int(cu[b + 1]), s), T)


def ragged_reference(q, k, v, cu, lens, causal, scale, out=None, lse=None):
    """fp64 ragged attention: q (T, H, d) packed, k / v (B, Hkv, Ncap, d), cu (B + 1,), lens (B,) or None (= Ncap).  Sequence b is
    decode_reference on its own rows (query head h reads cache head h // G).  Returns (out (T, H, d), lse (H, T)); the rows no sequence
    owns keep what ``out`` / ``lse`` held (NaN when not given)."""
    T, H, d = q.shape
    B, Hkv, Ncap, _ = k.shape
    G = H // Hkv
    out = np.full((T, H, v.shape[3]), np.nan) if out is None else out.astype(np.float64)
    lse = np.full((H, T), np.nan) if lse is None else lse.astype(np.float64)
    for b in range(B):
        s, e = seq_rows(cu, T, b)
        if e == s:
            continue
        n = Ncap if lens is None else lens[b]
        o, l = decode_reference(q[s:e].transpose(1, 0, 2), np.repeat(k[b], G, axis=0), np.repeat(v[b], G, axis=0), np.full(H, n), causal,
                                scale)
        out[s:e] = o.transpose(1, 0, 2)
        lse[:, s:e] = l
    return out, lse


def ragged_append_reference(k_new, cache, cu, lens):
    """The placement rule per sequence: k_new (T, Hkv, d_new) packed into a copy of cache (B, Ncap, Hkv, d); token i of sequence b goes
    to row clamp(len_b, 0, Ncap) - nq_b + i when that is >= 0, zeros in columns d_new .. d-1; every other row keeps its bits."""
    T = k_new.shape[0]
    out = cache.copy()
    for b in range(cache.shape[0]):
        s, e = seq_rows(cu, T, b)
        out[b:b + 1] = append_reference(k_new[s:e][None], cache[b:b + 1], None if lens is None else [lens[b]], e - s)
    return out


def test_ragged_reference_on_hand_made_cases():
    rng = np.random.default_rng(5)
    H, Hkv, d, Ncap = 4, 2, 8, 6
    q = rng.uniform(-1, 1, (9, H, d))
    k, v = (rng.uniform(-1, 1, (3, Hkv, Ncap, d)) for _ in range(2))
    k[0, :, 4:], v[0, :, 4:] = np.nan, np.nan   # rows at or past the length must not matter
    cu, lens = [0, 2, 2, 7], [4, 5, 6]            # counts 2, 0, 5; two unused rows behind them
    out, lse = ragged_reference(q, k, v, cu, lens, True, 0.5)
    assert np.all(np.isnan(out[7:])) and np.all(np.isnan(lse[:, 7:])) and np.all(np.isfinite(out[:7])) and np.all(np.isfinite(lse[:, :7]))
    # one row by hand: token 1 of sequence 0, head 3 (cache head 1), sits at position 4 - 2 + 1 = 3 and sees keys 0 .. 3
    s = 0.5 * k[0, 1, :4] @ q[1, 3]
    p = np.exp(s - s.max())
    assert np.allclose(out[1, 3], p @ v[0, 1, :4] / p.sum(), atol=1e-12) and np.isclose(lse[3, 1], s.max() + np.log(p.sum()))
    # token 0 of sequence 2 (5 tokens, length 6) sits at position 1 and sees keys 0 and 1; not causal: all six
    s = 0.5 * k[2, 0, :2] @ q[2, 0]
    p = np.exp(s - s.max())
    assert np.allclose(out[2, 0], p @ v[2, 0, :2] / p.sum(), atol=1e-12)
    full, _ = ragged_reference(q, k, v, cu, lens, False, 0.5)
    s = 0.5 * k[2, 0] @ q[2, 0]
    p = np.exp(s - s.max())
    assert np.allclose(full[2, 0], p @ v[2, 0] / p.sum(), atol=1e-12)
    # a sequence is decode_reference on its rows alone, whatever its neighbours are
    alone, _ = ragged_reference(q[2:7], k[2:], v[2:], [0, 5], lens[2:], True, 0.5)
    assert np.array_equal(alone, out[2:7])
    # more tokens than keys: the rows at negative positions are empty; a length of 0 empties the sequence; given buffers are kept
    out, lse = ragged_reference(q, k, v, [0, 6, 6, 9], [4, 0, 0], True, 0.5, out=np.full((9, H, d), 7.0), lse=np.full((H, 9), 7.0))
    assert np.all(out[:2] == 0) and np.all(np.isneginf(lse[:, :2])) and np.all(np.isfinite(lse[:, 2:6]))
    assert np.all(out[6:] == 0) and np.all(np.isneginf(lse[:, 6:]))
    # the clamp: entries beyond T and a decreasing pair (sequence 1 owns rows 4 .. 8, sequence 2 none)
    assert [seq_rows([0, 4, 99, 5], 9, b) for b in range(3)] == [(0, 4), (4, 9), (9, 9)]
    assert [seq_rows([-3, 4, 2], 9, b) for b in range(2)] == [(0, 4), (4, 4)]
    a, _ = ragged_reference(q, k, v, [0, 4, 99, 5], lens, True, 0.5)
    b, _ = ragged_reference(q, k, v, [0, 4, 9, 9], lens, True, 0.5)
    assert np.array_equal(a, b)


def test_ragged_append_reference_on_hand_made_cases():
    k_new = np.arange(1, 8 * 2 * 3 + 1, dtype=np.float32).reshape(8, 2, 3)
    cache = -np.ones((3, 5, 2, 4), dtype=np.float32)
    out = ragged_append_reference(k_new, cache, [0, 2, 2, 7], [4, 3, 3])   # counts 2, 0, 5; row 7 unused
    assert np.array_equal(out[0, 2:4, :, :3], k_new[0:2]) and np.all(out[0, 2:4, :, 3] == 0)
    assert np.all(out[0, :2] == -1) and np.all(out[0, 4] == -1) and np.all(out[1] == -1)
    # five tokens into a length of three: tokens 0 and 1 fall below row 0, tokens 2 .. 4 land on rows 0 .. 2
    assert np.array_equal(out[2, 0:3, :, :3], k_new[4:7]) and np.all(out[2, 3:] == -1)
    full = ragged_append_reference(k_new, cache, [0, 2, 2, 7], None)     # no lengths: the last nq_b rows
    assert np.array_equal(full[0, 3:5, :, :3], k_new[0:2]) and np.array_equal(full[2, 0:5, :, :3], k_new[2:7])
    clamped = ragged_append_reference(k_new, cache, [0, 2, 2, 7], [99, 3, -4])
    assert np.array_equal(clamped[0], full[0]) and np.all(clamped[2] == -1)


# ---- the C ABI ----

def _params(text, sym):
    m = re.search(r"\b%s\s*\(([^)]*)\)" % sym, text)
    assert m, sym
    return [p.strip() for p in m.group(1).split(",")]


def test_the_eight_ragged_symbols_are_declared_exported_and_bound(built):
    from test_lib_cpu import _ctypes_kind, _prototypes
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert '#include "flash_attn_mi355x_decode_ragged.h"' in open(os.path.join(ROOT, "include", "flash_attn_mi355x_decode.h")).read()
    assert sorted(set(re.findall(r"\b(fa_mi355x_\w+)\s*\(", text))) == sorted(RAGGED) == sorted(built.RAGGED_ABI)
    assert not [s for s in _declared() if "ragged" in s]   # (the decode header's own text declares none of them)
    assert len(built.PAGED_ABI) == 6
    protos = _prototypes("flash_attn_mi355x_decode_ragged.h")
    lib = built.decode()
    for s in RAGGED:
        assert hasattr(lib, s), s
        res, args = built.RAGGED_ABI[s]
        ret, kinds = protos[s]
        assert [_ctypes_kind(a) for a in args] == kinds and _ctypes_kind(res) == ret, s
        assert getattr(lib, s).argtypes == args and getattr(lib, s).restype is res, s
    for s in CALLS:
        params = _params(text, s)
        i = params.index("const int* cu_seqlens_q")
        assert params[i + 1] == "const int* cache_seqlens" and "int T" in params and "int Nq" not in params, s
        if s.endswith("_paged"):
            assert params[i + 2] == "const int* block_table", s
            j = params.index("int num_pages")
            assert params[j - 1] == "int T" and params[j:j + 3] == ["int num_pages", "int page_size", "int max_pages"], s
            assert "int Ncap" not in params, s
        else:
            assert params[params.index("int T") + 1] == "int Ncap" and "const int* block_table" not in params, s


# one valid call of each form (fake non-null device pointers: a launch would fail, so a code other than the expected one shows a
# HIP call)
_ONE = 16
_GOOD = dict(q=_ONE, kn=_ONE, vn=_ONE, k=_ONE, v=_ONE, out=_ONE, lse=_ONE, cu=_ONE, lens=_ONE, table=_ONE, ws=_ONE, B=2, H=4, Hkv=2, T=161,
             Ncap=2048, num_pages=40, page_size=128, max_pages=16, d_new=64, d=64, layout=1, scale=0.0, causal=1, dtype=1)
_VP = ctypes.c_void_p
BAD_ARG, BAD_D = 1, 2


def _call(lib, sym, **over):
    a = dict(_GOOD, **over)
    paged, fused, append = sym.endswith("_paged"), "fwd_ragged_append" in sym, "fwd" not in sym
    where = ("num_pages", "page_size", "max_pages") if paged else ("Ncap",)
    table = ("table",) if paged else ()
    if append:
        args = [_VP(a[n]) for n in ("kn", "vn", "k", "v", "cu", "lens") + table] + [a[n] for n in ("B", "Hkv", "T") + where + (
            "d_new", "d", "layout", "dtype")] + [None]
    else:
        ptrs = ("q", "kn", "vn", "k", "v", "out", "lse", "cu", "lens") if fused else ("q", "k", "v", "out", "lse", "cu", "lens")
        dims = ("d_new", "d") if fused else ("d",)
        args = [_VP(a[n]) for n in ptrs + table + ("ws",)] + [a[n] for n in ("B", "H", "Hkv", "T") + where + dims] + [
            a["layout"], a["scale"], a["causal"], a["dtype"], None]
    rc = getattr(lib, sym)(*args)
    return rc, lib.fa_mi355x_decode_last_error().decode()


# (overrides, code, message)
_EVERY = [   # what every form rejects
    (dict(cu=0), BAD_ARG, "cu_seqlens_q"), (dict(k=0), BAD_ARG, "null"), (dict(v=0), BAD_ARG, "null"),
    (dict(B=0), BAD_ARG, "positive"), (dict(B=-2), BAD_ARG, "positive"), (dict(T=0), BAD_ARG, "positive"), (dict(T=-5), BAD_ARG, "positive"),
    (dict(d=0, d_new=0), BAD_ARG, "positive"), (dict(H=0, Hkv=0), BAD_ARG, "positive"),
    (dict(layout=2), BAD_ARG, "layout"), (dict(dtype=5), BAD_ARG, "dtype"),
    (dict(d=48, d_new=48), BAD_D, "32, 64, 128"), (dict(d=256, d_new=256), BAD_D, "32, 64, 128"),
]
_ATTEND = [
    (dict(ws=0), BAD_ARG, "fa_mi355x_ragged_workspace_bytes"),
    (dict(q=0), BAD_ARG, "null"), (dict(out=0), BAD_ARG, "null"), (dict(H=-1), BAD_ARG, "positive"), (dict(Hkv=0), BAD_ARG, "Hkv"),
    (dict(H=8, Hkv=3), BAD_ARG, "Hkv = 3"),
    (dict(scale=-1.0), BAD_ARG, "softmax_scale"), (dict(scale=float("nan")), BAD_ARG, "softmax_scale"),
    (dict(scale=float("inf")), BAD_ARG, "softmax_scale"),
    (dict(T=1 << 22), BAD_ARG, "2 GiB"),                                       # q: 2^22 rows of 4 heads of 64 bf16
    (dict(H=1 << 12, Hkv=1, T=1 << 13, d=32, d_new=32), BAD_ARG, "2^25"),      # G * T = 2^25 rows of one kv head
]
_APPEND = [
    (dict(kn=0), BAD_ARG, "null"), (dict(vn=0), BAD_ARG, "null"),
    (dict(d_new=0), BAD_ARG, "d_new = 0"), (dict(d_new=-3), BAD_ARG, "d_new = -3"), (dict(d_new=65), BAD_ARG, "d_new = 65"),
    (dict(d=128, d_new=129), BAD_ARG, "d_new = 129"),
]
_CONTIGUOUS = [(dict(Ncap=0), BAD_ARG, "positive")]
_CONTIGUOUS_ATTEND = [(dict(Ncap=1 << 24), BAD_ARG, "2 GiB")]                  # the cache: 2^24 rows of 2 heads of 64 bf16
_PAGING = [
    (dict(table=0), BAD_ARG, "block_table"),
    (dict(page_size=0), BAD_ARG, "page_size"), (dict(page_size=64), BAD_ARG, "page_size"), (dict(page_size=129), BAD_ARG, "page_size"),
    (dict(page_size=-128), BAD_ARG, "page_size"),
    (dict(num_pages=0), BAD_ARG, "num_pages"), (dict(num_pages=-3), BAD_ARG, "num_pages"),
    (dict(max_pages=0), BAD_ARG, "max_pages"), (dict(max_pages=-1), BAD_ARG, "max_pages"),
    (dict(max_pages=1 << 24), BAD_ARG, "max_pages * page_size"),               # 2^24 * 128 = 2^31
    (dict(page_size=1 << 24), BAD_ARG, "2 GiB"),                               # 2^24 rows * 2 heads * 64 * 2 bytes in one page
]


def _cases():
    out = []
    for sym in CALLS:
        bad = list(_EVERY)
        if "fwd" in sym:
            bad += _ATTEND
        if "append" in sym:   # (the fused forms reject what either half rejects)
            bad += _APPEND
        if sym.endswith("_paged"):
            bad += _PAGING
        else:
            bad += _CONTIGUOUS + (_CONTIGUOUS_ATTEND if "fwd" in sym else [])
        out += [(sym, o, c, m) for o, c, m in bad]
    return out


def _id(case):
    sym, over = case[0], case[1]
    return sym[10:] + "-" + ",".join(f"{k}={v}" for k, v in over.items())


@pytest.mark.parametrize("sym,over,code,msg", _cases(), ids=[_id(c) for c in _cases()])
def test_ragged_forms_reject_each_bad_argument_before_any_hip_call(built, sym, over, code, msg):
    rc, err = _call(built.decode(), sym, **over)
    assert rc == code and err and msg in err, (rc, err)


def test_the_append_counts_its_lanes_and_optional_pointers_are_optional(built):
    lib = built.decode()
    for sym in ("fa_mi355x_ragged_append", "fa_mi355x_ragged_append_paged"):
        rc, err = _call(lib, sym, T=1 << 30, Hkv=64)
        assert rc == BAD_ARG and "too many" in err, (rc, err)
    # lse and cache_seqlens may be NULL: the answer of such a call comes from a check BEHIND them (never called with every check
    # passed: that would launch on the fake pointers)
    for sym in CALLS:
        rc, err = _call(lib, sym, lse=0, lens=0, **(dict(ws=0) if "fwd" in sym else dict(d_new=65)))
        assert rc == BAD_ARG and ("workspace" if "fwd" in sym else "d_new") in err, (sym, rc, err)
    # a ragged call needs its workspace even as one split (the block map lives there)
    assert lib.fa_mi355x_ragged_splits(2, 4, 2, 161, 256, 64, 1) == 1
    for sym in [s for s in CALLS if "fwd" in s]:
        rc, err = _call(lib, sym, ws=0, Ncap=256, max_pages=2)
        assert rc == BAD_ARG and "workspace" in err, (sym, rc, err)


# ---- the policy ----

def _blocks(B, H, Hkv, T):
    return (H // Hkv) * T // 128 + min(B, T)


def _policy(B, H, Hkv, T, Ncap):
    """The policy as the header states it: Hkv * (floor(G * T / 128) + min(B, T)) groups, 512 workgroups wanted, chunks a multiple of
    256 keys."""
    groups = Hkv * _blocks(B, H, Hkv, T)
    want = max(1, -(-512 // groups))
    chunk = max(256, -(-(-(-Ncap // want)) // 256) * 256)
    return -(-Ncap // chunk)


def _workspace(B, H, Hkv, T, Ncap, d, ns):
    return -(-_blocks(B, H, Hkv, T) * 8 // 16) * 16 + H * ns * T * (d + 2) * 4


# (B, H, Hkv, T, Ncap, d)
_SHAPES = [(2, 2, 2, 161, 2048, 64), (2, 2, 2, 161, 256, 64), (32, 32, 8, 543, 8192 + 512, 128), (8, 32, 8, 4096, 8192 + 512, 128),
           (32, 32, 8, 32, 4096, 128), (1, 8, 1, 1, 65536, 128), (8, 2, 2, 626, 520, 32), (1, 1, 1, 5000, 5000, 64), (64, 32, 8, 64, 4608, 128),
           (1, 1, 1, 1, 1, 32), (5, 3, 1, 3, 1300, 64), (300, 4, 4, 7, 700, 64)]


def test_ragged_split_policy_is_pure_and_sizes_the_workspace(built):
    lib = built.decode()
    seen = set()
    for B, H, Hkv, T, Ncap, d in _SHAPES:
        ns = [lib.fa_mi355x_ragged_splits(B, H, Hkv, T, Ncap, d, dt) for dt in (0, 1, 1)]
        ws = [lib.fa_mi355x_ragged_workspace_bytes(B, H, Hkv, T, Ncap, d) for _ in range(2)]
        assert ns[0] == ns[1] == ns[2] == _policy(B, H, Hkv, T, Ncap) >= 1, (B, H, Hkv, T, Ncap)
        assert ws[0] == ws[1] == _workspace(B, H, Hkv, T, Ncap, d, ns[0]) > 0, (B, H, Hkv, T, Ncap, d, ns[0], ws[0])
        assert ns[0] == 1 or Ncap / ns[0] >= 128   # at least 256 keys per chunk; the chunks cover Ncap
        seen.add(ns[0] > 1)
    assert seen == {True, False}
    # the bound on the row blocks stands in for the extend policy's count: B sequences of one token are B blocks, as B batch elements are
    assert lib.fa_mi355x_ragged_splits(32, 32, 8, 32, 4096, 128, 1) == lib.fa_mi355x_extend_splits(32, 32, 8, 1, 4096, 128, 1)
    # ... and the known weakness: 543 tokens of which 512 sit in one sequence count 48 blocks where the extend call on that sequence counts 16
    assert lib.fa_mi355x_ragged_splits(32, 32, 8, 543, 8704, 128, 1) < lib.fa_mi355x_extend_splits(1, 32, 8, 512, 8704, 128, 1)
    assert all(lib.fa_mi355x_ragged_splits(3, 2, 2, t, 256, 64, 1) == 1 for t in (1, 129, 100000))   # Ncap <= 256: one split
    assert lib.fa_mi355x_ragged_splits(0, 2, 2, 160, 2048, 64, 1) == 0
    assert lib.fa_mi355x_ragged_splits(1, 8, 3, 160, 2048, 64, 1) == 0
    assert lib.fa_mi355x_ragged_workspace_bytes(1, 2, 2, 0, 2048, 64) == 0


# the shapes of tests/test_gpu_ragged.py whose path depends on the policy: (B, H, Hkv, T, Ncap, d) -> splits
GPU_SPLITS = [((2, 2, 2, 161, 2048, 64), 8),         # counts [160, 1]: three row blocks of two kv heads, chunks of 256 keys
              ((2, 2, 2, 161, 2048, 128), 8),
              ((8, 64, 64, 118, 700, 32), 1),        # eight row blocks of 64 kv heads are 512 workgroups: one chunk of six super tiles
              ((8, 2, 2, 626, 520, 64), 3),          # the parity batch: chunks of 256 keys
              ((8, 2, 2, 676, 520, 64), 3),          # ... with an unused tail of 50 rows
              ((6, 4, 2, 368, 256, 64), 1),          # a cache of one chunk: the bitwise comparison with the extend call
              ((3, 4, 2, 400, 1000, 64), 4)]         # graph capture and repeatability


def test_ragged_split_counts_that_the_gpu_tests_rely_on(built):
    lib = built.decode()
    for (B, H, Hkv, T, Ncap, d), ns in GPU_SPLITS:
        for dt in (0, 1):
            assert lib.fa_mi355x_ragged_splits(B, H, Hkv, T, Ncap, d, dt) == ns, (B, H, Hkv, T, Ncap, d)
        assert lib.fa_mi355x_ragged_workspace_bytes(B, H, Hkv, T, Ncap, d) == _workspace(B, H, Hkv, T, Ncap, d, ns)
    # the extend call on one sequence of the bitwise comparison is one split as well
    assert all(lib.fa_mi355x_extend_splits(1, 4, 2, nq, 256, 64, 1) == 1 for nq in (1, 33, 129, 200, 5))


def test_a_paged_ragged_call_is_sized_as_the_contiguous_one(built):
    import torch
    from flash_attention_minitorch_amd import device_ops

    lib = built.decode()
    q = torch.zeros(161, 4, 128)
    cu = torch.zeros(3, dtype=torch.int32)
    pool = torch.zeros(40, 256, 2, 128)
    tbl = torch.zeros(2, 8, dtype=torch.int32)
    want = lib.fa_mi355x_ragged_workspace_bytes(2, 4, 2, 161, 8 * 256, 128)
    assert want == _workspace(2, 4, 2, 161, 2048, 128, lib.fa_mi355x_ragged_splits(2, 4, 2, 161, 2048, 128, 1))
    for kw in (dict(block_table=tbl), dict(max_pages=8)):
        assert device_ops.ragged_workspace(q, pool, cu, "bnhd", **kw).numel() * 4 == want
    slab = torch.zeros(2, 2048, 2, 128)
    assert device_ops.ragged_workspace(q, slab, cu).numel() * 4 == want
    assert device_ops.ragged_workspace(q, slab.transpose(1, 2).contiguous(), cu, "bhnd").numel() * 4 == want
    with pytest.raises(ValueError, match="max_pages"):
        device_ops.ragged_workspace(q, pool, cu, "bnhd", max_pages=0)
    with pytest.raises(ValueError, match="cu_seqlens_q"):
        device_ops.ragged_workspace(q, slab, torch.zeros(4, dtype=torch.int32))


# ---- the Python layer ----

def test_flash_attn_ragged_python_checks(built):
    import torch
    from flash_attention_minitorch_amd import device_ops

    q = torch.zeros(40, 4, 64)
    kc = torch.zeros(2, 256, 2, 64)
    cu = torch.zeros(3, dtype=torch.int32)
    call = lambda *a, **kw: device_ops.flash_attn_ragged(*a, **kw)
    with pytest.raises(built.FlashAttnLibraryError, match="GPU"):
        call(q, kc, kc.clone(), cu)
    with pytest.raises(ValueError, match="3-d"):
        call(q[None], kc, kc.clone(), cu)
    with pytest.raises(TypeError, match="dtype"):
        call(q, kc.bfloat16(), kc.bfloat16(), cu)
    with pytest.raises(TypeError, match="dtype"):
        call(q.double(), kc.double(), kc.double(), cu)
    with pytest.raises(TypeError, match="dtype"):
        call(q, kc, kc.bfloat16(), cu)
    with pytest.raises(ValueError, match="one shape"):
        call(q, kc, torch.zeros(2, 128, 2, 64), cu)
    for bad in (None, torch.zeros(4, dtype=torch.int32), torch.zeros(3, 1, dtype=torch.int32), torch.zeros(3, dtype=torch.int64),
                torch.zeros(6, dtype=torch.int32)[::2], torch.zeros(3, dtype=torch.int32, device="meta")):
        with pytest.raises(ValueError, match="cu_seqlens_q"):
            call(q, kc, kc.clone(), bad)
    for bad in (torch.zeros(3, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)):
        with pytest.raises(ValueError, match="cache_seqlens"):
            call(q, kc, kc.clone(), cu, cache_seqlens=bad)
    with pytest.raises(ValueError, match="heads"):
        call(q, torch.zeros(2, 256, 3, 64), torch.zeros(2, 256, 3, 64), cu)
    with pytest.raises(ValueError, match="layout"):
        call(q, kc, kc.clone(), cu, layout="nbhd")
    with pytest.raises(ValueError, match="row length"):
        call(torch.zeros(40, 4, 80), kc, kc.clone(), cu)
    with pytest.raises(ValueError, match="contiguous"):
        call(torch.zeros(40, 4, 128)[..., :64], kc, kc.clone(), cu)
    with pytest.raises(ValueError, match="out must"):
        call(q, kc, kc.clone(), cu, out=torch.zeros(40, 4, 32))
    with pytest.raises(ValueError, match=r"\(H, T\)"):
        call(q, kc, kc.clone(), cu, lse=torch.zeros(40, 4))
    with pytest.raises(ValueError, match="workspace too small"):
        call(q, kc, kc.clone(), cu, workspace=torch.zeros(4))
    with pytest.raises(ValueError, match="max_pages = 2"):   # (a contiguous cache has no table to hold it against)
        call(q, kc, kc.clone(), cu, max_pages=2)
    kn = torch.zeros(40, 2, 48)
    fused = lambda k_new, v_new, **kw: call(q, kc, kc.clone(), cu, k_new=k_new, v_new=v_new, **kw)
    for a, b in ((kn, None), (None, kn)):
        with pytest.raises(ValueError, match="together"):
            fused(a, b)
    with pytest.raises(ValueError, match="3-d"):
        fused(kn[None], kn[None])
    with pytest.raises(ValueError, match="Hkv"):
        fused(torch.zeros(40, 4, 48), torch.zeros(40, 4, 48))
    with pytest.raises(TypeError, match="dtype"):
        fused(kn, kn.bfloat16())
    with pytest.raises(ValueError, match="head dim"):
        fused(torch.zeros(40, 2, 65), torch.zeros(40, 2, 65))
    with pytest.raises(ValueError, match="packed rows"):
        fused(torch.zeros(39, 2, 48), torch.zeros(39, 2, 48))
    with pytest.raises(ValueError, match="contiguous"):
        fused(torch.zeros(40, 2, 96)[..., :48], kn)
    with pytest.raises(built.FlashAttnLibraryError, match="GPU"):
        fused(kn, kn.clone())
    # a paged cache: the pool's geometry and the table, as in tests/test_paged_cpu.py
    kp = torch.zeros(6, 128, 2, 64)
    tbl = torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(ValueError, match="page_size"):
        call(q, torch.zeros(6, 64, 2, 64), torch.zeros(6, 64, 2, 64), cu, block_table=tbl)
    for bad in (tbl.long(), tbl[0], torch.zeros(3, 3, dtype=torch.int32), torch.zeros(2, 6, dtype=torch.int32)[:, ::2]):
        with pytest.raises(ValueError, match="block_table"):
            call(q, kp, kp.clone(), cu, block_table=bad)
    with pytest.raises(ValueError, match="max_pages = 4"):
        call(q, kp, kp.clone(), cu, block_table=tbl, max_pages=4)
    for kw in (dict(), dict(max_pages=3)):
        with pytest.raises(built.FlashAttnLibraryError, match="GPU"):
            call(q, kp, kp.clone(), cu, block_table=tbl, **kw)


def test_ragged_append_python_checks(built):
    import torch
    from flash_attention_minitorch_amd import device_ops

    kc, vc = torch.zeros(2, 256, 2, 64), torch.zeros(2, 256, 2, 64)
    kn = torch.zeros(40, 2, 48)
    cu = torch.zeros(3, dtype=torch.int32)
    app = device_ops.ragged_append
    with pytest.raises(ValueError, match="layout"):
        app(kn, kn, kc, vc, cu, layout="nbhd")
    with pytest.raises(ValueError, match="one shape"):
        app(kn, kn, kc, torch.zeros(2, 128, 2, 64), cu)
    with pytest.raises(TypeError, match="dtype"):
        app(kn, kn, kc, vc.bfloat16(), cu)
    with pytest.raises(TypeError, match="dtype"):
        app(kn.double(), kn.double(), kc.double(), vc.double(), cu)
    with pytest.raises(ValueError, match="3-d"):
        app(kn[None], kn[None], kc, vc, cu)
    with pytest.raises(ValueError, match="Hkv"):
        app(kn, kn, torch.zeros(2, 256, 4, 64), torch.zeros(2, 256, 4, 64), cu)
    with pytest.raises(ValueError, match="head dim"):
        app(torch.zeros(40, 2, 80), torch.zeros(40, 2, 80), kc, vc, cu)
    for bad in (None, torch.zeros(4, dtype=torch.int32), torch.zeros(3, dtype=torch.int64)):
        with pytest.raises(ValueError, match="cu_seqlens_q"):
            app(kn, kn, kc, vc, bad)
    with pytest.raises(ValueError, match="cache_seqlens"):
        app(kn, kn, kc, vc, cu, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="contiguous"):
        app(kn, kn, torch.zeros(2, 256, 2, 128)[..., :64], torch.zeros(2, 256, 2, 128)[..., :64], cu)
    with pytest.raises(ValueError, match="block_table"):
        app(kn, kn, torch.zeros(6, 128, 2, 64), torch.zeros(6, 128, 2, 64), cu, block_table=torch.zeros(3, 3, dtype=torch.int32))
    with pytest.raises(built.FlashAttnLibraryError, match="GPU"):
        app(kn, kn.clone(), kc, vc, cu, torch.zeros(2, dtype=torch.int32))


# ---- the model layer ----

def _int_tensors(rec, n):
    """The int32 tensors of n elements whose addresses the calls since the last reset took, in order, once each."""
    import torch
    seen, out = set(), []
    for t in rec.alive:
        if t.dtype == torch.int32 and t.dim() == 1 and t.numel() == n and id(t) not in seen:
            seen.add(id(t))
            out.append(t.tolist())
    return out


def test_model_ragged_calls_under_the_recorder(monkeypatch):
    """attention_stack_ragged under the recorder of tests/test_device_ops_cpu.py (CPU tensors, no library): one fused ragged call per
    layer with cu_seqlens_q the running sum of the counts and the lengths grown by them; on a PagedKVCache the pages of the sequences
    that have tokens are reserved up to the bound first, and the calls are the _paged form."""
    import torch
    from flash_attention_minitorch_amd import modules_transformer as mt
    from test_device_ops_cpu import install_recorder

    rec = install_recorder(monkeypatch)
    B, P, H, Hkv, d, cap, T = 4, 16, 4, 2, 48, 512, 160
    counts = [1, 0, 130, 5]
    g = torch.Generator().manual_seed(0)
    x, xt = (torch.randn(s, generator=g).to(torch.bfloat16) for s in ((B, P, H * d), (T, H * d)))
    wq, wk = (torch.randn(s, generator=g).to(torch.bfloat16) for s in ((H * d, H * d), (H * d, Hkv * d)))
    layers = [(wq, wk, wk, wq)] * 2
    cache = mt.KVCache(2, B, cap, H, d, torch.bfloat16, x.device, n_kv_head=Hkv)
    mt.attention_stack_prefill(x, layers, H, cache)
    rec.reset({})
    y = mt.attention_stack_ragged(xt, counts, layers, H, cache)
    calls = [c for c in rec.calls if "workspace_bytes" not in c]
    sizes = [c for c in rec.calls if "workspace_bytes" in c]
    assert len(calls) == 2 and all(c.startswith("fa_mi355x_fwd_ragged_append(") for c in calls), calls
    # ... B, H, Hkv, T, Ncap, d_new, d, layout, scale, causal, dtype, stream
    assert all(c.endswith(f",{B},{H},{Hkv},{T},{cap},48,64,1,{48 ** -0.5!r},1,1,null)") for c in calls), calls
    assert sizes and all(c == f"fa_mi355x_ragged_workspace_bytes({B},{H},{Hkv},{T},{cap},64)" for c in sizes), sizes
    assert _int_tensors(rec, B + 1) == [[0, 1, 1, 131, 136]]
    assert _int_tensors(rec, B) == [[P + c for c in counts]]
    assert y.shape == (T, H * d) and cache.length_bound == P + 130 and cache.lengths.tolist() == [P + c for c in counts]
    for bad in ([1, 0, 130], [1, 0, 130, -1], [1, 0, 130, 30]):
        with pytest.raises(ValueError, match="counts"):
            mt.attention_stack_ragged(xt, bad, layers, H, cache)
    with pytest.raises(ValueError, match="packed"):
        mt.attention_stack_ragged(xt[None], counts, layers, H, cache)
    with pytest.raises(ValueError, match="capacity"):
        mt.attention_stack_ragged(torch.zeros(400, H * d, dtype=torch.bfloat16), [0, 0, 0, cap - P - 129], layers, H, cache)

    # a paged cache: 16 + 130 rows are two pages of 128 for the three sequences that have tokens, none for the one that has not
    ps, npg = 128, 11
    cache = mt.PagedKVCache(2, B, cap, H, d, torch.bfloat16, x.device, n_kv_head=Hkv, page_size=ps, n_pages=npg)
    mt.attention_stack_prefill(x, layers, H, cache)
    assert [len(p) for p in cache.pages] == [1, 1, 1, 1]
    reserved = []
    reserve = cache.reserve
    cache.reserve = lambda n, rows=None: (reserved.append((n, list(rows))), reserve(n, rows))[1]
    rec.reset({"table": cache.block_table})
    mt.attention_stack_ragged(xt, counts, layers, H, cache)
    calls = [c for c in rec.calls if "workspace_bytes" not in c]
    assert len(calls) == 2 and all(c.startswith("fa_mi355x_fwd_ragged_append_paged(") for c in calls), calls
    # ... cu, lens, table, workspace, B, H, Hkv, T, num_pages, page_size, max_pages, d_new, d, layout, scale, causal, dtype, stream
    assert all(re.search(r",table,\w+,%d,%d,%d,%d,%d,%d,%d,48,64,1,%s,1,1,null\)$" % (B, H, Hkv, T, npg, ps, cap // ps, re.escape(repr(48 ** -0.5))),
                         c) for c in calls), calls
    assert reserved == [(P + 130, [0, 2, 3])] and [len(p) for p in cache.pages] == [2, 1, 2, 2]
    assert _int_tensors(rec, B + 1) == [[0, 1, 1, 131, 136]] and cache.length_bound == P + 130
    # the pool runs out before any call is made: 276 rows are three pages for each of four sequences, twelve of a pool of eleven
    rec.reset({"table": cache.block_table})
    with pytest.raises(RuntimeError, match="exhausted"):
        mt.attention_stack_ragged(xt, [130, 1, 1, 1], layers, H, cache)
    assert not [c for c in rec.calls if "workspace_bytes" not in c]
