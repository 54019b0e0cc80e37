"""CPU-side checks of the sliding-window entry points (include/flash_attn_mi355x_decode_window.h: the decode, extend and ragged calls
in which the query at position p admits the W keys p - W < j <= p): this file's fp64 references (used by tests/test_gpu_window.py)
against decode_reference; the nine symbols declared, exported and bound; no scratch in any kernel of the library; every bad argument
answered before any HIP call (fake non-null pointers, as in tests/test_decode_cpu.py: a launch would fail with another code); the
split policy on the window span (pure, independent of Ncap beyond the span, the unwindowed figures where the window covers the
cache, and the counts the GPU tests rely on); PagedKVCache.release_behind_window on a CPU cache; the Python checks that need no GPU
and the model layer's calls under the recorder."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_abi_cpu import _device_kernels
from test_decode_cpu import _declared, built, decode_reference  # noqa: F401  (built: the module-scoped build fixture)
from test_ragged_cpu import seq_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "flash_attn_mi355x_decode_window.h")
FAMILIES = ("decode", "extend", "ragged")
WINDOW = ([f"fa_mi355x_{f}_window_splits" for f in FAMILIES] + [f"fa_mi355x_{f}_window_workspace_bytes" for f in FAMILIES]
          + [f"fa_mi355x_fwd_{f}_window" for f in FAMILIES])


# ---- the references (used by tests/test_gpu_window.py) ----

def window_reference(q, k, v, lens, window, scale):
    """decode_reference (causal) with the window's mask: q (BH, Nq, d), k / v (BH, Ncap, d), lens (BH,).  Query i sits at
    p = len - Nq + i and admits the keys p - window < j <= p (window = 0: every j <= p).  Keys below the lowest window edge of a
    batch element, max(len - Nq - window + 1, 0), are never touched: they may hold NaN.  Returns (out (BH, Nq, d), lse (BH, Nq));
    rows with no admissible key: 0, -inf."""
    BH, Nq, d = q.shape
    Ncap = k.shape[1]
    out = np.zeros((BH, Nq, v.shape[2]))
    lse = np.full((BH, Nq), -np.inf)
    for b in range(BH):
        n = int(min(max(int(lens[b]), 0), Ncap))
        if n == 0:
            continue
        pos = n - Nq + np.arange(Nq)
        lo = max(n - Nq - window + 1, 0) if window > 0 else 0
        j = np.arange(lo, n)
        s = scale * (q[b].astype(np.float64) @ k[b, lo:n].astype(np.float64).T)   # (Nq, n - lo)
        ok = j[None, :] <= pos[:, None]
        if window > 0:
            ok &= j[None, :] > pos[:, None] - window
        s = np.where(ok, s, -np.inf)
        m = s.max(axis=1)
        fin = np.isfinite(m)
        e = np.exp(s - np.where(fin, m, 0)[:, None])
        e[~fin] = 0
        l = e.sum(axis=1)
        out[b][fin] = (e[fin] @ v[b, lo:n].astype(np.float64)) / l[fin, None]
        lse[b][fin] = m[fin] + np.log(l[fin])
    return out, lse


def ragged_window_reference(q, k, v, cu, lens, window, scale):
    """ragged_reference of tests/test_ragged_cpu.py on window_reference: q (T, H, d) packed, k / v (B, Hkv, Ncap, d).  Returns
    (out (T, H, d), lse (H, T)), NaN in the rows no sequence owns."""
    T, H, d = q.shape
    B, Hkv, Ncap, _ = k.shape
    G = H // Hkv
    out, lse = np.full((T, H, v.shape[3]), np.nan), np.full((H, T), np.nan)
    for b in range(B):
        s, e = seq_rows(cu, T, b)
        if e == s:
            continue
        n = Ncap if lens is None else lens[b]
        o, l = window_reference(q[s:e].transpose(1, 0, 2), np.repeat(k[b], G, axis=0), np.repeat(v[b], G, axis=0), np.full(H, n), window, scale)
        out[s:e] = o.transpose(1, 0, 2)
        lse[:, s:e] = l
    return out, lse


NQ_GRID = (1, 3, 33, 128, 129, 257, 400)   # the decode and extend calls of tests/test_gpu_window.py


def test_window_reference_is_decode_reference_on_the_admitted_keys():
    rng = np.random.default_rng(2)
    BH, Ncap, d = 3, 70, 16
    k, v = (rng.uniform(-1, 1, (BH, Ncap, d)) for _ in range(2))
    q = rng.uniform(-1, 1, (BH, 1, d))
    # one query: a window of W on a cache of length L is the unwindowed call on keys L - W .. L - 1 alone
    for L, W in ((70, 1), (70, 7), (64, 32), (33, 33), (50, 49)):
        got = window_reference(q, k, v, np.full(BH, L), W, 0.3)
        want = decode_reference(q, k[:, L - W:L], v[:, L - W:L], np.full(BH, W), True, 0.3)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (L, W)
    # a window that covers the cache is the causal call, for every Nq of the GPU grid; and window = 0 is
    Ncap = 520
    k, v = (rng.uniform(-1, 1, (2, Ncap, d)) for _ in range(2))
    for Nq in NQ_GRID:
        q = rng.uniform(-1, 1, (2, Nq, d))
        lens = np.array([Ncap, 300])
        want = decode_reference(q, k, v, lens, True, 0.25)
        for W in (Ncap + Nq, Ncap + Nq + 1000, 0):
            got = window_reference(q, k, v, lens, W, 0.25)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (Nq, W)
    # one row by hand: 5 queries on a length of 12, W = 4: query 2 sits at 12 - 5 + 2 = 9 and admits keys 6 .. 9; NaN below the
    # lowest edge (12 - 5 - 4 + 1 = 4) and at or past the length does not matter
    q = rng.uniform(-1, 1, (1, 5, d))
    k2, v2 = k[:1, :20].copy(), v[:1, :20].copy()
    k2[0, :4] = v2[0, :4] = k2[0, 12:] = v2[0, 12:] = np.nan
    out, lse = window_reference(q, k2, v2, [12], 4, 0.5)
    s = 0.5 * k2[0, 6:10] @ q[0, 2]
    p = np.exp(s - s.max())
    assert np.allclose(out[0, 2], p @ v2[0, 6:10] / p.sum(), atol=1e-12) and np.isclose(lse[0, 2], s.max() + np.log(p.sum()))
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(lse))
    # rows at negative positions are empty
    out, lse = window_reference(q, k[:1, :20], v[:1, :20], [3], 2, 0.5)
    assert np.all(out[0, :2] == 0) and np.all(np.isneginf(lse[0, :2])) and np.all(np.isfinite(lse[0, 2:]))
    # the ragged reference is the uniform one on each sequence's rows
    q = rng.uniform(-1, 1, (9, 4, d))
    kr, vr = (rng.uniform(-1, 1, (3, 2, 30, d)) for _ in range(2))
    out, lse = ragged_window_reference(q, kr, vr, [0, 2, 2, 7], [20, 5, 30], 6, 0.5)
    assert np.all(np.isnan(out[7:])) and np.all(np.isfinite(out[:7]))
    o, l = window_reference(q[2:7].transpose(1, 0, 2), np.repeat(kr[2], 2, axis=0), np.repeat(vr[2], 2, axis=0), np.full(4, 30), 6, 0.5)
    assert np.array_equal(out[2:7], o.transpose(1, 0, 2)) and np.array_equal(lse[:, 2:7], l)


# ---- the C ABI ----

def test_the_nine_window_symbols_are_declared_exported_and_bound(built):
    from test_lib_cpu import _ctypes_kind, _prototypes
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert '#include "flash_attn_mi355x_decode_window.h"' in open(os.path.join(ROOT, "include", "flash_attn_mi355x_decode.h")).read()
    assert sorted(set(re.findall(r"\b(fa_mi355x_\w+)\s*\(", text))) == sorted(WINDOW) == sorted(built.WINDOW_ABI)
    assert not [s for s in _declared() if "window" in s]   # (the decode header's own text declares none of them)
    protos = _prototypes("flash_attn_mi355x_decode_window.h")
    lib = built.decode()
    for s in WINDOW:
        assert hasattr(lib, s), s
        res, args = built.WINDOW_ABI[s]
        ret, kinds = protos[s]
        assert [_ctypes_kind(a) for a in args] == kinds and _ctypes_kind(res) == ret, s
        assert getattr(lib, s).argtypes == args and getattr(lib, s).restype is res, s


def test_every_kernel_of_the_decode_library_has_no_scratch(built):
    kernels = _device_kernels(built.lib_path(built.DECODE_NAME))
    assert len(kernels) > 65   # (the windowed builds are there)
    for name, scratch, vgpr in kernels:
        assert scratch == 0, (name, scratch)
        assert vgpr <= 512, (name, vgpr)


# one valid call of each family (fake non-null device pointers: a launch would fail, so a code other than the expected one shows a
# HIP call)
_ONE = 16
_GOOD = dict(q=_ONE, kn=_ONE, vn=_ONE, k=_ONE, v=_ONE, out=_ONE, lse=_ONE, cu=_ONE, lens=_ONE, table=_ONE, ws=_ONE, B=2, H=4, Hkv=2, Nq=100,
             Ncap=2048, num_pages=40, page_size=128, max_pages=16, d_new=64, d=64, layout=1, scale=0.0, causal=1, window=300, dtype=1)
_VP = ctypes.c_void_p
BAD_ARG, BAD_D = 1, 2


def _call(lib, family, **over):
    a = dict(_GOOD, **over)
    ptrs = ("q", "kn", "vn", "k", "v", "out", "lse") + (("cu",) if family == "ragged" else ()) + ("lens", "table", "ws")
    args = [_VP(a[n]) for n in ptrs] + [a[n] for n in ("B", "H", "Hkv", "Nq", "Ncap", "num_pages", "page_size", "max_pages", "d_new", "d",
                                                       "layout", "scale", "causal", "window", "dtype")] + [None]
    rc = getattr(lib, f"fa_mi355x_fwd_{family}_window")(*args)
    return rc, lib.fa_mi355x_decode_last_error().decode()


# (overrides, code, message); `slab`: table = 0, `attend`: kn = vn = 0
_SLAB, _ATTEND_ONLY = dict(table=0), dict(kn=0, vn=0)
_BAD_WINDOW = [
    (dict(window=-1), BAD_ARG, "negative"), (dict(window=-300), BAD_ARG, "negative"),
    (dict(causal=0), BAD_ARG, "causal"), (dict(causal=0, window=1), BAD_ARG, "causal"),
    (dict(window=-1, **_SLAB, **_ATTEND_ONLY), BAD_ARG, "negative"), (dict(causal=0, **_SLAB), BAD_ARG, "causal"),
]
_BAD_FAMILY = [   # the existing checks, through the new entry points: attend-only and fused, slab and paged
    (dict(q=0), BAD_ARG, "null"), (dict(k=0, **_SLAB), BAD_ARG, "null"), (dict(out=0, **_ATTEND_ONLY), BAD_ARG, "null"),
    (dict(kn=0), BAD_ARG, "null"), (dict(vn=0, **_SLAB), BAD_ARG, "null"),
    (dict(B=0), BAD_ARG, "positive"), (dict(Nq=0, **_SLAB), BAD_ARG, "positive"), (dict(Ncap=0, **_SLAB), BAD_ARG, "positive"),
    (dict(H=8, Hkv=3), BAD_ARG, "Hkv = 3"), (dict(layout=2), BAD_ARG, "layout"), (dict(dtype=5, **_SLAB), BAD_ARG, "dtype"),
    (dict(d=48, d_new=48), BAD_D, "32, 64, 128"), (dict(d=256, d_new=256, **_SLAB, **_ATTEND_ONLY), BAD_D, "32, 64, 128"),
    (dict(scale=-1.0), BAD_ARG, "softmax_scale"), (dict(scale=float("nan"), **_SLAB), BAD_ARG, "softmax_scale"),
    (dict(d_new=65), BAD_ARG, "d_new = 65"), (dict(d_new=0, **_SLAB), BAD_ARG, "d_new = 0"),
    (dict(Ncap=1 << 24, **_SLAB), BAD_ARG, "2 GiB"),
    (dict(page_size=64), BAD_ARG, "page_size"), (dict(num_pages=0), BAD_ARG, "num_pages"), (dict(max_pages=0), BAD_ARG, "max_pages"),
    (dict(max_pages=1 << 24), BAD_ARG, "max_pages * page_size"), (dict(page_size=1 << 24), BAD_ARG, "2 GiB"),
    (dict(ws=0, Ncap=65536, window=30000, **_SLAB), BAD_ARG, "workspace"),
]


def _cases():
    out = []
    for family in FAMILIES:
        out += [(family, o, c, m) for o, c, m in _BAD_WINDOW + _BAD_FAMILY]
    out += [("decode", dict(Nq=129), BAD_ARG, "Nq > 128"), ("decode", dict(Nq=129, **_SLAB, **_ATTEND_ONLY), BAD_ARG, "Nq > 128"),
            ("ragged", dict(cu=0), BAD_ARG, "cu_seqlens_q"), ("ragged", dict(cu=0, **_SLAB, **_ATTEND_ONLY), BAD_ARG, "cu_seqlens_q"),
            ("ragged", dict(ws=0, window=1), BAD_ARG, "fa_mi355x_ragged_workspace_bytes"),   # (the block map: even as one split)
            ("extend", dict(H=1 << 12, Hkv=1, Nq=1 << 13, d=32, d_new=32), BAD_ARG, "2^25")]
    return out


def _id(case):
    return case[0] + "-" + ",".join(f"{k}={v}" for k, v in case[1].items())


@pytest.mark.parametrize("family,over,code,msg", _cases(), ids=[_id(c) for c in _cases()])
def test_window_forms_reject_each_bad_argument_before_any_hip_call(built, family, over, code, msg):
    rc, err = _call(built.decode(), family, **over)
    assert rc == code and err and msg in err, (rc, err)


# ---- the policy ----

def _span(W, Ncap, Nq, block):
    """The keys one row block can need (the header's formula); Ncap where the window covers the cache (or is 0)."""
    return Ncap if W == 0 or W >= Ncap else min(Ncap, W + min(Nq, block) - 1 + 127)


def _policy(groups, target, span):
    want = max(1, -(-target // groups))
    chunk = max(256, -(-(-(-span // want)) // 256) * 256)
    return -(-span // chunk)


def _model(family, B, H, Hkv, Nq, Ncap, W):
    G = H // Hkv
    if family == "decode":
        return _policy(B * Hkv * -(-G * Nq // 32), 1024, _span(W, Ncap, Nq, 32))
    if family == "extend":
        return _policy(B * Hkv * -(-G * Nq // 128), 512, _span(W, Ncap, Nq, 128))
    return _policy(Hkv * (G * Nq // 128 + min(B, Nq)), 512, _span(W, Ncap, Nq, 128))


def _splits(lib, family, B, H, Hkv, Nq, Ncap, d, W, dt=1):
    return getattr(lib, f"fa_mi355x_{family}_window_splits")(B, H, Hkv, Nq, Ncap, d, dt, W)


def _bytes(lib, family, B, H, Hkv, Nq, Ncap, d, W):
    return getattr(lib, f"fa_mi355x_{family}_window_workspace_bytes")(B, H, Hkv, Nq, Ncap, d, W)


def _unwindowed(lib, family, B, H, Hkv, Nq, Ncap, d):
    sp = {"decode": lib.fa_mi355x_decode_splits_gqa, "extend": lib.fa_mi355x_extend_splits, "ragged": lib.fa_mi355x_ragged_splits}[family]
    ws = {"decode": lib.fa_mi355x_decode_workspace_bytes_gqa, "extend": lib.fa_mi355x_extend_workspace_bytes,
          "ragged": lib.fa_mi355x_ragged_workspace_bytes}[family]
    return sp(B, H, Hkv, Nq, Ncap, d, 1), ws(B, H, Hkv, Nq, Ncap, d)


# (B, H, Hkv, Nq or T, Ncap, d)
_SHAPES = [(32, 32, 8, 1, 32768, 128), (32, 32, 8, 512, 32768 + 512, 128), (1, 8, 1, 1, 65536, 128), (8, 2, 2, 33, 520, 64),
           (8, 8, 1, 400, 520, 32), (2, 4, 2, 161, 2048, 64), (1, 1, 1, 1, 1, 32), (3, 6, 2, 128, 100000, 64)]
_WINDOWS = (1, 33, 128, 300, 4096, 30000)


@pytest.mark.parametrize("family", FAMILIES)
def test_window_split_policy_is_pure_follows_the_span_and_sizes_the_workspace(built, family):
    lib = built.decode()
    seen = set()
    for B, H, Hkv, Nq, Ncap, d in _SHAPES:
        if family == "decode" and Nq > 128:
            continue
        full = _unwindowed(lib, family, B, H, Hkv, Nq, Ncap, d)
        for W in _WINDOWS:
            ns = [_splits(lib, family, B, H, Hkv, Nq, Ncap, d, W, dt) for dt in (0, 1, 1)]
            ws = [_bytes(lib, family, B, H, Hkv, Nq, Ncap, d, W) for _ in range(2)]
            assert ns[0] == ns[1] == ns[2] == _model(family, B, H, Hkv, Nq, Ncap, W) >= 1, (family, B, H, Hkv, Nq, Ncap, W)
            assert ws[0] == ws[1]
            part = H * ns[0] * Nq * (d + 2) * 4 * (1 if family == "ragged" else B)
            if family == "ragged":
                assert ws[0] == -(-((H // Hkv) * Nq // 128 + min(B, Nq)) * 8 // 16) * 16 + part
            else:
                assert ws[0] == (0 if ns[0] == 1 else part)
            assert ns[0] <= full[0]
            seen.add(ns[0] > 1)
            # at fixed W the figures do not depend on Ncap once the cache holds the span
            block = 32 if family == "decode" else 128
            span = W + min(Nq, block) - 1 + 127
            if Ncap > span:
                for other in (span + 1, 10 * span, Ncap + 12345):
                    assert _splits(lib, family, B, H, Hkv, Nq, other, d, W) == ns[0], (family, W, other)
                    assert _bytes(lib, family, B, H, Hkv, Nq, other, d, W) == ws[0]
        # a window that covers the cache, and no window, are the unwindowed call's figures exactly
        for W in (0, Ncap, Ncap + Nq, Ncap + Nq + 1, 2 ** 31 - 1):
            assert (_splits(lib, family, B, H, Hkv, Nq, Ncap, d, W), _bytes(lib, family, B, H, Hkv, Nq, Ncap, d, W)) == full, (family, W)
    assert seen == {True, False}
    assert _splits(lib, family, 2, 4, 2, 16, 2048, 64, -1) == 0 and _bytes(lib, family, 2, 4, 2, 16, 2048, 64, -1) == 0
    assert _splits(lib, family, 0, 4, 2, 16, 2048, 64, 5) == 0 and _bytes(lib, family, 2, 4, 3, 16, 2048, 64, 5) == 0
    # the claim the feature rests on: a window of 4096 on a cache of 32768 is split as a cache of about 4096 is, not as 32768 is
    if family == "decode":
        assert _splits(lib, family, 32, 32, 8, 1, 32768, 128, 4096) == lib.fa_mi355x_decode_splits_gqa(32, 32, 8, 1, 4096 + 127, 128, 1)


# the grid of tests/test_gpu_window.py: every window at Ncap = 520 with B = 8 lengths per call, G = 1, 4, 8 cycling with the window
NCAP = 520
WINDOWS = [1, 31, 32, 33, 127, 128, 129, 200, 300]
HEADS = [(2, 2), (4, 1), (8, 1)]
RAGGED_T = 633   # sum(COUNTS) of tests/test_gpu_ragged.py and seven unused tail rows


def grid_heads(wi, d):
    """(H, Hkv) of window WINDOWS[wi] in the case of head dim d."""
    return HEADS[(wi + d // 32) % 3]


def grid_shapes():
    """(family, B, H, Hkv, Nq or T, Ncap, dp, W) of every call of the three edge grids."""
    out = []
    for d, dp in ((32, 32), (64, 64), (128, 128), (80, 128)):
        for wi, W in enumerate(WINDOWS):
            H, Hkv = grid_heads(wi, d)
            out += [("decode", 8, H, Hkv, Nq, NCAP, dp, W) for Nq in (1, 3, 33, 128)]
            out += [("extend", 8, H, Hkv, Nq, NCAP, dp, W) for Nq in (129, 257, 400)]
            out.append(("ragged", 8, H, Hkv, RAGGED_T, NCAP, dp, W))
    return out


# the shapes of tests/test_gpu_window.py whose path depends on the policy: (family, B, H, Hkv, Nq or T, Ncap, d, W) -> splits
GPU_SPLITS = [
    (("decode", 8, 2, 2, 1, 520, 32, 128), 1),     # span 128 + 127: one chunk, written directly
    (("decode", 8, 2, 2, 1, 520, 64, 200), 2),     # span 327: two chunks of 256 keys and the combine launch
    (("decode", 8, 4, 1, 128, 520, 64, 300), 2),   # span 300 + 31 + 127
    (("extend", 8, 8, 1, 129, 520, 64, 1), 1),     # span 1 + 127 + 127
    (("extend", 8, 2, 2, 129, 520, 64, 31), 2),    # span 285
    (("extend", 8, 4, 1, 257, 520, 64, 300), 3),   # span 554, clamped to the cache's 520
    (("ragged", 8, 8, 1, 633, 520, 64, 1), 1),     # the COUNTS of tests/test_gpu_ragged.py with a tail of seven rows
    (("ragged", 8, 2, 2, 633, 520, 64, 200), 2),   # span 454
    (("ragged", 6, 4, 2, 368, 256, 64, 100), 1),   # a cache of one chunk: the bitwise comparison with the extend call
    (("decode", 2, 4, 2, 1, 1024, 32, 160), 2),    # the graphed steps of the model test: span 287
]


def test_window_split_counts_that_the_gpu_tests_rely_on(built):
    lib = built.decode()
    for (family, B, H, Hkv, Nq, Ncap, d, W), ns in GPU_SPLITS:
        for dt in (0, 1):
            assert _splits(lib, family, B, H, Hkv, Nq, Ncap, d, W, dt) == ns, (family, B, H, Hkv, Nq, Ncap, d, W)
    # the extend call on one sequence of the ragged bitwise comparison is one split as well
    assert all(_splits(lib, "extend", 1, 4, 2, nq, 256, 64, 100) == 1 for nq in (1, 33, 129, 200, 5))
    # the edge grids: the library's count is the header's formula at every call, the pinned ones are calls of the grid, and every
    # family and head dim runs both as one split and as several
    grid = grid_shapes()
    assert all(s in grid for s, _ in GPU_SPLITS[:8])
    seen = {}
    for shape in grid:
        family, B, H, Hkv, Nq, Ncap, d, W = shape
        ns = _splits(lib, *shape)
        assert ns == _model(family, B, H, Hkv, Nq, Ncap, W), shape
        seen.setdefault((family, d), set()).add(ns > 1)
    assert len(seen) == 9 and all(v == {True, False} for v in seen.values()), seen


# ---- the paged cache's release ----

def _paged(B=3, cap=1024, W=160, ps=128, n_pages=None):
    import torch
    from flash_attention_minitorch_amd import modules_transformer as mt
    return mt.PagedKVCache(1, B, cap, 2, 32, torch.float32, "cpu", page_size=ps, n_pages=n_pages, window=W)


def _consistent(cache):
    """Every page is free or owned by exactly one sequence, and the table names the owned pages behind the released slots."""
    owned = [p for own in cache.pages for p in own]
    assert len(set(owned)) == len(owned) and not set(owned) & set(cache.free) and len(owned) + len(cache.free) == cache.n_pages
    for b, own in enumerate(cache.pages):
        gone = cache.released[b]
        assert cache.block_table[b, gone:gone + len(own)].tolist() == own


def test_release_behind_window_frees_the_pages_no_later_query_can_see():
    W, ps = 160, 128
    cache = _paged(W=W, ps=ps)
    cache.reserve(520)   # five pages each
    assert [len(p) for p in cache.pages] == [5, 5, 5] and len(cache.free) == 24 - 15
    first = [own[0] for own in cache.pages]
    # page 0 (rows 0 .. 127) is out of reach once its last row 127 <= n - W, n >= 287: one row below, at, and above that; the page
    # boundary plus W itself (288)
    assert cache.release_behind_window([286, 287, 288]) == 2
    assert cache.released == [0, 1, 1] and [len(p) for p in cache.pages] == [5, 4, 4]
    assert cache.free[-2:] == [first[1], first[2]]
    _consistent(cache)
    assert cache.release_behind_window([286, 287, 288]) == 0   # (nothing twice)
    # two more pages for the third sequence: rows up to 383 are behind n = 384 + 159 = 543, not behind 542
    assert cache.release_behind_window([0, 414, 542]) == 1 and cache.released == [0, 1, 2]
    assert cache.release_behind_window([0, 415, 543]) == 2 and cache.released == [0, 2, 3]
    # a length far ahead of what the sequence owns frees what it owns and no more
    assert cache.release_behind_window([5000, 0, 0]) == 5 and cache.released == [5, 2, 3] and cache.pages[0] == []
    _consistent(cache)
    # reserve afterwards: the released leading slots stay unowned, the new pages go behind the owned ones
    before = [list(p) for p in cache.pages]
    cache.reserve(700)   # six slots: sequence 0 owns none of its first five
    assert [cache.released[b] + len(cache.pages[b]) for b in range(3)] == [6, 6, 6] and cache.released == [5, 2, 3]
    assert [len(p) for p in cache.pages] == [1, 4, 3]
    for b in range(3):
        assert cache.pages[b][:len(before[b])] == before[b]
        assert cache.block_table[b, :cache.released[b]].tolist() == [0] * cache.released[b]
    _consistent(cache)
    cache.reserve(700)   # (nothing to do)
    assert [len(p) for p in cache.pages] == [1, 4, 3]
    # the pool runs out as before, counting only what is missing behind the released slots
    small = _paged(B=2, cap=1024, W=W, ps=ps, n_pages=6)
    small.reserve(384)
    assert small.release_behind_window([300, 300]) == 2 and len(small.free) == 2
    small.reserve(512)   # one more page each: exactly the two that came back
    assert small.free == [] and [len(p) for p in small.pages] == [3, 3]
    with pytest.raises(RuntimeError, match="exhausted"):
        small.reserve(640)
    # a finished sequence starts over and owns its first slot again
    small.release(0)
    assert small.released == [0, 1] and len(small.free) == 3
    small.reserve(100, rows=[0])
    assert len(small.pages[0]) == 1 and small.block_table[0, 0].item() == small.pages[0][0]
    _consistent(small)
    # a page of 256 rows: rows 0 .. 255 are behind n = 256 + 159
    big = _paged(B=1, cap=1024, W=W, ps=256)
    big.reserve(1024)
    assert big.release_behind_window([414]) == 0 and big.release_behind_window([415]) == 1 and big.release_behind_window([1024]) == 2
    with pytest.raises(ValueError, match="one int per sequence"):
        big.release_behind_window([1, 2])
    import torch
    from flash_attention_minitorch_amd import modules_transformer as mt
    with pytest.raises(ValueError, match="window"):
        mt.PagedKVCache(1, 1, 256, 2, 32, torch.float32, "cpu").release_behind_window([300])
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="window"):
            mt.KVCache(1, 1, 256, 2, 32, torch.float32, "cpu", window=bad)


# ---- the Python layer ----

def test_window_python_checks_that_need_no_gpu(built):
    import torch
    from flash_attention_minitorch_amd import device_ops

    q, kc = torch.zeros(2, 1, 4, 64), torch.zeros(2, 256, 2, 64)
    qr, cu = torch.zeros(40, 4, 64), torch.zeros(3, dtype=torch.int32)
    calls = [lambda **kw: device_ops.flash_attn_decode(q, kc, kc.clone(), **kw), lambda **kw: device_ops.flash_attn_extend(q, kc, kc.clone(), **kw),
             lambda **kw: device_ops.flash_attn_ragged(qr, kc, kc.clone(), cu, **kw)]
    for call in calls:
        with pytest.raises(ValueError, match="causal"):
            call(window=8, causal=False)
        with pytest.raises(ValueError, match="negative"):
            call(window=-1)
        for bad in (2.0, "8", True):
            with pytest.raises(ValueError, match="int"):
                call(window=bad)
        for ok in (None, 0, 8, np.int64(8), 10 ** 6):   # past the window checks: the next complaint is the missing GPU
            with pytest.raises(built.FlashAttnLibraryError, match="GPU"):
                call(window=ok)
        with pytest.raises(built.FlashAttnLibraryError, match="GPU"):
            call(window=0, causal=False)   # (no window: nothing to object to)
    with pytest.raises(ValueError, match="workspace too small"):
        device_ops.flash_attn_ragged(qr, kc, kc.clone(), cu, window=8, workspace=torch.zeros(4))
    # the workspace queries take the window: sized by the library's windowed figures
    lib = built.decode()
    big = torch.zeros(2, 4096, 2, 64)
    for W in (None, 0, 300, 5000):
        n = lambda t: 0 if t is None else t.numel() * 4
        if W is None:
            want = (lib.fa_mi355x_decode_workspace_bytes_gqa(2, 4, 2, 1, 4096, 64), lib.fa_mi355x_extend_workspace_bytes(2, 4, 2, 1, 4096, 64),
                    lib.fa_mi355x_ragged_workspace_bytes(2, 4, 2, 40, 4096, 64))
        else:
            want = (_bytes(lib, "decode", 2, 4, 2, 1, 4096, 64, W), _bytes(lib, "extend", 2, 4, 2, 1, 4096, 64, W),
                    _bytes(lib, "ragged", 2, 4, 2, 40, 4096, 64, W))
        got = (n(device_ops.decode_workspace(q, big, window=W)), n(device_ops.extend_workspace(q, big, window=W)),
               n(device_ops.ragged_workspace(qr, big, cu, window=W)))
        assert got == want, (W, got, want)
    assert n(device_ops.decode_workspace(q, big, window=300)) < n(device_ops.decode_workspace(q, big))
    with pytest.raises(ValueError, match="negative"):
        device_ops.decode_workspace(q, big, window=-2)


def test_model_window_calls_under_the_recorder(monkeypatch):
    """The stack functions on a windowed cache under the recorder of tests/test_device_ops_cpu.py (CPU tensors, no library): every
    attention call is the family's _window entry point with the cache's window, fused with the append; a prompt goes through the
    extend call (the square forward has no window); a cache without a window makes the calls it made before."""
    import torch
    from flash_attention_minitorch_amd import modules_transformer as mt
    from test_device_ops_cpu import install_recorder

    rec = install_recorder(monkeypatch)
    B, P, H, Hkv, d, cap, W = 2, 200, 4, 2, 64, 512, 160
    g = torch.Generator().manual_seed(0)
    x = torch.randn((B, P, H * d), generator=g).to(torch.bfloat16)
    wq, wk = (torch.randn(s, generator=g).to(torch.bfloat16) for s in ((H * d, H * d), (H * d, Hkv * d)))
    layers = [(wq, wk, wk, wq)] * 2
    tail = lambda fam, n, geo: f",{B},{H},{Hkv},{n},{geo},64,64,1,0.0,1,{W},1,null)"

    cache = mt.KVCache(2, B, cap, H, d, torch.bfloat16, x.device, n_kv_head=Hkv, window=W)
    rec.reset({})
    mt.attention_stack_prefill(x, layers, H, cache)
    calls = [c for c in rec.calls if "workspace_bytes" not in c]
    assert len(calls) == 2 and all(c.startswith("fa_mi355x_fwd_extend_window(") and c.endswith(tail("extend", P, f"{cap},0,0,0")) for c in calls), calls
    assert all(",null," in c for c in calls)   # (no block table)
    assert {c for c in rec.calls if "workspace_bytes" in c} == {f"fa_mi355x_extend_window_workspace_bytes({B},{H},{Hkv},{P},{cap},64,{W})"}
    assert cache.length_bound == P
    rec.reset({})
    mt.attention_stack_step_fused(x[:, :1].contiguous(), layers, H, cache)
    mt.attention_stack_step(x[:, :3].contiguous(), layers, H, cache)
    calls = [c for c in rec.calls if "workspace_bytes" not in c]
    assert len(calls) == 4 and all(c.startswith("fa_mi355x_fwd_decode_window(") for c in calls), calls
    assert all(c.endswith(tail("decode", 1, f"{cap},0,0,0")) for c in calls[:2]) and all(c.endswith(tail("decode", 3, f"{cap},0,0,0")) for c in calls[2:])
    assert all(c.split("(")[1].split(",")[1:3] == ["null", "null"] for c in calls[2:])   # (the caller-side append: attend only)
    rec.reset({})
    mt.attention_stack_ragged(x[0, :50].contiguous(), [7, 40], layers, H, cache)
    calls = [c for c in rec.calls if "workspace_bytes" not in c]
    assert len(calls) == 2 and all(c.startswith("fa_mi355x_fwd_ragged_window(") and c.endswith(tail("ragged", 50, f"{cap},0,0,0")) for c in calls), calls

    # a paged windowed cache: the table and the pool's geometry; steps, release, and a cache without a window
    paged = mt.PagedKVCache(2, B, cap, H, d, torch.bfloat16, x.device, n_kv_head=Hkv, page_size=128, n_pages=7, window=W)
    rec.reset({"table": paged.block_table})
    mt.attention_stack_prefill_chunked(x, layers, H, paged, 150)
    calls = [c for c in rec.calls if "workspace_bytes" not in c]
    assert [c.split("(")[0] for c in calls] == ["fa_mi355x_fwd_extend_window"] * 2 + ["fa_mi355x_fwd_decode_window"] * 2, calls
    assert all(",table," in c for c in calls) and calls[0].endswith(tail("extend", 150, "0,7,128,4")) and calls[2].endswith(tail("decode", 50, "0,7,128,4"))
    assert [len(p) for p in paged.pages] == [2, 2] and paged.release_behind_window([P, P]) == 0
    assert paged.release_behind_window([300, 287]) == 2 and len(paged.free) == 5

    plain = mt.KVCache(2, B, cap, H, d, torch.bfloat16, x.device, n_kv_head=Hkv)
    rec.reset({})
    mt.attention_stack_prefill(x, layers, H, plain)
    mt.attention_stack_step_fused(x[:, :1].contiguous(), layers, H, plain)
    names = [c.split("(")[0] for c in rec.calls]
    assert not [n for n in names if "window" in n] and "fa_mi355x_fwd_decode_append" in names, names
