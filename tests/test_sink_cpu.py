"""CPU-side checks of the attention-sink entry points (include/flash_attn_mi355x_decode_sink.h: the windowed decode, extend and ragged
calls in which the query at position p admits j <= p with j > p - W or j < S): this file's fp64 references (used by
tests/test_gpu_sink.py) against window_reference, decode_reference and a row worked by hand; the nine symbols declared, exported and
bound, beside the window header's own nine; every bad argument answered before any HIP call (fake non-null pointers, as in
tests/test_window_cpu.py); the split policy on the span with its sink tiles (pure, the windowed figures at sink = 0, the unwindowed
ones where the call is the unwindowed call, independent of Ncap beyond the span, and the counts and tile walks the GPU tests rely
on); PagedKVCache.release_behind_window with sink pages on a CPU cache; the Python checks that need no GPU and the model layer's
calls under the recorder."""
import ctypes
import os
import re

import numpy as np
import pytest

from flash_attention_minitorch_amd._lib import SINK_ABI   # (the table this file holds against the header and the library)
from test_decode_cpu import _declared, built, decode_reference  # noqa: F401  (built: the module-scoped build fixture)
from test_ragged_cpu import seq_rows
from test_window_cpu import WINDOW, _policy, window_reference
from test_window_cpu import _bytes as _window_bytes, _splits as _window_splits, _unwindowed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "flash_attn_mi355x_decode_sink.h")
FAMILIES = ("decode", "extend", "ragged")
SINK = ([f"fa_mi355x_{f}_sink_splits" for f in FAMILIES] + [f"fa_mi355x_{f}_sink_workspace_bytes" for f in FAMILIES]
        + [f"fa_mi355x_fwd_{f}_sink" for f in FAMILIES])


# ---- the references (used by tests/test_gpu_sink.py) ----

def sink_reference(q, k, v, lens, window, sink, scale):
    """window_reference with the sinks' mask: q (BH, Nq, d), k / v (BH, Ncap, d), lens (BH,).  Query i sits at p = len - Nq + i and
    admits the keys j <= p with j > p - window or j < sink (window = 0: every j <= p).  The rows sink <= j < the lowest window edge
    of a batch element, max(len - Nq - window + 1, 0), are never touched: they may hold NaN.  Returns (out (BH, Nq, d),
    lse (BH, Nq)); rows with no admissible key: 0, -inf."""
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
        j = np.concatenate([np.arange(0, min(sink, lo)), np.arange(lo, n)])
        s = scale * (q[b].astype(np.float64) @ k[b][j].astype(np.float64).T)   # (Nq, keys)
        ok = j[None, :] <= pos[:, None]
        if window > 0:
            ok &= (j[None, :] > pos[:, None] - window) | (j[None, :] < sink)
        s = np.where(ok, s, -np.inf)
        m = s.max(axis=1)
        fin = np.isfinite(m)
        e = np.exp(s - np.where(fin, m, 0)[:, None])
        e[~fin] = 0
        l = e.sum(axis=1)
        out[b][fin] = (e[fin] @ v[b][j].astype(np.float64)) / l[fin, None]
        lse[b][fin] = m[fin] + np.log(l[fin])
    return out, lse


def ragged_sink_reference(q, k, v, cu, lens, window, sink, scale):
    """ragged_window_reference of tests/test_window_cpu.py on sink_reference: q (T, H, d) packed, k / v (B, Hkv, Ncap, d).  Returns
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
        o, l = sink_reference(q[s:e].transpose(1, 0, 2), np.repeat(k[b], G, axis=0), np.repeat(v[b], G, axis=0), np.full(H, n), window, sink,
                              scale)
        out[s:e] = o.transpose(1, 0, 2)
        lse[:, s:e] = l
    return out, lse


def test_sink_reference_is_the_window_reference_without_sinks_and_decode_reference_on_the_compacted_cache():
    rng = np.random.default_rng(3)
    d, Ncap = 16, 520
    k, v = (rng.uniform(-1, 1, (2, Ncap, d)) for _ in range(2))
    # S = 0: the windowed reference, array-equal, at every Nq of the GPU grids
    for Nq in (1, 3, 33, 128, 129, 257, 400):
        q = rng.uniform(-1, 1, (2, Nq, d))
        for W in (0, 1, 33, 200, Ncap + Nq):
            got, want = sink_reference(q, k, v, [Ncap, 300], W, 0, 0.25), window_reference(q, k, v, [Ncap, 300], W, 0.25)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (Nq, W)
    # one query: S sinks and a window of W on a length of L is the unwindowed call on the compacted cache, sink rows then window rows
    # (the two ranges apart, adjacent, overlapping, and a length below S)
    q = rng.uniform(-1, 1, (2, 1, d))
    for L, W, S in ((520, 33, 4), (520, 1, 200), (300, 100, 200), (300, 100, 250), (150, 33, 200), (70, 7, 1), (5, 3, 4)):
        rows = np.concatenate([np.arange(0, min(S, max(L - W, 0))), np.arange(max(L - W, 0), L)])
        got = sink_reference(q, k, v, np.full(2, L), W, S, 0.3)
        want = decode_reference(q, k[:, rows], v[:, rows], np.full(2, len(rows)), True, 0.3)
        assert np.abs(got[0] - want[0]).max() < 1e-12 and np.abs(got[1] - want[1]).max() < 1e-12, (L, W, S)
    # one row by hand: 5 queries on a length of 30, W = 4, S = 3: query 2 sits at 30 - 5 + 2 = 27 and admits keys 0, 1, 2 and
    # 24 .. 27; NaN in the rows 3 .. 21 between the sinks and the lowest edge (30 - 5 - 4 + 1 = 22) and at or past the length
    q = rng.uniform(-1, 1, (1, 5, d))
    k2, v2 = k[:1, :40].copy(), v[:1, :40].copy()
    k2[0, 3:22] = v2[0, 3:22] = k2[0, 30:] = v2[0, 30:] = np.nan
    out, lse = sink_reference(q, k2, v2, [30], 4, 3, 0.5)
    rows = [0, 1, 2, 24, 25, 26, 27]
    s = 0.5 * k2[0, rows] @ q[0, 2]
    p = np.exp(s - s.max())
    assert np.allclose(out[0, 2], p @ v2[0, rows] / p.sum(), atol=1e-12) and np.isclose(lse[0, 2], s.max() + np.log(p.sum()))
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(lse))
    # a key that is a sink and inside the window counts once: S = 28 covers the window of query 2 but not key 28, 29
    out2, lse2 = sink_reference(q, k[:1, :40], v[:1, :40], [30], 4, 28, 0.5)
    full = decode_reference(q, k[:1, :40], v[:1, :40], [30], True, 0.5)
    assert np.abs(out2 - full[0]).max() < 1e-12 and np.abs(lse2 - full[1]).max() < 1e-12
    # rows at negative positions are empty
    out, lse = sink_reference(q, k[:1, :40], v[:1, :40], [3], 2, 1, 0.5)
    assert np.all(out[0, :2] == 0) and np.all(np.isneginf(lse[0, :2])) and np.all(np.isfinite(lse[0, 2:]))
    # the ragged reference is the uniform one on each sequence's rows
    q = rng.uniform(-1, 1, (9, 4, d))
    kr, vr = (rng.uniform(-1, 1, (3, 2, 30, d)) for _ in range(2))
    out, lse = ragged_sink_reference(q, kr, vr, [0, 2, 2, 7], [20, 5, 30], 6, 2, 0.5)
    assert np.all(np.isnan(out[7:])) and np.all(np.isfinite(out[:7]))
    o, l = sink_reference(q[2:7].transpose(1, 0, 2), np.repeat(kr[2], 2, axis=0), np.repeat(vr[2], 2, axis=0), np.full(4, 30), 6, 2, 0.5)
    assert np.array_equal(out[2:7], o.transpose(1, 0, 2)) and np.array_equal(lse[:, 2:7], l)


# ---- the C ABI ----

def test_the_nine_sink_symbols_are_declared_exported_and_bound(built):
    from test_lib_cpu import _ctypes_kind, _prototypes
    include = os.path.join(ROOT, "include")
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    main = open(os.path.join(include, "flash_attn_mi355x_decode.h")).read()
    assert main.rstrip().endswith("#endif /* FLASH_ATTN_MI355X_DECODE_H */")
    assert '#include "flash_attn_mi355x_decode_sink.h"' in main[main.index('#include "flash_attn_mi355x_decode_fp8.h"'):]
    assert sorted(set(re.findall(r"\b(fa_mi355x_\w+)\s*\(", text))) == sorted(SINK) == sorted(built.SINK_ABI) == sorted(SINK_ABI)
    assert not [s for s in SINK if "window" in s]
    assert not [s for s in _declared() if "sink" in s]   # (the decode header's own text declares none of them)
    # the window header still declares exactly its nine
    wtext = re.sub(r"/\*.*?\*/", "", open(os.path.join(include, "flash_attn_mi355x_decode_window.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(fa_mi355x_\w+)\s*\(", wtext))) == sorted(WINDOW) == sorted(built.WINDOW_ABI)
    protos = _prototypes("flash_attn_mi355x_decode_sink.h")
    wprotos = _prototypes("flash_attn_mi355x_decode_window.h")
    lib = built.decode()
    for s in SINK:
        assert hasattr(lib, s), s
        res, args = built.SINK_ABI[s]
        ret, kinds = protos[s]
        assert [_ctypes_kind(a) for a in args] == kinds and _ctypes_kind(res) == ret, s
        assert getattr(lib, s).argtypes == args and getattr(lib, s).restype is res, s
        # the windowed form's arguments with one more int
        wret, wkinds = wprotos[s.replace("_sink", "_window")]
        assert ret == wret and len(kinds) == len(wkinds) + 1 and sorted(kinds) == sorted(wkinds + ["int"]), s
    # `int sink` stands directly after `int window`
    flat = re.sub(r"\s+", " ", text)
    assert flat.count("int window, int sink") == 9


# one valid call of each family (fake non-null device pointers: a launch would fail, so a code other than the expected one shows a
# HIP call)
_ONE = 16
_GOOD = dict(q=_ONE, kn=_ONE, vn=_ONE, k=_ONE, v=_ONE, out=_ONE, lse=_ONE, cu=_ONE, lens=_ONE, table=_ONE, ws=_ONE, B=2, H=4, Hkv=2, Nq=100,
             Ncap=2048, num_pages=40, page_size=128, max_pages=16, d_new=64, d=64, layout=1, scale=0.0, causal=1, window=300, sink=4, dtype=1)
_VP = ctypes.c_void_p
BAD_ARG, BAD_D = 1, 2


def _call(lib, family, **over):
    a = dict(_GOOD, **over)
    ptrs = ("q", "kn", "vn", "k", "v", "out", "lse") + (("cu",) if family == "ragged" else ()) + ("lens", "table", "ws")
    args = [_VP(a[n]) for n in ptrs] + [a[n] for n in ("B", "H", "Hkv", "Nq", "Ncap", "num_pages", "page_size", "max_pages", "d_new", "d",
                                                       "layout", "scale", "causal", "window", "sink", "dtype")] + [None]
    rc = getattr(lib, f"fa_mi355x_fwd_{family}_sink")(*args)
    return rc, lib.fa_mi355x_decode_last_error().decode()


_SLAB, _ATTEND_ONLY = dict(table=0), dict(kn=0, vn=0)
_BAD_SINK = [
    (dict(sink=-1), BAD_ARG, "sink must not be negative"), (dict(sink=-4, **_SLAB, **_ATTEND_ONLY), BAD_ARG, "sink must not be negative"),
    (dict(sink=-1, window=0), BAD_ARG, "sink must not be negative"),
    (dict(window=-1), BAD_ARG, "window must not be negative"), (dict(window=-300, **_SLAB), BAD_ARG, "window must not be negative"),
    (dict(causal=0), BAD_ARG, "causal"), (dict(causal=0, sink=1, window=1, **_SLAB), BAD_ARG, "causal"),
    (dict(causal=0, sink=5000), BAD_ARG, "causal"),   # (the window's own check, whatever the sinks cover)
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
    (dict(ws=0, Ncap=65536, window=100, sink=30000, **_SLAB), BAD_ARG, "workspace"),   # (the sink tiles alone make it several splits)
]
_TWO_FAULTS = [   # which error wins: the prelude (sink, window, causal), the page geometry, the attention's checks in order, the append's
    (dict(window=-1, q=0), BAD_ARG, "window must not be negative"), (dict(sink=-1, window=-1), BAD_ARG, "sink must not be negative"),
    (dict(causal=0, page_size=64), BAD_ARG, "causal"), (dict(page_size=64, q=0), BAD_ARG, "page_size = 64"),
    (dict(num_pages=0, B=0), BAD_ARG, "num_pages"), (dict(max_pages=1 << 24, q=0), BAD_ARG, "max_pages * page_size"),
    (dict(H=8, Hkv=3, B=0), BAD_ARG, "must be positive"), (dict(layout=2, dtype=5), BAD_ARG, "unknown dtype"),
    (dict(q=0, d_new=65), BAD_ARG, "null pointer argument"), (dict(d=48, d_new=48, kn=0), BAD_D, "32, 64, 128"),
    (dict(scale=-1.0, d=48, d_new=48), BAD_D, "32, 64, 128"),
]


def _cases():
    out = []
    for family in FAMILIES:
        out += [(family, o, c, m) for o, c, m in _BAD_SINK + _BAD_FAMILY + _TWO_FAULTS]
        # (the attention's last check in front of the append's first)
        out.append((family, dict(ws=0, Ncap=65536, window=30000, table=0, d_new=65), BAD_ARG, f"fa_mi355x_{family}_workspace_bytes"))
    out += [("decode", dict(Nq=129, layout=2), BAD_ARG, "Nq > 128"), ("ragged", dict(cu=0, q=0), BAD_ARG, "null pointer argument"),
            ("ragged", dict(cu=0, d=48, d_new=48), BAD_ARG, "null cu_seqlens_q"),
            ("ragged", dict(ws=0, d_new=65), BAD_ARG, "fa_mi355x_ragged_workspace_bytes")]
    out += [("decode", dict(Nq=129), BAD_ARG, "Nq > 128"), ("decode", dict(Nq=129, **_SLAB, **_ATTEND_ONLY), BAD_ARG, "Nq > 128"),
            ("ragged", dict(cu=0), BAD_ARG, "cu_seqlens_q"), ("ragged", dict(cu=0, **_SLAB, **_ATTEND_ONLY), BAD_ARG, "cu_seqlens_q"),
            ("ragged", dict(ws=0, window=1, sink=1), BAD_ARG, "fa_mi355x_ragged_workspace_bytes"),   # (the block map: even as one split)
            ("extend", dict(H=1 << 12, Hkv=1, Nq=1 << 13, d=32, d_new=32), BAD_ARG, "2^25")]
    return out


def _id(case):
    return case[0] + "-" + ",".join(f"{k}={v}" for k, v in case[1].items())


@pytest.mark.parametrize("family,over,code,msg", _cases(), ids=[_id(c) for c in _cases()])
def test_sink_forms_reject_each_bad_argument_before_any_hip_call(built, family, over, code, msg):
    rc, err = _call(built.decode(), family, **over)
    assert rc == code and err and msg in err, (rc, err)


# ---- the policy ----

def _span(W, S, Ncap, Nq, block):
    """The keys one row block can need (the header's formula); Ncap in the cases that are the unwindowed call."""
    if W == 0 or W >= Ncap or S >= Ncap:
        return Ncap
    return min(Ncap, -(-S // 128) * 128 + W + min(Nq, block) - 1 + 127)


def _model(family, B, H, Hkv, Nq, Ncap, W, S):
    G = H // Hkv
    if family == "decode":
        return _policy(B * Hkv * -(-G * Nq // 32), 1024, _span(W, S, Ncap, Nq, 32))
    if family == "extend":
        return _policy(B * Hkv * -(-G * Nq // 128), 512, _span(W, S, Ncap, Nq, 128))
    return _policy(Hkv * (G * Nq // 128 + min(B, Nq)), 512, _span(W, S, Ncap, Nq, 128))


def _splits(lib, family, B, H, Hkv, Nq, Ncap, d, W, S, dt=1):
    return getattr(lib, f"fa_mi355x_{family}_sink_splits")(B, H, Hkv, Nq, Ncap, d, dt, W, S)


def _bytes(lib, family, B, H, Hkv, Nq, Ncap, d, W, S):
    return getattr(lib, f"fa_mi355x_{family}_sink_workspace_bytes")(B, H, Hkv, Nq, Ncap, d, W, S)


# (B, H, Hkv, Nq or T, Ncap, d)
_SHAPES = [(32, 32, 8, 1, 32768, 128), (32, 32, 8, 512, 32768 + 512, 128), (1, 8, 1, 1, 65536, 128), (8, 2, 2, 33, 520, 64),
           (8, 8, 1, 400, 520, 32), (2, 4, 2, 161, 2048, 64), (1, 1, 1, 1, 1, 32), (3, 6, 2, 128, 100000, 64)]
_WINDOWS = (1, 33, 128, 300, 4096, 30000)
_SINKS = (1, 4, 128, 129, 1000, 20000)


@pytest.mark.parametrize("family", FAMILIES)
def test_sink_split_policy_is_pure_follows_the_span_and_sizes_the_workspace(built, family):
    lib = built.decode()
    seen = set()
    for B, H, Hkv, Nq, Ncap, d in _SHAPES:
        if family == "decode" and Nq > 128:
            continue
        full = _unwindowed(lib, family, B, H, Hkv, Nq, Ncap, d)
        for W in _WINDOWS:
            # no sinks: the window functions
            assert _splits(lib, family, B, H, Hkv, Nq, Ncap, d, W, 0) == _window_splits(lib, family, B, H, Hkv, Nq, Ncap, d, W)
            assert _bytes(lib, family, B, H, Hkv, Nq, Ncap, d, W, 0) == _window_bytes(lib, family, B, H, Hkv, Nq, Ncap, d, W)
            for S in _SINKS:
                ns = [_splits(lib, family, B, H, Hkv, Nq, Ncap, d, W, S, dt) for dt in (0, 1, 1)]
                ws = [_bytes(lib, family, B, H, Hkv, Nq, Ncap, d, W, S) for _ in range(2)]
                assert ns[0] == ns[1] == ns[2] == _model(family, B, H, Hkv, Nq, Ncap, W, S) >= 1, (family, B, H, Hkv, Nq, Ncap, W, S)
                assert ws[0] == ws[1]
                part = H * ns[0] * Nq * (d + 2) * 4 * (1 if family == "ragged" else B)
                if family == "ragged":
                    assert ws[0] == -(-((H // Hkv) * Nq // 128 + min(B, Nq)) * 8 // 16) * 16 + part
                else:
                    assert ws[0] == (0 if ns[0] == 1 else part)
                seen.add(ns[0] > 1)   # (the count is not monotonic in the span: a longer span can take a longer chunk)
                # at fixed W and S the figures do not depend on Ncap once the cache holds the span
                span = -(-S // 128) * 128 + W + min(Nq, 32 if family == "decode" else 128) - 1 + 127
                if Ncap > span:
                    for other in (span + 1, 10 * span, Ncap + 12345):
                        assert _splits(lib, family, B, H, Hkv, Nq, other, d, W, S) == ns[0], (family, W, S, other)
                        assert _bytes(lib, family, B, H, Hkv, Nq, other, d, W, S) == ws[0]
        # no window, a window that covers the cache, or sinks that do: the unwindowed call's figures exactly
        for W, S in [(W, S) for W in (0, Ncap, Ncap + Nq, 2 ** 31 - 1) for S in (0, 1, 4, 200, Ncap, 2 ** 31 - 1)] + \
                    [(W, S) for W in (1, 33, 300) for S in (Ncap, Ncap + 1, 2 ** 31 - 1)]:
            assert (_splits(lib, family, B, H, Hkv, Nq, Ncap, d, W, S), _bytes(lib, family, B, H, Hkv, Nq, Ncap, d, W, S)) == full, (family, W, S)
    assert seen == {True, False}
    for W, S in ((-1, 4), (5, -1), (-1, -1), (0, -1)):
        assert _splits(lib, family, 2, 4, 2, 16, 2048, 64, W, S) == 0 and _bytes(lib, family, 2, 4, 2, 16, 2048, 64, W, S) == 0
    assert _splits(lib, family, 0, 4, 2, 16, 2048, 64, 5, 4) == 0 and _bytes(lib, family, 2, 4, 3, 16, 2048, 64, 5, 4) == 0
    # one sink tile beside a window of 4096 on a cache of 32768: split as a cache of 4096 + 128 + 127 keys is
    if family == "decode":
        assert _splits(lib, family, 32, 32, 8, 1, 32768, 128, 4096, 4) == lib.fa_mi355x_decode_splits_gqa(32, 32, 8, 1, 4096 + 255, 128, 1)


# ---- the grids of tests/test_gpu_sink.py ----
NCAP = 520
SINKS = [1, 4, 127, 128, 129, 200]
WINDOWS = [1, 33, 128, 200]
HEADS = [(2, 2), (4, 1), (8, 1)]
PAIRS = [(S, W) for S in SINKS for W in WINDOWS]   # the cross product, in this order
DECODE_NQ, EXTEND_NQ = (1, 3, 33, 128), (1, 129, 257, 400)
RAGGED_T = 633   # sum(COUNTS) of tests/test_gpu_ragged.py and seven unused tail rows
DIMS = ((32, 32), (64, 64), (128, 128), (80, 128))   # (d, dp)


def grid_lens(S, W):
    """Per-batch lengths of one call: empty, one key, the sinks alone, around the point where the first key falls between the sinks
    and the window (S + W - 1, S + W, S + W + 1), a length whose last tile is partial, full, and out of range (clamped)."""
    return [0, 1, S, S + W - 1, S + W, S + W + 1, 300, NCAP, 9999]


def grid_pairs(d, nq_index):
    """The (pair index, S, W) of the case of head dim d and the nq_index-th Nq: a rotating half of the cross product (a checkerboard
    over the S and W indices that shifts with the Nq and with d), so that the four Nq of a family cover every pair twice."""
    return [(pi, S, W) for pi, (S, W) in enumerate(PAIRS) if (pi // len(WINDOWS) + pi % len(WINDOWS) + nq_index + d // 32) % 2 == 0]


def grid_heads(pi, d):
    """(H, Hkv) of pair PAIRS[pi] in the case of head dim d: G cycles through 1, 4, 8."""
    return HEADS[(pi + d // 32) % 3]


def grid_shapes():
    """(family, B, H, Hkv, Nq or T, Ncap, dp, W, S) of every call of the three edge grids."""
    out = []
    for d, dp in DIMS:
        for family, nqs in (("decode", DECODE_NQ), ("extend", EXTEND_NQ)):
            for ni, Nq in enumerate(nqs):
                for pi, S, W in grid_pairs(d, ni):
                    H, Hkv = grid_heads(pi, d)
                    out.append((family, len(grid_lens(S, W)), H, Hkv, Nq, NCAP, dp, W, S))
        for pi, S, W in grid_pairs(d, 0) + grid_pairs(d, 1):
            H, Hkv = grid_heads(pi, d)
            out.append(("ragged", 8, H, Hkv, RAGGED_T, NCAP, dp, W, S))
    return out


def block_walk(n, nq, i0, W, S, chunk):
    """The super tiles a row block walks, split by split, as the header describes it: n the (clamped) length, nq the new tokens, i0
    the query index of the block's first row.  Returns a list (one entry per non-empty split) of lists of tile starts."""
    wedge = max(n - nq + i0 - W + 1, 0)
    lo = wedge // 128 * 128
    vs = min(-(-S // 128) * 128, lo)
    tiles = list(range(0, vs, 128)) + list(range(lo, n, 128))
    per = chunk // 128
    return [tiles[i:i + per] for i in range(0, len(tiles), per)]


# the shapes of tests/test_gpu_sink.py whose path depends on the policy: (family, B, H, Hkv, Nq or T, Ncap, d, W, S) -> splits
GPU_SPLITS = [
    (("decode", 9, 8, 1, 1, 520, 32, 1, 4), 1),      # span 128 + 1 + 127 = 256: one chunk, written directly
    (("decode", 9, 4, 1, 1, 520, 64, 33, 4), 2),     # span 288: the jump 0 -> 384 inside the first chunk
    (("decode", 9, 2, 2, 1, 520, 32, 1, 200), 2),    # span 384: the jump 128 -> 512 on the chunk boundary
    (("extend", 9, 8, 1, 1, 520, 32, 1, 4), 1),
    (("extend", 9, 4, 1, 257, 520, 64, 33, 4), 2),   # span 128 + 33 + 127 + 127 = 415
    (("extend", 9, 2, 2, 400, 520, 32, 200, 200), 3),  # span 710, clamped to the cache's 520
    (("ragged", 8, 4, 1, 633, 520, 64, 33, 4), 2),
    (("ragged", 8, 8, 1, 633, 520, 128, 200, 129), 3),
    (("ragged", 6, 4, 2, 368, 256, 64, 100, 4), 1),  # a cache of one chunk: the bitwise comparison with the extend call
    (("decode", 2, 4, 2, 1, 1024, 32, 160, 4), 2),   # the graphed steps of the model test: span 128 + 160 + 127 = 415
]


def test_sink_split_counts_and_tile_walks_that_the_gpu_tests_rely_on(built):
    lib = built.decode()
    for (family, B, H, Hkv, Nq, Ncap, d, W, S), ns in GPU_SPLITS:
        for dt in (0, 1):
            assert _splits(lib, family, B, H, Hkv, Nq, Ncap, d, W, S, dt) == ns, (family, B, H, Hkv, Nq, Ncap, d, W, S)
    # the extend call on one sequence of the ragged bitwise comparison is one split as well
    assert all(_splits(lib, "extend", 1, 4, 2, nq, 256, 64, 100, 4) == 1 for nq in (1, 33, 129, 200, 5))
    # the edge grids: the library's count is the header's formula at every call, the pinned ones are calls of the grid, every pair
    # of the cross product is run by every family, and decode and extend run both as one split and as several
    grid = grid_shapes()
    assert all(s in grid for s, _ in GPU_SPLITS[:8])
    seen, pairs = {}, {}
    for shape in grid:
        family, B, H, Hkv, Nq, Ncap, d, W, S = shape
        ns = _splits(lib, *shape)
        assert ns == _model(family, B, H, Hkv, Nq, Ncap, W, S), shape
        seen.setdefault(family, set()).add(ns > 1)
        pairs.setdefault(family, set()).add((S, W))
    assert seen["decode"] == seen["extend"] == {True, False} and all(len(p) == len(PAIRS) for p in pairs.values()), seen
    # (every ragged call of the grid is several splits: 8 sequences and 633 rows make the chunk 256 and the span is at least 382;
    # the ragged family runs as one split in the Ncap = 256 comparison above)
    assert seen["ragged"] == {True}
    # the cases the grid must hit, from the walk of the header
    decode1 = [s for s in grid if s[0] == "decode" and s[4] == 1]
    assert ("decode", 9, 4, 1, 1, 520, 64, 33, 4) in decode1 and 520 in grid_lens(4, 33)
    assert block_walk(520, 1, 0, 33, 4, 256) == [[0, 384], [512]]          # a jump inside a chunk
    assert any(s[7:] == (1, 200) for s in decode1) and 520 in grid_lens(200, 1)
    assert block_walk(520, 1, 0, 1, 200, 256) == [[0, 128], [512]]         # a jump on a chunk boundary
    assert any(s[7:] == (128, 128) for s in decode1)
    assert block_walk(300, 1, 0, 128, 128, 256) == [[0, 128], [256]]       # adjacent ranges: lo = 128 = the end of the sink tile
    assert any(s[7:] == (128, 200) for s in decode1)
    assert block_walk(300, 1, 0, 128, 200, 256) == [[0, 128], [256]]       # overlapping: the tile at lo = 128 straddles S = 200
    assert block_walk(201, 1, 0, 1, 200, 256) == [[0], [128]] or block_walk(201, 1, 0, 1, 200, 256) == [[0, 128]]
    for S, W in PAIRS:
        lens = grid_lens(S, W)
        assert lens[2] == S and 1 in lens and (S == 1 or 1 < S)            # a length below S (1, for every S > 1) and S itself
    assert all(any(n - nq < 0 for n in grid_lens(4, 33)) for nq in (3, 33, 128, 129, 257, 400))   # rows at negative positions
    assert {s[4] for s in grid if s[0] == "decode"} == {1, 3, 33, 128} and {s[4] for s in grid if s[0] == "extend"} == {1, 129, 257, 400}


# ---- the paged cache's release ----

def _paged(B=3, cap=1024, W=160, S=4, ps=128, n_pages=None):
    import torch
    from flash_attention_minitorch_amd import modules_transformer as mt
    return mt.PagedKVCache(1, B, cap, 2, 32, torch.float32, "cpu", page_size=ps, n_pages=n_pages, window=W, sink=S)


def _consistent(cache):
    """Every page is free or owned by exactly one sequence, and the table names the owned pages: the sink slots first, then the slots
    behind the released ones."""
    owned = [p for own in cache.pages for p in own]
    assert len(set(owned)) == len(owned) and not set(owned) & set(cache.free) and len(owned) + len(cache.free) == cache.n_pages
    keep = cache.sink_pages
    for b, own in enumerate(cache.pages):
        gone = cache.released[b]
        assert gone == 0 or len(own) >= keep
        assert cache.block_table[b, :min(keep, len(own))].tolist() == own[:keep]
        assert cache.block_table[b, keep + gone:gone + len(own)].tolist() == own[keep:]


def test_release_behind_window_keeps_the_sink_pages():
    W, ps = 160, 128
    cache = _paged(W=W, S=4, ps=ps)
    assert cache.sink_pages == 1 and cache.windowing() == dict(window=W, sink=4)
    cache.reserve(520)   # five pages each
    first = [list(own) for own in cache.pages]
    # the worked case: at n = 400 only slot 0 is behind the window, and it is kept; at n = 416 slot 1 is freed, never slot 0
    assert cache.release_behind_window([400, 414, 416]) == 1
    assert cache.released == [0, 0, 1] and [len(p) for p in cache.pages] == [5, 5, 4]
    assert cache.pages[2] == [first[2][0]] + first[2][2:] and cache.free[-1] == first[2][1]
    _consistent(cache)
    assert cache.release_behind_window([400, 414, 416]) == 0   # (nothing twice)
    assert cache.release_behind_window([416, 543, 544]) == 4 and cache.released == [1, 2, 2]
    assert [own[0] for own in cache.pages] == [f[0] for f in first]   # (slot 0 is still every sequence's first page)
    # a length far ahead of what the sequence owns frees what it owns behind the sink page and no more
    assert cache.release_behind_window([5000, 0, 0]) == 3 and cache.released == [4, 2, 2] and cache.pages[0] == [first[0][0]]
    _consistent(cache)
    # reserve afterwards: the released slots stay unowned, the new pages go behind the owned ones
    before = [list(p) for p in cache.pages]
    cache.reserve(700)   # six slots
    assert [cache.released[b] + len(cache.pages[b]) for b in range(3)] == [6, 6, 6] and cache.released == [4, 2, 2]
    for b in range(3):
        assert cache.pages[b][:len(before[b])] == before[b]
        assert cache.block_table[b, 0].item() == first[b][0]
        assert cache.block_table[b, 1:1 + cache.released[b]].tolist() == [0] * cache.released[b]
    _consistent(cache)
    cache.reserve(700)   # (nothing to do)
    assert [len(p) for p in cache.pages] == [2, 4, 4]
    # the pool runs out as before, counting only what is missing
    small = _paged(B=2, cap=1024, W=W, S=4, ps=ps, n_pages=8)
    small.reserve(512)
    assert small.release_behind_window([420, 420]) == 2 and len(small.free) == 2
    small.reserve(640)   # one more page each: exactly the two that came back
    assert small.free == [] and [len(p) for p in small.pages] == [4, 4] and small.released == [1, 1]
    with pytest.raises(RuntimeError, match="exhausted"):
        small.reserve(768)
    # a finished sequence starts over and owns its first slots again
    small.release(0)
    assert small.released == [0, 1] and len(small.free) == 4 and small.pages[0] == []
    small.reserve(300, rows=[0])
    assert len(small.pages[0]) == 3 and small.block_table[0, :3].tolist() == small.pages[0]
    _consistent(small)
    # S spanning two pages: slots 0 and 1 stay; slot 2 (rows 256 .. 383) is behind n = 384 + 159
    two = _paged(B=1, cap=1024, W=W, S=129, ps=ps)
    assert two.sink_pages == 2
    two.reserve(1024)
    own = list(two.pages[0])
    assert two.release_behind_window([542]) == 0 and two.release_behind_window([543]) == 1 and two.released == [1]
    assert two.pages[0] == own[:2] + own[3:]
    assert two.release_behind_window([1024]) == 3 and two.pages[0] == own[:2] + own[6:]
    _consistent(two)
    # a sequence shorter than its sinks owns fewer pages than sink_pages and releases nothing
    short = _paged(B=1, cap=1024, W=1, S=300, ps=ps)
    short.reserve(100)
    assert short.sink_pages == 3 and short.release_behind_window([100]) == 0 and len(short.pages[0]) == 1
    short.reserve(700)
    assert short.release_behind_window([700]) == 2 and short.released == [2] and len(short.pages[0]) == 4
    _consistent(short)
    # a page of 256 rows: S = 4 keeps slot 0; slot 1 (rows 256 .. 511) is behind n = 512 + 159; S = 257 keeps two slots
    big = _paged(B=1, cap=1024, W=W, S=4, ps=256)
    big.reserve(1024)
    assert big.sink_pages == 1 and big.release_behind_window([670]) == 0 and big.release_behind_window([671]) == 1
    assert big.release_behind_window([1024]) == 1 and big.released == [2] and len(big.pages[0]) == 2
    _consistent(big)
    assert _paged(B=1, W=W, S=257, ps=256).sink_pages == 2 and _paged(B=1, W=W, S=256, ps=256).sink_pages == 1
    # S = 0 (and None) is the cache without sinks
    for S in (0, None):
        none = _paged(B=1, W=W, S=S)
        none.reserve(520)
        assert none.sink is None and none.sink_pages == 0 and none.windowing() == dict(window=W)
        assert none.release_behind_window([287]) == 1 and none.released == [1]
    import torch
    from flash_attention_minitorch_amd import modules_transformer as mt
    for cls in (mt.KVCache, mt.PagedKVCache):
        with pytest.raises(ValueError, match="window"):
            cls(1, 1, 256, 2, 32, torch.float32, "cpu", sink=4)
        for bad in (-3, 2.5, True, "4"):
            with pytest.raises(ValueError, match="sink"):
                cls(1, 1, 256, 2, 32, torch.float32, "cpu", window=64, sink=bad)
        if hasattr(torch, "float8_e4m3fn"):
            with pytest.raises(ValueError, match="window"):   # (the window's refusal on an fp8 cache)
                cls(1, 1, 256, 2, 32, torch.bfloat16, "cpu", window=64, sink=4, kv_dtype=torch.float8_e4m3fn)
    slab = mt.KVCache(1, 1, 256, 2, 32, torch.float32, "cpu", window=64, sink=4)
    assert slab.windowing() == dict(window=64, sink=4)
    assert mt.KVCache(1, 1, 256, 2, 32, torch.float32, "cpu", window=64, sink=0).windowing() == dict(window=64)


# ---- the Python layer ----

def test_sink_python_checks_that_need_no_gpu(built):
    import torch
    from flash_attention_minitorch_amd import device_ops

    q, kc = torch.zeros(2, 1, 4, 64), torch.zeros(2, 256, 2, 64)
    qr, cu = torch.zeros(40, 4, 64), torch.zeros(3, dtype=torch.int32)
    calls = [lambda **kw: device_ops.flash_attn_decode(q, kc, kc.clone(), **kw), lambda **kw: device_ops.flash_attn_extend(q, kc, kc.clone(), **kw),
             lambda **kw: device_ops.flash_attn_ragged(qr, kc, kc.clone(), cu, **kw)]
    for call in calls:
        with pytest.raises(ValueError, match="needs window"):
            call(sink=4)
        with pytest.raises(ValueError, match="negative"):
            call(window=8, sink=-1)
        with pytest.raises(ValueError, match="causal"):
            call(window=8, sink=4, causal=False)
        for bad in (2.0, "8", True):
            with pytest.raises(ValueError, match="sink must be None or an int"):
                call(window=8, sink=bad)
        for ok in (None, 0, 4, np.int64(4), 10 ** 6):   # past the checks: the next complaint is the missing GPU
            with pytest.raises(built.FlashAttnLibraryError, match="GPU"):
                call(window=8, sink=ok)
        with pytest.raises(built.FlashAttnLibraryError, match="GPU"):
            call(sink=0)   # (no sinks: no window needed)
        with pytest.raises(built.FlashAttnLibraryError, match="GPU"):
            call(window=0, sink=4)   # (an int window: the sink entry point, which makes it the unwindowed call)
    with pytest.raises(ValueError, match="workspace too small"):
        device_ops.flash_attn_ragged(qr, kc, kc.clone(), cu, window=8, sink=4, workspace=torch.zeros(4))
    if hasattr(torch, "float8_e4m3fn"):
        k8 = torch.zeros(2, 256, 2, 64, dtype=torch.float8_e4m3fn)
        qb = q.to(torch.bfloat16)
        for fn in (device_ops.flash_attn_decode, device_ops.flash_attn_extend):
            with pytest.raises(ValueError, match="a sliding window on an fp8 cache is not built"):
                fn(qb, k8, k8.clone(), window=8, sink=4)
            with pytest.raises(ValueError, match="window"):
                fn(qb, k8, k8.clone(), sink=4)
    # the workspace queries take the sinks: sized by the library's figures; None and 0 are the windowed figures
    lib = built.decode()
    big = torch.zeros(2, 4096, 2, 64)
    n = lambda t: 0 if t is None else t.numel() * 4
    for W, S in ((300, 4), (300, 1000), (5000, 4), (300, 5000), (0, 4)):
        want = (_bytes(lib, "decode", 2, 4, 2, 1, 4096, 64, W, S), _bytes(lib, "extend", 2, 4, 2, 1, 4096, 64, W, S),
                _bytes(lib, "ragged", 2, 4, 2, 40, 4096, 64, W, S))
        got = (n(device_ops.decode_workspace(q, big, window=W, sink=S)), n(device_ops.extend_workspace(q, big, window=W, sink=S)),
               n(device_ops.ragged_workspace(qr, big, cu, window=W, sink=S)))
        assert got == want, (W, S, got, want)
    for S in (None, 0):
        assert n(device_ops.decode_workspace(q, big, window=300, sink=S)) == _window_bytes(lib, "decode", 2, 4, 2, 1, 4096, 64, 300)
    assert n(device_ops.decode_workspace(q, big, window=300)) < n(device_ops.decode_workspace(q, big, window=300, sink=1000))
    with pytest.raises(ValueError, match="negative"):
        device_ops.decode_workspace(q, big, window=300, sink=-2)
    with pytest.raises(ValueError, match="needs window"):
        device_ops.extend_workspace(q, big, sink=2)


def test_model_sink_calls_under_the_recorder(monkeypatch):
    """The stack functions on a cache with sinks under the recorder of tests/test_device_ops_cpu.py (CPU tensors, no library): every
    attention call is the family's _sink entry point with the cache's window and sink, fused with the append; the workspaces are
    sized by the _sink queries; a cache with a window alone makes the _window calls it made before."""
    import torch
    from flash_attention_minitorch_amd import modules_transformer as mt
    from test_device_ops_cpu import install_recorder

    rec = install_recorder(monkeypatch)
    B, P, H, Hkv, d, cap, W, S = 2, 200, 4, 2, 64, 512, 160, 4
    g = torch.Generator().manual_seed(0)
    x = torch.randn((B, P, H * d), generator=g).to(torch.bfloat16)
    wq, wk = (torch.randn(s, generator=g).to(torch.bfloat16) for s in ((H * d, H * d), (H * d, Hkv * d)))
    layers = [(wq, wk, wk, wq)] * 2
    tail = lambda n, geo: f",{B},{H},{Hkv},{n},{geo},64,64,1,0.0,1,{W},{S},1,null)"

    cache = mt.KVCache(2, B, cap, H, d, torch.bfloat16, x.device, n_kv_head=Hkv, window=W, sink=S)
    rec.reset({})
    mt.attention_stack_prefill(x, layers, H, cache)
    calls = [c for c in rec.calls if "workspace_bytes" not in c]
    assert len(calls) == 2 and all(c.startswith("fa_mi355x_fwd_extend_sink(") and c.endswith(tail(P, f"{cap},0,0,0")) for c in calls), calls
    assert {c for c in rec.calls if "workspace_bytes" in c} == {f"fa_mi355x_extend_sink_workspace_bytes({B},{H},{Hkv},{P},{cap},64,{W},{S})"}
    rec.reset({})
    mt.attention_stack_step_fused(x[:, :1].contiguous(), layers, H, cache)
    mt.attention_stack_step(x[:, :3].contiguous(), layers, H, cache)
    calls = [c for c in rec.calls if "workspace_bytes" not in c]
    assert len(calls) == 4 and all(c.startswith("fa_mi355x_fwd_decode_sink(") for c in calls), calls
    assert all(c.endswith(tail(1, f"{cap},0,0,0")) for c in calls[:2]) and all(c.endswith(tail(3, f"{cap},0,0,0")) for c in calls[2:])
    assert {c.split("(")[0] for c in rec.calls if "workspace_bytes" in c} == {"fa_mi355x_decode_sink_workspace_bytes"}
    rec.reset({})
    mt.attention_stack_extend(x[:, :150].contiguous(), layers, H, cache)
    calls = [c for c in rec.calls if "workspace_bytes" not in c]
    assert len(calls) == 2 and all(c.startswith("fa_mi355x_fwd_extend_sink(") and c.endswith(tail(150, f"{cap},0,0,0")) for c in calls), calls
    rec.reset({})
    mt.attention_stack_ragged(x[0, :50].contiguous(), [7, 40], layers, H, cache)
    calls = [c for c in rec.calls if "workspace_bytes" not in c]
    assert len(calls) == 2 and all(c.startswith("fa_mi355x_fwd_ragged_sink(") and c.endswith(tail(50, f"{cap},0,0,0")) for c in calls), calls
    assert {c.split("(")[0] for c in rec.calls if "workspace_bytes" in c} == {"fa_mi355x_ragged_sink_workspace_bytes"}

    # a paged cache with sinks: the table and the pool's geometry; chunked prefill; the release keeps slot 0
    paged = mt.PagedKVCache(2, B, cap, H, d, torch.bfloat16, x.device, n_kv_head=Hkv, page_size=128, n_pages=8, window=W, sink=S)
    rec.reset({"table": paged.block_table})
    mt.attention_stack_prefill_chunked(x, layers, H, paged, 150)
    calls = [c for c in rec.calls if "workspace_bytes" not in c]
    assert [c.split("(")[0] for c in calls] == ["fa_mi355x_fwd_extend_sink"] * 2 + ["fa_mi355x_fwd_decode_sink"] * 2, calls
    assert all(",table," in c for c in calls) and calls[0].endswith(tail(150, "0,8,128,4")) and calls[2].endswith(tail(50, "0,8,128,4"))
    assert [len(p) for p in paged.pages] == [2, 2] and paged.release_behind_window([300, 287]) == 0
    paged.reserve(450)
    assert paged.release_behind_window([416, 414]) == 1 and paged.released == [1, 0]

    # the workspace cache keys hold the sinks: a cache that differs in sink alone never shares a buffer
    other = mt.KVCache(2, B, cap, H, d, torch.bfloat16, x.device, n_kv_head=Hkv, window=W, sink=S + 1)
    qq = torch.zeros(B, 1, H, d, dtype=torch.bfloat16)
    cache._workspaces.clear()
    cache.workspace(qq), cache.extend_workspace(qq)
    assert all(W in key and S in key for key in cache._workspaces) and len(cache._workspaces) == 2
    other.workspace(qq)
    assert not set(cache._workspaces) & set(other._workspaces)

    windowed = mt.KVCache(2, B, cap, H, d, torch.bfloat16, x.device, n_kv_head=Hkv, window=W)
    rec.reset({})
    mt.attention_stack_prefill(x, layers, H, windowed)
    mt.attention_stack_step_fused(x[:, :1].contiguous(), layers, H, windowed)
    names = [c.split("(")[0] for c in rec.calls]
    assert not [n for n in names if "sink" in n] and "fa_mi355x_fwd_decode_window" in names, names
