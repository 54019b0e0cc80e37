"""CPU-side checks of the logit soft-capping entry points (include/flash_attn_mi355x_decode_softcap.h: the decode, extend and ragged
calls in which every score becomes softcap * tanh(tau * q.k / softcap) before the masks): this file's fp64 references (used by
tests/test_gpu_softcap.py), which cap BEFORE masking over the mask of tests/test_window_cpu.py's reference; the three symbols
declared, exported and bound, and their parameter table in prototype order; the softcap builds present and free of scratch; every bad
cap and every other bad argument of the _window form answered before any HIP call (fake non-null pointers: a launch would fail with
another code); the window size queries answering for these calls; what device_ops sends under the recorder of
tests/test_device_ops_cpu.py, and what it refuses; the model layer's calls on a cache with a cap."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_abi_cpu import _device_kernels
from test_decode_cpu import built  # noqa: F401  (the module-scoped build fixture)
from test_ragged_cpu import seq_rows
from test_window_cpu import _BAD_FAMILY, _BAD_WINDOW, _bytes, _splits, _unwindowed, ragged_window_reference, window_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "flash_attn_mi355x_decode_softcap.h"
FAMILIES = ("decode", "extend", "ragged")
SOFTCAP = [f"fa_mi355x_fwd_{f}_softcap" for f in FAMILIES]


# ---- the references (used by tests/test_gpu_softcap.py) ----

def softcap_reference(q, k, v, lens, window, scale, softcap, causal=True):
    """fp64 attention with the cap applied to every score BEFORE the mask: q (BH, Nq, d), k / v (BH, Ncap, d), lens (BH,).  The mask
    is window_reference's (tests/test_window_cpu.py): query i sits at p = len - Nq + i and admits j <= p, and j > p - window when
    window > 0; ``causal`` False (window 0 only) admits every j < len.  softcap = 0: no cap.  Rows at or past a length are never
    touched (they may hold NaN).  Returns (out (BH, Nq, d), lse (BH, Nq)); rows with no admissible key: 0, -inf."""
    assert causal or window == 0
    BH, Nq, d = q.shape
    Ncap = k.shape[1]
    out = np.zeros((BH, Nq, v.shape[2]))
    lse = np.full((BH, Nq), -np.inf)
    for b in range(BH):
        n = int(min(max(int(lens[b]), 0), Ncap))
        if n == 0:
            continue
        pos = n - Nq + np.arange(Nq)
        j = np.arange(n)
        s = scale * (q[b].astype(np.float64) @ k[b, :n].astype(np.float64).T)   # (Nq, n)
        if softcap > 0:
            s = softcap * np.tanh(s / softcap)   # the cap first: a masked score stays -inf below
        ok = np.ones((Nq, n), bool)
        if causal:
            ok &= j[None, :] <= pos[:, None]
        if window > 0:
            ok &= j[None, :] > pos[:, None] - window
        s = np.where(ok, s, -np.inf)
        m = s.max(axis=1)
        fin = np.isfinite(m)
        e = np.exp(s - np.where(fin, m, 0)[:, None])
        e[~fin] = 0
        l = e.sum(axis=1)
        out[b][fin] = (e[fin] @ v[b, :n].astype(np.float64)) / l[fin, None]
        lse[b][fin] = m[fin] + np.log(l[fin])
    return out, lse


def ragged_softcap_reference(q, k, v, cu, lens, window, scale, softcap, causal=True):
    """ragged_window_reference of tests/test_window_cpu.py on softcap_reference: q (T, H, d) packed, k / v (B, Hkv, Ncap, d).  Returns
    (out (T, H, d), lse (H, T)), NaN in the rows no sequence owns."""
    T, H, d = q.shape
    B, Hkv, Ncap, _ = k.shape
    G = H // Hkv
    out, lse = np.full((T, H, v.shape[3]), np.nan), np.full((H, T), np.nan)
    for b in range(B):
        s, e = seq_rows(cu, T, b)
        if e == s:
            continue
        o, l = softcap_reference(q[s:e].transpose(1, 0, 2), np.repeat(k[b], G, axis=0), np.repeat(v[b], G, axis=0), np.full(H, lens[b]),
                                 window, scale, softcap, causal)
        out[s:e] = o.transpose(1, 0, 2)
        lse[:, s:e] = l
    return out, lse


def test_softcap_reference_caps_before_the_mask_and_is_the_window_reference_without_a_cap():
    rng = np.random.default_rng(3)
    BH, Ncap, d = 3, 300, 16
    k, v = (rng.uniform(-1, 1, (BH, Ncap, d)) for _ in range(2))
    lens = np.array([300, 140, 2])
    for Nq in (1, 3, 33):
        q = rng.uniform(-1, 1, (BH, Nq, d))
        for W in (0, 5, 100):
            want = window_reference(q, k, v, lens, W, 0.25)
            got = softcap_reference(q, k, v, lens, W, 0.25, 0.0)
            assert np.allclose(got[0], want[0], atol=1e-13) and np.array_equal(np.isneginf(got[1]), np.isneginf(want[1]))
            fin = np.isfinite(want[1])
            assert np.allclose(got[1][fin], want[1][fin], atol=1e-13)
            # a cap far above every score changes nothing to 1e-9; the cap of the GPU tests does
            big = softcap_reference(q, k, v, lens, W, 0.25, 1e4)
            assert np.allclose(big[0], want[0], atol=1e-9) and np.allclose(big[1][fin], want[1][fin], atol=1e-9)
    # one row by hand: 5 queries on a length of 12, W = 4, cap 0.3: query 2 sits at 9 and admits keys 6 .. 9
    q = rng.uniform(-1, 1, (1, 5, d))
    out, lse = softcap_reference(q, k[:1, :20], v[:1, :20], [12], 4, 0.5, 0.3)
    z = 0.3 * np.tanh(0.5 * k[0, 6:10] @ q[0, 2] / 0.3)
    p = np.exp(z - z.max())
    assert np.allclose(out[0, 2], p @ v[0, 6:10] / p.sum(), atol=1e-13) and np.isclose(lse[0, 2], z.max() + np.log(p.sum()))
    assert np.all(lse[0] <= 0.3 + np.log(4) + 1e-12)   # |z| <= softcap
    # the cap goes BEFORE the mask: rows at negative positions stay empty (a mask applied first would come back as -softcap)
    out, lse = softcap_reference(q, k[:1, :20], v[:1, :20], [3], 0, 0.5, 0.3)
    assert np.all(out[0, :2] == 0) and np.all(np.isneginf(lse[0, :2])) and np.all(np.isfinite(lse[0, 2:]))
    # non-causal: every key below the length, for every row
    out, lse = softcap_reference(q, k[:1, :20], v[:1, :20], [3], 0, 0.5, 0.3, causal=False)
    z = 0.3 * np.tanh(0.5 * q[0] @ k[0, :3].T / 0.3)
    assert np.allclose(lse[0], np.log(np.exp(z).sum(axis=1)), atol=1e-13)
    # the ragged reference is the uniform one on each sequence's rows
    q = rng.uniform(-1, 1, (9, 4, d))
    kr, vr = (rng.uniform(-1, 1, (3, 2, 30, d)) for _ in range(2))
    out, lse = ragged_softcap_reference(q, kr, vr, [0, 2, 2, 7], [20, 5, 30], 6, 0.5, 0.25)
    assert np.all(np.isnan(out[7:])) and np.all(np.isfinite(out[:7]))
    o, l = softcap_reference(q[2:7].transpose(1, 0, 2), np.repeat(kr[2], 2, axis=0), np.repeat(vr[2], 2, axis=0), np.full(4, 30), 6, 0.5, 0.25)
    assert np.array_equal(out[2:7], o.transpose(1, 0, 2)) and np.array_equal(lse[:, 2:7], l)
    want = ragged_window_reference(q, kr, vr, [0, 2, 2, 7], [20, 5, 30], 6, 0.5)
    got = ragged_softcap_reference(q, kr, vr, [0, 2, 2, 7], [20, 5, 30], 6, 0.5, 0.0)
    assert np.allclose(got[0][:7], want[0][:7], atol=1e-13)


# ---- the C ABI ----

def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)


def _param_names(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return {sym: [re.findall(r"\w+", p)[-1] for p in params.split(",")]
            for sym, params in re.findall(r"\b(fa_mi355x_\w+)\s*\(([^()]*)\)\s*;", text)}


def test_the_three_softcap_symbols_are_declared_exported_and_bound(built):
    from test_lib_cpu import _ctypes_kind, _prototypes
    main = open(os.path.join(ROOT, "include", "flash_attn_mi355x_decode.h")).read()
    assert f'#include "{HEADER}"' in main and main.rstrip().endswith("#endif /* FLASH_ATTN_MI355X_DECODE_H */")
    assert sorted(set(re.findall(r"\b(fa_mi355x_\w+)\s*\(", _header_text()))) == sorted(SOFTCAP) == sorted(built.SOFTCAP_ABI)
    protos, wprotos = _prototypes(HEADER), _prototypes("flash_attn_mi355x_decode_window.h")
    names, wnames = _param_names(HEADER), _param_names("flash_attn_mi355x_decode_window.h")
    lib = built.decode()
    for s in SOFTCAP:
        assert hasattr(lib, s), s
        res, args = built.SOFTCAP_ABI[s]
        ret, kinds = protos[s]
        assert [_ctypes_kind(a) for a in args] == kinds and _ctypes_kind(res) == ret, s
        assert getattr(lib, s).argtypes == args and getattr(lib, s).restype is res, s
        # the family's _window prototype with `float softcap` behind `int window`
        w = s.replace("_softcap", "_window")
        i = wnames[w].index("window") + 1
        assert names[s] == wnames[w][:i] + ["softcap"] + wnames[w][i:], s
        assert kinds == wprotos[w][1][:i] + ["float"] + wprotos[w][1][i:] and ret == wprotos[w][0], s
    assert re.sub(r"\s+", " ", _header_text()).count("int window, float softcap") == 3
    # no size query of its own: the header says which ones answer
    raw = open(os.path.join(ROOT, "include", HEADER)).read()
    assert "window_splits" in raw and "window_workspace_bytes" in raw and "no size queries of their own" in raw


def test_softcap_parameter_table_is_in_prototype_order(built):
    names = _param_names(HEADER)
    synonyms = {"T": "Nq"}
    assert sorted(built.KV_SOFTCAP_PARAMS) == sorted(SOFTCAP)
    for sym, params in built.KV_SOFTCAP_PARAMS.items():
        assert [synonyms.get(n, n) for n in names[sym]] == list(params), sym
        _, argtypes = built.SOFTCAP_ABI[sym]
        assert len(argtypes) == len(params), sym
        for n, t in zip(params, argtypes):
            want = ctypes.c_void_p if n in built.KV_POINTERS else ctypes.c_float if n in ("softmax_scale", "softcap") else ctypes.c_int
            assert t is want, (sym, n)
        assert built.KV_CALL_PARAMS[sym] == params
    assert all(built.KV_CALL_PARAMS[s] == p for s, p in built.KV_PARAMS.items()) and not set(built.KV_PARAMS) & set(SOFTCAP)


def test_the_softcap_builds_are_in_the_library_without_scratch(built):
    """(tests/test_window_cpu.py walks every kernel of the library; here: the new builds are among them.)"""
    kernels = _device_kernels(built.lib_path(built.DECODE_NAME))
    new = [k for k in kernels if "softcap_kernel" in k[0]]
    # T = float, bf16; D = 32, 64, 128; decode: PAGED x WINDOW; extend: PAGED x RAGGED x WINDOW
    assert len([k for k in new if "decode_split_softcap_kernel" in k[0]]) == 24
    assert len([k for k in new if "extend_split_softcap_kernel" in k[0]]) == 48
    for name, scratch, vgpr in new:
        assert scratch == 0 and vgpr <= 512, (name, scratch, vgpr)
    assert not [k for k in kernels if "combine" in k[0] and "softcap" in k[0]]   # (the combine kernel is not rebuilt)


# one valid call of each family (fake non-null device pointers: a launch would fail, so a code other than the expected one shows a
# HIP call)
_ONE = 16
_GOOD = dict(q=_ONE, kn=_ONE, vn=_ONE, k=_ONE, v=_ONE, out=_ONE, lse=_ONE, cu=_ONE, lens=_ONE, table=_ONE, ws=_ONE, B=2, H=4, Hkv=2, Nq=100,
             Ncap=2048, num_pages=40, page_size=128, max_pages=16, d_new=64, d=64, layout=1, scale=0.0, causal=1, window=300, softcap=30.0,
             dtype=1)
_VP = ctypes.c_void_p
BAD_ARG = 1
_SLAB, _ATTEND_ONLY = dict(table=0), dict(kn=0, vn=0)


def _call(lib, family, **over):
    a = dict(_GOOD, **over)
    ptrs = ("q", "kn", "vn", "k", "v", "out", "lse") + (("cu",) if family == "ragged" else ()) + ("lens", "table", "ws")
    args = [_VP(a[n]) for n in ptrs] + [a[n] for n in ("B", "H", "Hkv", "Nq", "Ncap", "num_pages", "page_size", "max_pages", "d_new", "d",
                                                       "layout", "scale", "causal", "window", "softcap", "dtype")] + [None]
    rc = getattr(lib, f"fa_mi355x_fwd_{family}_softcap")(*args)
    return rc, lib.fa_mi355x_decode_last_error().decode()


_BAD_CAP = [
    (dict(softcap=-1.0), BAD_ARG, "softcap"), (dict(softcap=-1e-30, **_SLAB, **_ATTEND_ONLY), BAD_ARG, "softcap"),
    (dict(softcap=float("nan")), BAD_ARG, "softcap"), (dict(softcap=float("nan"), window=0, causal=0, **_SLAB), BAD_ARG, "softcap"),
    (dict(softcap=float("inf")), BAD_ARG, "softcap"), (dict(softcap=float("-inf"), **_ATTEND_ONLY), BAD_ARG, "softcap"),
    # a bad cap is found with the window checks, in front of everything else: null pointers, bad pages, bad sizes
    (dict(softcap=-1.0, q=0, k=0), BAD_ARG, "softcap"), (dict(softcap=float("inf"), page_size=64, B=0), BAD_ARG, "softcap"),
    # a cap does not need the causal mask (the call goes on to the next check: the null q); a window still does
    (dict(causal=0, window=0, q=0), BAD_ARG, "null"), (dict(causal=0, window=0, softcap=0.0, q=0, **_SLAB), BAD_ARG, "null"),
]


def _cases():
    out = []
    for family in FAMILIES:
        out += [(family, o, c, m) for o, c, m in _BAD_CAP + _BAD_WINDOW + _BAD_FAMILY]
        out += [(family, dict(o, softcap=0.0), c, m) for o, c, m in _BAD_WINDOW]   # (softcap = 0: the _window call's checks)
    out += [("decode", dict(Nq=129), BAD_ARG, "Nq > 128"), ("ragged", dict(cu=0), BAD_ARG, "cu_seqlens_q"),
            ("ragged", dict(ws=0, window=1), BAD_ARG, "fa_mi355x_ragged_workspace_bytes"),
            ("extend", dict(H=1 << 12, Hkv=1, Nq=1 << 13, d=32, d_new=32), BAD_ARG, "2^25")]
    return out


def _id(case):
    return case[0] + "-" + ",".join(f"{k}={v}" for k, v in case[1].items())


@pytest.mark.parametrize("family,over,code,msg", _cases(), ids=[_id(c) for c in _cases()])
def test_softcap_forms_reject_each_bad_argument_before_any_hip_call(built, family, over, code, msg):
    rc, err = _call(built.decode(), family, **over)
    assert rc == code and err and msg in err, (rc, err)


# the shapes of tests/test_gpu_softcap.py whose path depends on the policy: (family, B, H, Hkv, Nq or T, Ncap, d, W) -> splits.  The
# cap is no argument of the policy: the window queries answer, window = 0 for a call without one.
GPU_SPLITS = [
    (("decode", 7, 4, 2, 1, 384, 64, 0), 2), (("decode", 7, 4, 2, 33, 384, 64, 0), 2), (("decode", 7, 4, 2, 3, 384, 64, 100), 1),
    (("extend", 7, 4, 2, 129, 384, 64, 0), 2), (("extend", 7, 4, 2, 130, 384, 64, 100), 2),
    (("ragged", 6, 4, 2, 172, 384, 64, 0), 2), (("ragged", 6, 4, 2, 172, 384, 64, 100), 2),
    (("ragged", 6, 4, 2, 169, 256, 64, 0), 1), (("ragged", 6, 4, 2, 169, 256, 64, 100), 1),   # the bitwise comparison with extend
    (("decode", 2, 4, 2, 1, 1024, 32, 0), 4),   # the graphed steps of the model test
]


def test_window_size_queries_answer_for_the_capped_calls(built):
    lib = built.decode()
    for (family, B, H, Hkv, Nq, Ncap, d, W), ns in GPU_SPLITS:
        for dt in (0, 1):
            assert _splits(lib, family, B, H, Hkv, Nq, Ncap, d, W, dt) == ns, (family, B, H, Hkv, Nq, Ncap, d, W)
    assert all(_splits(lib, "extend", 1, 4, 2, nq, 256, 64, W) == 1 for nq in (1, 33, 129, 5) for W in (0, 100))
    # window = 0 gives the unwindowed figures, splits and bytes
    for family, B, H, Hkv, Nq, Ncap, d in (("decode", 32, 32, 8, 1, 4096, 128), ("extend", 32, 32, 8, 512, 8704, 128),
                                           ("ragged", 8, 8, 2, 633, 520, 64), ("decode", 7, 4, 2, 33, 384, 32)):
        full = _unwindowed(lib, family, B, H, Hkv, Nq, Ncap, d)
        assert (_splits(lib, family, B, H, Hkv, Nq, Ncap, d, 0), _bytes(lib, family, B, H, Hkv, Nq, Ncap, d, 0)) == full
    assert not [s for s in dir(lib) if "softcap_splits" in s or "softcap_workspace" in s]
    for f in FAMILIES:   # (no size query of their own is exported)
        assert not hasattr(lib, f"fa_mi355x_{f}_softcap_splits") and not hasattr(lib, f"fa_mi355x_{f}_softcap_workspace_bytes")


# ---- the Python layer, under the recorder ----

def _attend_calls(rec):
    return [c for c in rec.calls if "workspace_bytes" not in c and "rope" not in c]


def _args(call):
    sym, rest = call.split("(", 1)
    return sym, rest[:-1].split(",")


@pytest.mark.parametrize("family", FAMILIES)
def test_a_capped_call_sends_the_softcap_symbol_with_the_cap_in_place(monkeypatch, family):
    from flash_attention_minitorch_amd import _lib
    from test_kv_ops_cpu import W, call, install, make
    rec = install(monkeypatch, False)
    sym = f"fa_mi355x_fwd_{family}_softcap"
    params = _lib.KV_SOFTCAP_PARAMS[sym]
    for paged in (False, True):
        for fused in (False, True):
            for window in (None, 0, W):
                for cap in (0.25, 50, np.float32(30.0)):
                    a = make(family, "attend", paged=paged, fused=fused, softcap=cap, **({} if window is None else dict(window=window)))
                    rec.reset(a)
                    call(family, "attend", a)
                    calls = _attend_calls(rec)
                    assert len(calls) == 1, calls
                    got, args = _args(calls[0])
                    assert got == sym and len(args) == len(params), calls
                    f = dict(zip(params, args))
                    assert f["softcap"] == repr(float(cap)) and f["window"] == str(window or 0), (f, window)
                    assert (f["k_new"], f["v_new"]) == (("k_new", "v_new") if fused else ("null", "null"))
                    assert f["block_table"] == ("block_table" if paged else "null")
                    assert (f["q"], f["k_cache"], f["v_cache"], f["causal"]) == ("q", "k_cache", "v_cache", "1")
                    # the workspace is sized by the queries that were there: none of them is a softcap symbol
                    sizes = {c.split("(")[0] for c in rec.calls if "workspace_bytes" in c}
                    assert sizes and not [s for s in sizes if "softcap" in s], sizes
    # a cap without the causal mask is a call; with rotary tables the roped append runs in front of the attend-only capped call
    a = make(family, "attend", softcap=0.25, causal=False)
    rec.reset(a)
    call(family, "attend", a)
    got, args = _args(_attend_calls(rec)[0])
    assert got == sym and dict(zip(params, args))["causal"] == "0"
    a = make(family, "attend", fused=True, rope=True, softcap=0.25)
    rec.reset(a)
    call(family, "attend", a)
    names = [c.split("(")[0] for c in rec.calls if "workspace_bytes" not in c]
    assert names == ["fa_mi355x_rope_append_ragged" if family == "ragged" else "fa_mi355x_rope_append", sym], names
    f = dict(zip(params, _args(rec.calls[-1])[1]))
    assert (f["k_new"], f["v_new"], f["softcap"]) == ("null", "null", "0.25")


@pytest.mark.parametrize("family", FAMILIES)
def test_no_cap_and_a_cap_of_zero_send_exactly_what_they_send_today(monkeypatch, family):
    from test_kv_ops_cpu import S, W, call, install, make
    rec = install(monkeypatch, False)
    for opts in ({}, dict(paged=True, fused=True), dict(window=W), dict(window=W, sink=S, paged=True), dict(fused=True, rope=True),
                 dict(causal=False)):
        a = make(family, "attend", **opts)
        rec.reset(a)
        call(family, "attend", a)
        today = list(rec.calls)
        assert today and not [c for c in today if "softcap" in c]
        for cap in (None, 0, 0.0):
            rec.reset(a)
            call(family, "attend", dict(a, softcap=cap))
            assert rec.calls == today, (opts, cap)


@pytest.mark.parametrize("family", FAMILIES)
def test_softcap_python_refusals_come_before_any_library_call(monkeypatch, family):
    from test_kv_ops_cpu import S, W, call, install, make
    rec = install(monkeypatch, False)
    a = make(family, "attend")
    rec.reset(a)
    for bad in (True, False, "50", -1, -0.5, float("nan"), float("inf"), float("-inf"), [50.0], 1j):
        with pytest.raises(ValueError, match="softcap"):
            call(family, "attend", dict(a, softcap=bad))
    with pytest.raises(ValueError, match="(?s)softcap.*sink"):
        call(family, "attend", dict(a, softcap=30.0, window=W, sink=S))
    assert rec.calls == []
    if family != "ragged":   # (the ragged calls have no fp8 form at all)
        a = make(family, "attend", fp8=True)
        rec.reset(a)
        with pytest.raises(ValueError, match="(?s)softcap.*fp8"):
            call(family, "attend", dict(a, softcap=30.0))
        assert rec.calls == []
    # a sink of 0 is no sink: the capped windowed call
    a = make(family, "attend", softcap=30.0, window=W, sink=0)
    rec.reset(a)
    call(family, "attend", a)
    assert _attend_calls(rec)[0].startswith(f"fa_mi355x_fwd_{family}_softcap(")


# ---- the model layer ----

def test_model_softcap_calls_under_the_recorder(monkeypatch):
    """The stack functions on a cache with a cap (CPU tensors, no library): every attention call is the family's _softcap entry point
    with the cache's cap, fused with the append; a prompt goes through the extend call (the square forward has no cap); a cache
    without a cap sends no new keyword and makes the calls it made before."""
    import torch
    from flash_attention_minitorch_amd import modules_transformer as mt
    from test_device_ops_cpu import install_recorder

    rec = install_recorder(monkeypatch)
    B, P, H, Hkv, d, cap, W, C = 2, 200, 4, 2, 64, 512, 160, 30.0
    g = torch.Generator().manual_seed(0)
    x = torch.randn((B, P, H * d), generator=g).to(torch.bfloat16)
    wq, wk = (torch.randn(s, generator=g).to(torch.bfloat16) for s in ((H * d, H * d), (H * d, Hkv * d)))
    layers = [(wq, wk, wk, wq)] * 2
    tail = lambda n, geo, w: f",{B},{H},{Hkv},{n},{geo},64,64,1,0.0,1,{w},{C!r},1,null)"
    attends = lambda: [c for c in rec.calls if "workspace_bytes" not in c]

    cache = mt.KVCache(2, B, cap, H, d, torch.bfloat16, x.device, n_kv_head=Hkv, softcap=C)
    assert cache.capping() == dict(softcap=C) and cache.keywords(0) == dict(softcap=C) and cache.windowing() == {}
    rec.reset({})
    mt.attention_stack_prefill(x, layers, H, cache)
    calls = attends()
    assert len(calls) == 2 and all(c.startswith("fa_mi355x_fwd_extend_softcap(") and c.endswith(tail(P, f"{cap},0,0,0", 0)) for c in calls), calls
    assert {c.split("(")[0] for c in rec.calls if "workspace_bytes" in c} == {"fa_mi355x_extend_workspace_bytes"}
    assert cache.length_bound == P
    rec.reset({})
    mt.attention_stack_step_fused(x[:, :1].contiguous(), layers, H, cache)
    mt.attention_stack_step(x[:, :3].contiguous(), layers, H, cache)
    calls = attends()
    assert len(calls) == 4 and all(c.startswith("fa_mi355x_fwd_decode_softcap(") for c in calls), calls
    assert all(c.endswith(tail(1, f"{cap},0,0,0", 0)) for c in calls[:2]) and all(c.endswith(tail(3, f"{cap},0,0,0", 0)) for c in calls[2:])
    assert all(_args(c)[1][1:3] == ["null", "null"] for c in calls[2:])   # (the caller-side append: attend only)
    assert all(_args(c)[1][1:3] != ["null", "null"] for c in calls[:2])
    rec.reset({})
    mt.attention_stack_ragged(x[0, :50].contiguous(), [7, 40], layers, H, cache)
    calls = attends()
    assert len(calls) == 2 and all(c.startswith("fa_mi355x_fwd_ragged_softcap(") and c.endswith(tail(50, f"{cap},0,0,0", 0)) for c in calls), calls
    rec.reset({})
    mt.attention_stack_extend(x[:, :150].contiguous(), layers, H, cache)
    assert [c.split("(")[0] for c in attends()] == ["fa_mi355x_fwd_extend_softcap"] * 2

    # a paged windowed cache with a cap: the table, the pool's geometry, the window and the cap in one call
    paged = mt.PagedKVCache(2, B, cap, H, d, torch.bfloat16, x.device, n_kv_head=Hkv, page_size=128, n_pages=7, window=W, softcap=C)
    assert paged.keywords(1, k_new=1) == dict(k_new=1, block_table=paged.block_table, window=W, softcap=C)
    rec.reset({"table": paged.block_table})
    mt.attention_stack_prefill_chunked(x, layers, H, paged, 150)
    calls = attends()
    assert [c.split("(")[0] for c in calls] == ["fa_mi355x_fwd_extend_softcap"] * 2 + ["fa_mi355x_fwd_decode_softcap"] * 2, calls
    assert all(",table," in c for c in calls) and calls[0].endswith(tail(150, "0,7,128,4", W)) and calls[2].endswith(tail(50, "0,7,128,4", W))
    assert {c.split("(")[0] for c in rec.calls if "workspace_bytes" in c} == {"fa_mi355x_extend_window_workspace_bytes",
                                                                              "fa_mi355x_decode_window_workspace_bytes"}
    # a roped cache with a cap: the roped append, then the attend-only capped call
    roped = mt.KVCache(2, B, cap, H, d, torch.bfloat16, x.device, n_kv_head=Hkv, rope=mt.Rotary.table(cap, 32), softcap=C)
    rec.reset({})
    mt.attention_stack_step_fused(x[:, :1].contiguous(), layers, H, roped)
    assert [c.split("(")[0] for c in attends()] == ["fa_mi355x_rope_append", "fa_mi355x_fwd_decode_softcap"] * 2

    # a cache without a cap sends no new keyword, and the calls it made before
    plain = mt.KVCache(2, B, cap, H, d, torch.bfloat16, x.device, n_kv_head=Hkv)
    assert plain.capping() == {} and plain.keywords(0) == {} and plain.softcap is None
    rec.reset({})
    mt.attention_stack_prefill(x, layers, H, plain)
    mt.attention_stack_step_fused(x[:, :1].contiguous(), layers, H, plain)
    names = [c.split("(")[0] for c in rec.calls]
    assert not [n for n in names if "softcap" in n or "window" in n] and "fa_mi355x_fwd_decode_append" in names, names


def test_cache_constructor_checks_the_cap_last():
    import torch
    from flash_attention_minitorch_amd import modules_transformer as mt
    mk = lambda cls=mt.KVCache, **kw: cls(1, 1, 256, 2, 32, torch.bfloat16, "cpu", **kw)
    for bad in (0, 0.0, -1.0, True, "30", float("nan"), float("inf")):
        with pytest.raises(ValueError, match="softcap"):
            mk(softcap=bad)
    assert mk(softcap=30).softcap == 30.0 and mk(softcap=np.float32(0.25)).softcap == 0.25 and mk(mt.PagedKVCache, softcap=50.0).softcap == 50.0
    with pytest.raises(ValueError, match="(?s)softcap.*sink"):
        mk(window=64, sink=4, softcap=30.0)
    assert mk(window=64, sink=0, softcap=30.0).keywords(0) == dict(window=64, softcap=30.0)
    with pytest.raises(ValueError, match="(?s)softcap.*fp8"):
        mk(kv_dtype=torch.float8_e4m3fn, softcap=30.0)
    # the documented order of first faults stays: window, sink, n_kv_head, the layout's own, rope, kv_dtype / kv_scale, then the cap
    with pytest.raises(ValueError, match="window must be"):
        mk(window=0, softcap=-1.0)
    with pytest.raises(ValueError, match="n_kv_head"):
        mk(n_kv_head=3, softcap=-1.0)
    with pytest.raises(ValueError, match="page_size"):
        mk(mt.PagedKVCache, page_size=100, softcap=-1.0)
    with pytest.raises(ValueError, match="kv_scale belongs"):
        mk(kv_scale=(1, 2), softcap=-1.0)
    with pytest.raises(ValueError, match="kv_dtype must be"):
        mk(kv_dtype=torch.float16, softcap=-1.0)
