"""CPU-side checks of the learned sink logits of the KV-cache calls (include/flash_attn_mi355x_decode_lsink.h: the decode, extend and
ragged calls in which one learned fp32 logit per query head joins every softmax as an extra column without a value vector): this
file's fp64 references (used by tests/test_gpu_lsink.py), written as a softmax over the admitted scores plus one column, against the
sigmoid / softplus identity and a row worked by hand; the three symbols declared, exported and bound, and their parameter table in
prototype order; the lsink builds present and free of scratch; every bad argument of the _window form answered before any HIP call
(fake non-null pointers: a launch would fail with another code); what device_ops sends under the recorder of
tests/test_device_ops_cpu.py, and what it refuses; the model layer's calls on a cache with logits; and the case list of the GPU tests
with, for every case, the proof that the reference with the logits is many tolerances away from the one without."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import oracle
from gpu_util import maxabs, rand_u
from test_abi_cpu import _device_kernels
from test_decode_cpu import built  # noqa: F401  (the module-scoped build fixture)
from test_ragged_cpu import seq_rows
from test_window_cpu import _BAD_FAMILY, _BAD_WINDOW, _splits, ragged_window_reference, window_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "flash_attn_mi355x_decode_lsink.h"
FAMILIES = ("decode", "extend", "ragged")
LSINK = [f"fa_mi355x_fwd_{f}_lsink" for f in FAMILIES]
TOL = {"f32": 1e-4, "bf16": 1e-3}   # the project's own (tests/test_gpu_decode.py): the sink column only shrinks P


# ---- the references (used by tests/test_gpu_lsink.py) ----

def lsink_reference(q, k, v, lens, window, scale, logits, causal=True):
    """fp64 attention with one extra softmax column: q (BH, Nq, d), k / v (BH, Ncap, d), lens (BH,), logits (BH,) -- the logit of
    each row of BH -- or None (no column: the call without the logits).  The mask is window_reference's (tests/test_window_cpu.py):
    query i sits at p = len - Nq + i and admits j <= p, and j > p - window when window > 0; ``causal`` False (window 0 only) admits
    every j < len.  The column's logit is not scaled and not masked.  Rows at or past a length are never touched (they may hold NaN).
    Returns (out (BH, Nq, d), lse (BH, Nq)); a row with no admissible key: out = 0 and lse = its logit (-inf without logits)."""
    assert causal or window == 0
    BH, Nq, d = q.shape
    Ncap = k.shape[1]
    out = np.zeros((BH, Nq, v.shape[2]))
    lse = np.full((BH, Nq), -np.inf)
    for b in range(BH):
        n = int(min(max(int(lens[b]), 0), Ncap))
        pos = n - Nq + np.arange(Nq)
        j = np.arange(n)
        s = scale * (q[b].astype(np.float64) @ k[b, :n].astype(np.float64).T)   # (Nq, n)
        ok = np.ones((Nq, n), bool)
        if causal:
            ok &= j[None, :] <= pos[:, None]
        if window > 0:
            ok &= j[None, :] > pos[:, None] - window
        s = np.where(ok, s, -np.inf)
        if logits is not None:   # the extra column: every row admits it
            s = np.concatenate([s, np.full((Nq, 1), float(logits[b]))], axis=1)
        if s.shape[1] == 0:
            continue
        m = s.max(axis=1)
        fin = np.isfinite(m)
        e = np.exp(s - np.where(fin, m, 0)[:, None])
        e[~fin] = 0
        l = e.sum(axis=1)
        p = e[fin] / l[fin, None]
        out[b][fin] = p[:, :n] @ v[b, :n].astype(np.float64)   # (the column has no value vector)
        lse[b][fin] = m[fin] + np.log(l[fin])
    return out, lse


def ragged_lsink_reference(q, k, v, cu, lens, window, scale, logits, causal=True):
    """ragged_window_reference of tests/test_window_cpu.py on lsink_reference: q (T, H, d) packed, k / v (B, Hkv, Ncap, d), logits
    (H,) or None.  Returns (out (T, H, d), lse (H, T)), NaN in the rows no sequence owns."""
    T, H, d = q.shape
    B, Hkv, Ncap, _ = k.shape
    G = H // Hkv
    out, lse = np.full((T, H, v.shape[3]), np.nan), np.full((H, T), np.nan)
    for b in range(B):
        s, e = seq_rows(cu, T, b)
        if e == s:
            continue
        o, l = lsink_reference(q[s:e].transpose(1, 0, 2), np.repeat(k[b], G, axis=0), np.repeat(v[b], G, axis=0), np.full(H, lens[b]),
                               window, scale, logits, causal)
        out[s:e] = o.transpose(1, 0, 2)
        lse[:, s:e] = l
    return out, lse


def test_lsink_reference_is_the_identity_on_the_plain_call_and_a_row_by_hand():
    rng = np.random.default_rng(5)
    BH, Ncap, d = 3, 300, 16
    k, v = (rng.uniform(-1, 1, (BH, Ncap, d)) for _ in range(2))
    lens = np.array([300, 140, 2])
    a = np.array([-1.0, 0.5, 3.0])
    for Nq in (1, 3, 33):
        q = rng.uniform(-1, 1, (BH, Nq, d))
        for W, causal in ((0, True), (5, True), (100, True), (0, False)):
            # without logits: the window reference (causal) itself
            o0, l0 = lsink_reference(q, k, v, lens, W, 0.25, None, causal)
            if causal:
                want = window_reference(q, k, v, lens, W, 0.25)
                assert np.allclose(o0, want[0], atol=1e-13) and np.array_equal(np.isneginf(l0), np.isneginf(want[1]))
                assert np.allclose(l0[np.isfinite(l0)], want[1][np.isfinite(l0)], atol=1e-13)
            # with: out = out0 * sigmoid(lse0 - a), lse = lse0 + softplus(a - lse0); an empty row: out = 0, lse = a
            o, l = lsink_reference(q, k, v, lens, W, 0.25, a, causal)
            assert np.all(np.isfinite(l))
            x = l0 - a[:, None]
            fin = np.isfinite(l0)
            sig = np.where(fin, 1.0 / (1.0 + np.exp(-np.where(fin, x, 0.0))), 0.0)
            assert np.allclose(o, o0 * sig[..., None], atol=1e-13)
            assert np.allclose(l[fin], l0[fin] + np.logaddexp(0.0, -x[fin]), atol=1e-12)
            assert np.array_equal(l[~fin], np.broadcast_to(a[:, None], l.shape)[~fin]) and not o[~fin].any()
            assert np.all(l > l0)   # (the column only adds mass: every row of P sums to less than 1)
    # one row by hand: 5 queries on a length of 12, W = 4, a = 0.7: query 2 sits at 9 and admits keys 6 .. 9 and the column
    q = rng.uniform(-1, 1, (1, 5, d))
    out, lse = lsink_reference(q, k[:1, :20], v[:1, :20], [12], 4, 0.5, [0.7])
    z = np.append(0.5 * k[0, 6:10] @ q[0, 2], 0.7)
    p = np.exp(z - z.max())
    p /= p.sum()
    assert np.allclose(out[0, 2], p[:4] @ v[0, 6:10], atol=1e-13) and np.isclose(lse[0, 2], np.log(np.exp(z).sum()))
    assert p[:4].sum() < 1.0
    # the logit is in logit units: the scale does not touch it (halving the scale with doubled q leaves everything)
    o2, l2 = lsink_reference(2 * q, k[:1, :20], v[:1, :20], [12], 4, 0.25, [0.7])
    assert np.allclose(o2, out, atol=1e-13) and np.allclose(l2, lse, atol=1e-13)
    # a sequence of length 0, and rows at negative positions: out = 0 and lse = a exactly
    out, lse = lsink_reference(q, k[:1, :20], v[:1, :20], [0], 0, 0.5, [0.7])
    assert not out.any() and np.all(lse == 0.7)
    out, lse = lsink_reference(q, k[:1, :20], v[:1, :20], [3], 0, 0.5, [0.7])
    assert not out[0, :2].any() and np.all(lse[0, :2] == 0.7) and np.all(lse[0, 2:] > 0.7)
    # the ragged reference is the uniform one on each sequence's rows, a head's logit with its head
    q = rng.uniform(-1, 1, (9, 4, d))
    kr, vr = (rng.uniform(-1, 1, (3, 2, 30, d)) for _ in range(2))
    ah = np.array([-1.0, 0.0, 1.0, 3.0])
    out, lse = ragged_lsink_reference(q, kr, vr, [0, 2, 2, 7], [20, 5, 30], 6, 0.5, ah)
    assert np.all(np.isnan(out[7:])) and np.all(np.isfinite(out[:7]))
    o, l = lsink_reference(q[2:7].transpose(1, 0, 2), np.repeat(kr[2], 2, axis=0), np.repeat(vr[2], 2, axis=0), np.full(4, 30), 6, 0.5, ah)
    assert np.array_equal(out[2:7], o.transpose(1, 0, 2)) and np.array_equal(lse[:, 2:7], l)
    want = ragged_window_reference(q, kr, vr, [0, 2, 2, 7], [20, 5, 30], 6, 0.5)
    got = ragged_lsink_reference(q, kr, vr, [0, 2, 2, 7], [20, 5, 30], 6, 0.5, None)
    assert np.allclose(got[0][:7], want[0][:7], atol=1e-13)


# ---- the cases of tests/test_gpu_lsink.py: inputs made here, so that the CPU side can show what the GPU side relies on ----

HKV = 2
GROUPS = (1, 4)                     # H = G * HKV query heads: the ungrouped call (the grouped build at G = 1) and a group of four
WINDOWS = (0, 64)                   # none, and one that ends inside the first super tile of a length above 64
NCAP = 384                          # three 128-key super tiles
LENS = [1, 127, 128, 129, 300, 0]   # one key, around a tile edge, several tiles with a partial last one; a sequence of length 0
LONG_NCAP, LONG_LENS = 2048, [2000, 3]   # the longer length: many splits, beside a row of three keys in the same call
COUNTS = [0, 1, 37, 130]            # ragged: no token, one, part of a block, more than a block (G * 130 rows)
RLENS = [300, 1, 127, 300]          # ... against these lengths: one token into an empty cache; as many keys as tokens and more
TAIL = 3                            # unused rows behind the last sequence
# (family, Nq or None, lengths, Ncap)
KV_CASES = [("decode", 1, LENS, NCAP), ("decode", 5, LENS, NCAP), ("decode", 1, LONG_LENS, LONG_NCAP), ("decode", 5, LONG_LENS, LONG_NCAP),
            ("extend", 130, LENS, NCAP), ("ragged", None, RLENS, NCAP)]


def _round(x, dtype):
    return oracle.bf16_round(x) if dtype == "bf16" else x


def kv_case(family, dtype, d, G, W, Nq, lens, Ncap):
    """The inputs of one GPU case, a function of its parameters alone: q (B, H, Nq, d) -- ragged: packed (T, H, d) and cu -- and k, v
    (B, Hkv, Ncap, d) in U(-1, 1), rounded to the dtype, NaN at and past every length; logits (H,) fp32 in U(-1, 3)."""
    H = G * HKV
    seed = [FAMILIES.index(family), dtype == "bf16", d, G, W, Nq or 0, Ncap]
    rng = np.random.default_rng(seed)
    B = len(lens)
    k, v = (_round(rand_u(rng, (B, HKV, Ncap, d)), dtype) for _ in range(2))
    for b, n in enumerate(lens):
        k[b, :, n:] = np.nan
        v[b, :, n:] = np.nan
    logits = rng.uniform(-1.0, 3.0, H).astype(np.float32)
    if family == "ragged":
        cu = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.int32)
        return dict(q=_round(rand_u(rng, (sum(COUNTS) + TAIL, H, d)), dtype), k=k, v=v, cu=cu, logits=logits, H=H)
    return dict(q=_round(rand_u(rng, (B, H, Nq, d)), dtype), k=k, v=v, logits=logits, H=H)


def kv_reference(family, c, lens, W, with_logits=True):
    """The fp64 reference of a kv_case, with or without its logits: uniform (out (B, H, Nq, d), lse (B, H, Nq)), or the ragged pair."""
    d = c["q"].shape[-1]
    a = c["logits"].astype(np.float64) if with_logits else None
    if family == "ragged":
        return ragged_lsink_reference(c["q"], c["k"], c["v"], c["cu"], lens, W, 1.0 / math.sqrt(d), a)
    B, H, Nq, _ = c["q"].shape
    G = H // HKV
    ks, vs = (np.repeat(t, G, axis=1).reshape(B * H, *t.shape[2:]) for t in (c["k"], c["v"]))
    o, l = lsink_reference(c["q"].reshape(B * H, Nq, d), ks, vs, np.repeat(lens, H), W, 1.0 / math.sqrt(d), None if a is None else np.tile(a, B))
    return o.reshape(B, H, Nq, -1), l.reshape(B, H, Nq)


def discriminates(with_, without, dtype):
    """The condition on the REFERENCES of a case: with and without the logits they differ by at least 10 tolerances, in out and in
    lse (the largest difference over the case's rows), so the tolerance tells a kernel that reads the logits from one that does not."""
    own = ~np.isnan(with_[1])
    lw, lo = with_[1][own], np.where(np.isfinite(without[1][own]), without[1][own], -1e30)
    rows = ~np.isnan(with_[0][..., 0])
    return maxabs(with_[0][rows], without[0][rows]) >= 10 * TOL[dtype] and float(np.max(lw - lo)) >= 10 * TOL[dtype]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_every_gpu_case_tells_the_logits_from_their_absence(built, d, dtype):
    """Every case of tests/test_gpu_lsink.py's parity tests: the two references are at least 10 tolerances apart in out and in lse,
    so the GPU tests cannot pass on code that ignores the argument.  And the case list holds both epilogues: calls of one split (the
    split kernel's own store) and of several (the combine kernel), by the library's own size query."""
    lib = built.decode()
    seen = set()
    for family, Nq, lens, Ncap in KV_CASES:
        for G in GROUPS:
            for W in WINDOWS:
                c = kv_case(family, dtype, d, G, W, Nq, lens, Ncap)
                assert c["logits"].min() >= -1 and c["logits"].max() <= 3
                assert discriminates(kv_reference(family, c, lens, W), kv_reference(family, c, lens, W, False), dtype), (family, Nq, G, W)
                n = c["q"].shape[0] if family == "ragged" else Nq
                ns = _splits(lib, family, len(lens), G * HKV, HKV, n, Ncap, d, W, 0 if dtype == "f32" else 1)
                if family == "decode":
                    seen.add(ns > 1)
    assert seen == {True, False}


# ---- the C ABI ----

def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)


def _param_names(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return {sym: [re.findall(r"\w+", p)[-1] for p in params.split(",")]
            for sym, params in re.findall(r"\b(fa_mi355x_\w+)\s*\(([^()]*)\)\s*;", text)}


def test_the_three_lsink_symbols_are_declared_exported_and_bound(built):
    from test_lib_cpu import _ctypes_kind, _prototypes
    main = open(os.path.join(ROOT, "include", "flash_attn_mi355x_decode.h")).read()
    assert f'#include "{HEADER}"' in main and main.rstrip().endswith("#endif /* FLASH_ATTN_MI355X_DECODE_H */")
    assert sorted(set(re.findall(r"\b(fa_mi355x_\w+)\s*\(", _header_text()))) == sorted(LSINK) == sorted(built.LSINK_ABI)
    protos, wprotos = _prototypes(HEADER), _prototypes("flash_attn_mi355x_decode_window.h")
    names, wnames = _param_names(HEADER), _param_names("flash_attn_mi355x_decode_window.h")
    lib = built.decode()
    for s in LSINK:
        assert hasattr(lib, s), s
        res, args = built.LSINK_ABI[s]
        ret, kinds = protos[s]
        assert [_ctypes_kind(a) for a in args] == kinds and _ctypes_kind(res) == ret, s
        assert getattr(lib, s).argtypes == args and getattr(lib, s).restype is res, s
        # the family's _window prototype with `const float* sink_logits` behind `int window`
        w = s.replace("_lsink", "_window")
        i = wnames[w].index("window") + 1
        assert names[s] == wnames[w][:i] + ["sink_logits"] + wnames[w][i:], s
        assert kinds == wprotos[w][1][:i] + ["pointer"] + wprotos[w][1][i:] and ret == wprotos[w][0], s
    assert re.sub(r"\s+", " ", _header_text()).count("int window, const float* sink_logits") == 3
    # no size query of its own: the header says which ones answer
    raw = open(os.path.join(ROOT, "include", HEADER)).read()
    assert "window_splits" in raw and "window_workspace_bytes" in raw and "no size queries of their own" in raw
    assert not [s for s in dir(lib) if "lsink_splits" in s or "lsink_workspace" in s]


def test_lsink_parameter_table_is_in_prototype_order(built):
    names = _param_names(HEADER)
    synonyms = {"T": "Nq"}
    assert sorted(built.KV_LSINK_PARAMS) == sorted(LSINK)
    for sym, params in built.KV_LSINK_PARAMS.items():
        assert [synonyms.get(n, n) for n in names[sym]] == list(params), sym
        _, argtypes = built.LSINK_ABI[sym]
        assert len(argtypes) == len(params), sym
        for n, t in zip(params, argtypes):
            want = ctypes.c_void_p if n in built.KV_POINTERS else ctypes.c_float if n == "softmax_scale" else ctypes.c_int
            assert t is want, (sym, n)
        assert built.KV_CALL_PARAMS[sym] == params
    assert "sink_logits" in built.KV_POINTERS
    assert all(built.KV_CALL_PARAMS[s] == p for s, p in built.KV_PARAMS.items()) and not set(built.KV_PARAMS) & set(LSINK)
    assert all(built.KV_CALL_PARAMS[s] == p for s, p in built.KV_SOFTCAP_PARAMS.items())


def test_the_lsink_builds_are_in_the_library_without_scratch(built):
    """(tests/test_window_cpu.py walks every kernel of the library; here: the new builds are among them.)"""
    kernels = _device_kernels(built.lib_path(built.DECODE_NAME))
    new = [k for k in kernels if "lsink_kernel" in k[0]]
    # T = float, bf16; D = 32, 64, 128; decode: PAGED x WINDOW; extend: PAGED x RAGGED x WINDOW; combine: D x RAGGED
    assert len([k for k in new if "decode_split_lsink_kernel" in k[0]]) == 24
    assert len([k for k in new if "extend_split_lsink_kernel" in k[0]]) == 48
    assert len([k for k in new if "decode_combine_lsink_kernel" in k[0]]) == 6
    assert len(new) == 78
    for name, scratch, vgpr in new:
        assert scratch == 0 and vgpr <= 512, (name, scratch, vgpr)
    # the combine kernel keeps its nine builds under the names they had
    assert len([k for k in kernels if re.search(r"decode_combine_kernelILi(32|64|128)ELb[01]ELb[01]EEEv", k[0])]) == 9


# one valid call of each family (fake non-null device pointers: a launch would fail, so a code other than the expected one shows a
# HIP call)
_ONE = 16
_GOOD = dict(q=_ONE, kn=_ONE, vn=_ONE, k=_ONE, v=_ONE, out=_ONE, lse=_ONE, cu=_ONE, lens=_ONE, table=_ONE, ws=_ONE, B=2, H=4, Hkv=2, Nq=100,
             Ncap=2048, num_pages=40, page_size=128, max_pages=16, d_new=64, d=64, layout=1, scale=0.0, causal=1, window=300, logits=_ONE,
             dtype=1)
_VP = ctypes.c_void_p
BAD_ARG = 1
_SLAB = dict(table=0)


def _call(lib, family, **over):
    a = dict(_GOOD, **over)
    ptrs = ("q", "kn", "vn", "k", "v", "out", "lse") + (("cu",) if family == "ragged" else ()) + ("lens", "table", "ws")
    args = [_VP(a[n]) for n in ptrs] + [a[n] for n in ("B", "H", "Hkv", "Nq", "Ncap", "num_pages", "page_size", "max_pages", "d_new", "d",
                                                       "layout", "scale", "causal", "window")] + [_VP(a["logits"]), a["dtype"], None]
    rc = getattr(lib, f"fa_mi355x_fwd_{family}_lsink")(*args)
    return rc, lib.fa_mi355x_decode_last_error().decode()


_BAD_LSINK = [
    # the logits do not need the causal mask (the call goes on to the next check: the null q); a window still does
    (dict(causal=0, window=0, q=0), BAD_ARG, "null"), (dict(causal=0, window=0, logits=0, q=0, **_SLAB), BAD_ARG, "null"),
    (dict(causal=0, window=7), BAD_ARG, "causal"), (dict(window=-1, q=0, k=0), BAD_ARG, "negative"),
]


def _cases():
    out = []
    for family in FAMILIES:
        out += [(family, o, c, m) for o, c, m in _BAD_LSINK + _BAD_WINDOW + _BAD_FAMILY]
        out += [(family, dict(o, logits=0), c, m) for o, c, m in _BAD_WINDOW]   # (null logits: the _window call's checks)
    out += [("decode", dict(Nq=129), BAD_ARG, "Nq > 128"), ("ragged", dict(cu=0), BAD_ARG, "cu_seqlens_q"),
            ("ragged", dict(ws=0, window=1), BAD_ARG, "fa_mi355x_ragged_workspace_bytes"),
            ("extend", dict(H=1 << 12, Hkv=1, Nq=1 << 13, d=32, d_new=32), BAD_ARG, "2^25")]
    return out


def _id(case):
    return case[0] + "-" + ",".join(f"{k}={v}" for k, v in case[1].items())


@pytest.mark.parametrize("family,over,code,msg", _cases(), ids=[_id(c) for c in _cases()])
def test_lsink_forms_reject_each_bad_argument_before_any_hip_call(built, family, over, code, msg):
    rc, err = _call(built.decode(), family, **over)
    assert rc == code and err and msg in err, (rc, err)


# ---- the Python layer, under the recorder ----

def _attend_calls(rec):
    return [c for c in rec.calls if "workspace_bytes" not in c and "rope" not in c]


def _args(call):
    sym, rest = call.split("(", 1)
    return sym, rest[:-1].split(",")


def _logits(a, heads=None):
    import torch
    H = a["q"].shape[1] if a["q"].dim() == 3 or a["layout"] == "bhnd" else a["q"].shape[2]
    return torch.zeros(heads or H)


@pytest.mark.parametrize("family", FAMILIES)
def test_a_call_with_logits_sends_the_lsink_symbol_with_the_pointer_in_place(monkeypatch, family):
    from flash_attention_minitorch_amd import _lib
    from test_kv_ops_cpu import W, call, install, make
    rec = install(monkeypatch, False)
    sym = f"fa_mi355x_fwd_{family}_lsink"
    params = _lib.KV_LSINK_PARAMS[sym]
    for paged in (False, True):
        for fused in (False, True):
            for window in (None, 0, W):
                for layout in ("bnhd", "bhnd"):
                    a = make(family, "attend", paged=paged, fused=fused, layout=layout, sink_logits=_logits,
                             **({} if window is None else dict(window=window)))
                    rec.reset(a)
                    call(family, "attend", a)
                    calls = _attend_calls(rec)
                    assert len(calls) == 1, calls
                    got, args = _args(calls[0])
                    assert got == sym and len(args) == len(params), calls
                    f = dict(zip(params, args))
                    assert f["sink_logits"] == "sink_logits" and f["window"] == str(window or 0), (f, window)
                    assert (f["k_new"], f["v_new"]) == (("k_new", "v_new") if fused else ("null", "null"))
                    assert f["block_table"] == ("block_table" if paged else "null")
                    assert (f["q"], f["k_cache"], f["v_cache"], f["causal"]) == ("q", "k_cache", "v_cache", "1")
                    # the workspace is sized by the queries that were there: none of them is an lsink symbol
                    sizes = {c.split("(")[0] for c in rec.calls if "workspace_bytes" in c}
                    assert sizes and not [s for s in sizes if "lsink" in s], sizes
    # logits without the causal mask are a call; with rotary tables the roped append runs in front of the attend-only call
    a = make(family, "attend", sink_logits=_logits, causal=False)
    rec.reset(a)
    call(family, "attend", a)
    got, args = _args(_attend_calls(rec)[0])
    assert got == sym and dict(zip(params, args))["causal"] == "0"
    a = make(family, "attend", fused=True, rope=True, sink_logits=_logits)
    rec.reset(a)
    call(family, "attend", a)
    names = [c.split("(")[0] for c in rec.calls if "workspace_bytes" not in c]
    assert names == ["fa_mi355x_rope_append_ragged" if family == "ragged" else "fa_mi355x_rope_append", sym], names
    f = dict(zip(params, _args(rec.calls[-1])[1]))
    assert (f["k_new"], f["v_new"], f["sink_logits"]) == ("null", "null", "sink_logits")


@pytest.mark.parametrize("family", FAMILIES)
def test_no_logits_send_exactly_what_they_send_today(monkeypatch, family):
    """``sink_logits=None`` is today's call: the same symbols with the same arguments, for every kind of call."""
    from test_kv_ops_cpu import S, W, call, install, make
    rec = install(monkeypatch, False)
    for opts in ({}, dict(paged=True, fused=True), dict(window=W), dict(window=W, sink=S, paged=True), dict(fused=True, rope=True),
                 dict(causal=False), dict(softcap=30.0), dict(heads=2)) + (() if family == "ragged" else (dict(fp8=True),)):
        a = make(family, "attend", **opts)
        rec.reset(a)
        call(family, "attend", a)
        today = list(rec.calls)
        assert today and not [c for c in today if "lsink" in c]
        rec.reset(a)
        call(family, "attend", dict(a, sink_logits=None))
        assert rec.calls == today, opts


@pytest.mark.parametrize("family", FAMILIES)
def test_lsink_python_refusals_come_before_any_library_call(monkeypatch, family):
    import torch
    from test_kv_ops_cpu import H, S, W, call, install, make
    rec = install(monkeypatch, False)
    a = make(family, "attend")
    rec.reset(a)
    good = torch.zeros(H)
    for bad in (0.5, [0.0] * H, torch.zeros(H + 1), torch.zeros(1, H), torch.zeros(H, dtype=torch.float64), torch.zeros(H, dtype=torch.bfloat16),
                torch.zeros(2 * H)[::2], torch.zeros(H, device="meta")):
        with pytest.raises(ValueError, match="sink_logits"):
            call(family, "attend", dict(a, sink_logits=bad))
    with pytest.raises(ValueError, match="(?s)sink_logits.*sink="):
        call(family, "attend", dict(a, sink_logits=good, window=W, sink=S))
    with pytest.raises(ValueError, match="(?s)sink_logits.*softcap"):
        call(family, "attend", dict(a, sink_logits=good, softcap=30.0))
    with pytest.raises(ValueError, match="causal"):   # (a window still needs the causal mask)
        call(family, "attend", dict(a, sink_logits=good, window=W, causal=False))
    assert rec.calls == []
    if family != "ragged":   # (the ragged calls have no fp8 form at all)
        a = make(family, "attend", fp8=True)
        rec.reset(a)
        with pytest.raises(ValueError, match="(?s)sink_logits.*fp8"):
            call(family, "attend", dict(a, sink_logits=good))
        assert rec.calls == []
    # a sink of 0 and a cap of 0 are none: the windowed call with logits
    a = make(family, "attend", sink_logits=good, window=W, sink=0, softcap=0)
    rec.reset(a)
    call(family, "attend", a)
    assert _attend_calls(rec)[0].startswith(f"fa_mi355x_fwd_{family}_lsink(")


def test_sink_logits_is_the_last_keyword_of_the_three_calls():
    import inspect
    from flash_attention_minitorch_amd import device_ops
    for fn in (device_ops.flash_attn_decode, device_ops.flash_attn_extend, device_ops.flash_attn_ragged):
        p = inspect.signature(fn).parameters
        assert list(p)[-1] == "sink_logits" and p["sink_logits"].default is None


# ---- the model layer ----

def test_model_lsink_calls_under_the_recorder(monkeypatch):
    """The stack functions on a cache with learned sink logits (CPU tensors, no library): every attention call is the family's _lsink
    entry point with ITS LAYER's row of the logits, fused with the append; a prompt goes through the extend call (the square forward
    has no logit); a cache without logits sends no new keyword and makes the calls it made before."""
    import torch
    from flash_attention_minitorch_amd import modules_transformer as mt
    from test_device_ops_cpu import install_recorder

    rec = install_recorder(monkeypatch)
    B, P, H, Hkv, d, cap, W, L = 2, 200, 4, 2, 64, 512, 160, 2
    g = torch.Generator().manual_seed(0)
    x = torch.randn((B, P, H * d), generator=g).to(torch.bfloat16)
    wq, wk = (torch.randn(s, generator=g).to(torch.bfloat16) for s in ((H * d, H * d), (H * d, Hkv * d)))
    layers = [(wq, wk, wk, wq)] * L
    logits = torch.randn((L, H), generator=g)
    named = {"row0": logits[0], "row1": logits[1]}
    tail = lambda n, geo, w, li: f",{B},{H},{Hkv},{n},{geo},64,64,1,0.0,1,{w},row{li},1,null)"
    attends = lambda: [c for c in rec.calls if "workspace_bytes" not in c]

    cache = mt.KVCache(L, B, cap, H, d, torch.bfloat16, x.device, n_kv_head=Hkv, sink_logits=logits)
    assert cache.sink_logits.data_ptr() == logits.data_ptr()   # (the caller's tensor: an in-place update is what the next call reads)
    assert cache.learned_sinks(1)["sink_logits"].data_ptr() == logits[1].data_ptr() and set(cache.keywords(0)) == {"sink_logits"}
    assert cache.windowing() == {} and cache.capping() == {}
    rec.reset(named)
    mt.attention_stack_prefill(x, layers, H, cache)
    calls = attends()
    assert len(calls) == L and all(c.startswith("fa_mi355x_fwd_extend_lsink(") and c.endswith(tail(P, f"{cap},0,0,0", 0, li))
                                   for li, c in enumerate(calls)), calls
    assert {c.split("(")[0] for c in rec.calls if "workspace_bytes" in c} == {"fa_mi355x_extend_workspace_bytes"}
    assert cache.length_bound == P
    rec.reset(named)
    mt.attention_stack_step_fused(x[:, :1].contiguous(), layers, H, cache)
    mt.attention_stack_step(x[:, :3].contiguous(), layers, H, cache)
    calls = attends()
    assert len(calls) == 2 * L and all(c.startswith("fa_mi355x_fwd_decode_lsink(") for c in calls), calls
    assert all(c.endswith(tail(1, f"{cap},0,0,0", 0, li)) for li, c in enumerate(calls[:L]))
    assert all(c.endswith(tail(3, f"{cap},0,0,0", 0, li)) for li, c in enumerate(calls[L:]))
    assert all(_args(c)[1][1:3] == ["null", "null"] for c in calls[L:])   # (the caller-side append: attend only)
    assert all(_args(c)[1][1:3] != ["null", "null"] for c in calls[:L])
    rec.reset(named)
    mt.attention_stack_ragged(x[0, :50].contiguous(), [7, 40], layers, H, cache)
    calls = attends()
    assert len(calls) == L and all(c.startswith("fa_mi355x_fwd_ragged_lsink(") and c.endswith(tail(50, f"{cap},0,0,0", 0, li))
                                   for li, c in enumerate(calls)), calls
    rec.reset(named)
    mt.attention_stack_extend(x[:, :150].contiguous(), layers, H, cache)
    assert [c.split("(")[0] for c in attends()] == ["fa_mi355x_fwd_extend_lsink"] * L

    # a paged windowed cache with logits: the table, the pool's geometry, the window and the layer's row in one call
    paged = mt.PagedKVCache(L, B, cap, H, d, torch.bfloat16, x.device, n_kv_head=Hkv, page_size=128, n_pages=7, window=W, sink_logits=logits)
    kw = paged.keywords(1, k_new=1)
    assert set(kw) == {"k_new", "block_table", "window", "sink_logits"} and kw["window"] == W
    rec.reset({"table": paged.block_table, **named})
    mt.attention_stack_prefill_chunked(x, layers, H, paged, 150)
    calls = attends()
    assert [c.split("(")[0] for c in calls] == ["fa_mi355x_fwd_extend_lsink"] * L + ["fa_mi355x_fwd_decode_lsink"] * L, calls
    assert all(",table," in c for c in calls) and calls[0].endswith(tail(150, "0,7,128,4", W, 0)) and calls[3].endswith(tail(50, "0,7,128,4", W, 1))
    assert {c.split("(")[0] for c in rec.calls if "workspace_bytes" in c} == {"fa_mi355x_extend_window_workspace_bytes",
                                                                              "fa_mi355x_decode_window_workspace_bytes"}
    # a roped cache with logits: the roped append, then the attend-only call
    roped = mt.KVCache(L, B, cap, H, d, torch.bfloat16, x.device, n_kv_head=Hkv, rope=mt.Rotary.table(cap, 32), sink_logits=logits)
    rec.reset(named)
    mt.attention_stack_step_fused(x[:, :1].contiguous(), layers, H, roped)
    assert [c.split("(")[0] for c in attends()] == ["fa_mi355x_rope_append", "fa_mi355x_fwd_decode_lsink"] * L

    # a cache without logits sends no new keyword, and the calls it made before
    plain = mt.KVCache(L, B, cap, H, d, torch.bfloat16, x.device, n_kv_head=Hkv)
    assert plain.learned_sinks(0) == {} and plain.keywords(0) == {} and plain.sink_logits is None
    rec.reset({})
    mt.attention_stack_prefill(x, layers, H, plain)
    mt.attention_stack_step_fused(x[:, :1].contiguous(), layers, H, plain)
    names = [c.split("(")[0] for c in rec.calls]
    assert not [n for n in names if "lsink" in n or "window" in n] and "fa_mi355x_fwd_decode_append" in names, names


def test_cache_constructor_checks_the_logits_last():
    import torch
    from flash_attention_minitorch_amd import modules_transformer as mt
    L, H = 3, 2
    mk = lambda cls=mt.KVCache, **kw: cls(L, 1, 256, H, 32, torch.bfloat16, "cpu", **kw)
    good = torch.zeros(L, H)
    for bad in (0.5, [[0.0] * H] * L, torch.zeros(H), torch.zeros(L, H + 1), torch.zeros(L - 1, H), torch.zeros(L, H, dtype=torch.float64)):
        with pytest.raises(ValueError, match="sink_logits"):
            mk(sink_logits=bad)
    assert mk(sink_logits=good).sink_logits.shape == (L, H) and mk(mt.PagedKVCache, sink_logits=good).sink_logits is not None
    assert mk(n_kv_head=1, sink_logits=good).keywords(2)["sink_logits"].shape == (H,)   # (per QUERY head)
    noncontig = torch.zeros(H, L).T
    assert mk(sink_logits=noncontig).sink_logits.is_contiguous()
    with pytest.raises(ValueError, match="(?s)sink_logits.*sink="):
        mk(window=64, sink=4, sink_logits=good)
    assert set(mk(window=64, sink=0, sink_logits=good).keywords(0)) == {"window", "sink_logits"}
    with pytest.raises(ValueError, match="(?s)sink_logits.*softcap"):
        mk(softcap=30.0, sink_logits=good)
    with pytest.raises(ValueError, match="(?s)sink_logits.*fp8"):
        mk(kv_dtype=torch.float8_e4m3fn, sink_logits=good)
    # the documented order of first faults stays: ..., kv_dtype / kv_scale, the cap, then the logits
    with pytest.raises(ValueError, match="softcap must be"):
        mk(softcap=-1.0, sink_logits=torch.zeros(1))
    with pytest.raises(ValueError, match="kv_dtype must be"):
        mk(kv_dtype=torch.float16, sink_logits=torch.zeros(1))
    with pytest.raises(ValueError, match="window must be"):
        mk(window=0, sink_logits=torch.zeros(1))


# ==== the training side (include/flash_attn_mi355x_lsink.h, libflash_attn_mi355x_lsink.so) ==========================================

TRAIN_HEADER = "flash_attn_mi355x_lsink.h"
TRAIN = ["fa_mi355x_fwd_window_lsink", "fa_mi355x_sink_logits_grad_workspace_bytes", "fa_mi355x_sink_logits_grad", "fa_mi355x_lsink_last_error"]
TB, TH, THKV = 2, 4, 2                      # the GPU training cases: B = 2, H = 4, Hkv = 2
TRAIN_N, TRAIN_W = (1, 33, 129, 300), (0, 64)   # (0: no window)


def lsink_train_reference(q, k, v, do, W, a):
    """fp64 dense causal attention of (B, H, N, d) arrays (k, v already expanded to H heads) under a window of W (0: none) with the
    logit a[h] as one more column of head h's softmax, and its analytic backward.  Returns out, lse, dq, dk, dv, da (H,), and the
    terms of the logit gradient's bound: p = e^(a - lse) (B, H, N), |dO|_1 per row, delta."""
    q, k, v, do = (t.astype(np.float64) for t in (q, k, v, do))
    a = np.asarray(a, np.float64)
    N, d = q.shape[-2:]
    i, j = np.arange(N)[:, None], np.arange(N)[None, :]
    admit = (j <= i) & ((j > i - W) | (W == 0))
    tau = 1.0 / np.sqrt(d)
    s = np.where(admit, tau * q @ k.swapaxes(-1, -2), -np.inf)
    col = np.broadcast_to(a[None, :, None, None], s.shape[:-1] + (1,))
    lse = np.logaddexp.reduce(np.concatenate([s, col], -1), axis=-1)
    p = np.exp(s - lse[..., None])
    o = p @ v
    delta = (do * o).sum(-1)
    ds = p * (do @ v.swapaxes(-1, -2) - delta[..., None])
    ps = np.exp(a[None, :, None] - lse)
    da = -(ps * delta).sum((0, 2))
    return o, lse, tau * ds @ k, tau * ds.swapaxes(-1, -2) @ q, p.swapaxes(-1, -2) @ do, da, ps, np.abs(do).sum(-1), delta


def train_case(dtype, d, N, W):
    """The inputs of one GPU training case, a function of its parameters: q, do (B, H, N, d), k, v (B, Hkv, N, d) in U(-1, 1),
    rounded to the dtype; logits (H,) fp32 in U(-1, 3)."""
    rng = np.random.default_rng([7, dtype == "bf16", d, N, W])
    q, do = (_round(rand_u(rng, (TB, TH, N, d)), dtype) for _ in range(2))
    k, v = (_round(rand_u(rng, (TB, THKV, N, d)), dtype) for _ in range(2))
    return dict(q=q, k=k, v=v, do=do, logits=rng.uniform(-1.0, 3.0, TH).astype(np.float32))


def train_reference(c, W, with_logits=True):
    G = TH // THKV
    a = c["logits"].astype(np.float64) if with_logits else np.full(TH, -np.inf)
    with np.errstate(divide="ignore"):
        r = lsink_train_reference(c["q"], np.repeat(c["k"], G, 1), np.repeat(c["v"], G, 1), c["do"], W, a)
    N, d = c["q"].shape[-2:]
    dk, dv = (t.reshape(TB, THKV, G, N, d).sum(2) for t in (r[3], r[4]))
    return r[:3] + (dk, dv) + r[5:]


def test_training_reference_is_the_cache_reference_and_its_gradients_are_the_finite_differences():
    rng = np.random.default_rng(11)
    B, H, N, d, W = 1, 2, 9, 8, 4
    q, k, v, do = (rng.uniform(-1, 1, (B, H, N, d)) for _ in range(4))
    a = np.array([0.3, 2.0])
    o, lse, dq, dk, dv, da, ps, l1, delta = lsink_train_reference(q, k, v, do, W, a)
    # forward: the cache reference with all N tokens as queries on a cache of length N
    ro, rl = lsink_reference(q[0], k[0], v[0], [N] * H, W, 1.0 / np.sqrt(d), a)
    assert np.allclose(o[0], ro, atol=1e-13) and np.allclose(lse[0], rl, atol=1e-13)
    # backward: central differences of the scalar sum(dO o out)
    loss = lambda q_, k_, v_, a_: float((do * lsink_train_reference(q_, k_, v_, do, W, a_)[0]).sum())
    eps = 1e-6
    for h in range(H):
        e = np.zeros(H)
        e[h] = eps
        assert np.isclose((loss(q, k, v, a + e) - loss(q, k, v, a - e)) / (2 * eps), da[h], rtol=1e-6, atol=1e-9)
    for t, g, idx in ((0, dq, (0, 1, 5, 3)), (1, dk, (0, 0, 2, 7)), (2, dv, (0, 1, 4, 0))):
        args = [q.copy(), k.copy(), v.copy()]
        args[t][idx] += eps
        up = loss(*args, a)
        args[t][idx] -= 2 * eps
        assert np.isclose((up - loss(*args, a)) / (2 * eps), g[idx], rtol=1e-6, atol=1e-9)
    # a logit of -inf is the plain softmax: rows of P sum to 1, the logit gets no gradient
    with np.errstate(divide="ignore"):
        r0 = lsink_train_reference(q, k, v, do, W, np.full(H, -np.inf))
    assert np.allclose(r0[6], 0) and np.allclose(r0[5], 0) and np.all(ps > 0) and np.all(lse > r0[1])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_every_gpu_training_case_tells_the_logits_from_their_absence(d, dtype):
    for N in TRAIN_N:
        for W in TRAIN_W:
            c = train_case(dtype, d, N, W)
            with_, without = train_reference(c, W), train_reference(c, W, False)
            assert maxabs(with_[0], without[0]) >= 10 * TOL[dtype] and float(np.max(with_[1] - without[1])) >= 10 * TOL[dtype], (N, W)


def test_the_lsink_library_declares_exports_and_binds_its_symbols(built):
    from test_lib_cpu import _ctypes_kind, _prototypes
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", TRAIN_HEADER)).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(fa_mi355x_\w+)\s*\(", text))) == sorted(TRAIN) == sorted(built.LSINK_TRAIN_ABI)
    protos = _prototypes(TRAIN_HEADER)
    lib = built.lsink()
    for s in TRAIN:
        assert hasattr(lib, s), s
        res, args = built.LSINK_TRAIN_ABI[s]
        ret, kinds = protos[s]
        assert [_ctypes_kind(x) for x in args] == kinds and _ctypes_kind(res) == ret, s
        assert getattr(lib, s).argtypes == args and getattr(lib, s).restype is res, s
    names = _param_names(TRAIN_HEADER)
    assert names["fa_mi355x_fwd_window_lsink"] == "q k v out lse sink_logits B H Hkv N d layout softmax_scale window dtype stream".split()
    assert names["fa_mi355x_sink_logits_grad"] == "out out_grad lse sink_logits sink_grad workspace B H N d layout dtype stream".split()
    assert names["fa_mi355x_sink_logits_grad_workspace_bytes"] == "B H N d".split()
    # an eighth kernel library with a line of its own in the build script, loaded by build()
    assert "kernel_lib fa_lsink  _lsink" in open(os.path.join(ROOT, "compile_cuda.sh")).read()
    assert len(re.findall(r"^kernel_lib ", open(os.path.join(ROOT, "compile_cuda.sh")).read(), flags=re.M)) == 8
    # the header and DESIGN.md say why there is no backward kernel for q, k and v
    raw = open(os.path.join(ROOT, "include", TRAIN_HEADER)).read()
    assert "NO new kernel" in raw and "fa_mi355x_bwd_window" in raw
    assert "### Learned sinks (training)" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_the_lsink_library_holds_its_kernels_without_scratch_and_the_others_gain_none(built):
    kernels = _device_kernels(built.lib_path(built.LSINK_NAME))
    names = [k[0] for k in kernels]
    count = lambda pat: len([n for n in names if re.search(pat, n)])
    # bf16 and fp32, d in {32, 64, 128}: the forward (both layouts are one build) and the first stage of the gradient; one second stage
    assert count("win_lsink_fwd_kernel") == 6 and count("sink_grad_partial_kernel") == 6 and count("sink_grad_sum_kernel") == 1
    # (and the two non-template kernels of the shared headers that every training-side library carries)
    rest = [n for n in names if "lsink" not in n and "sink_grad" not in n]
    assert len(rest) == 2 and any("group_sum_kernel" in n for n in rest) and any("mfma_peak_kernel" in n for n in rest), rest
    for name, scratch, vgpr in kernels:
        assert scratch == 0 and vgpr <= 512, (name, scratch, vgpr)
    for other in (built.WINDOW_NAME, built.VARLEN_NAME):   # (they include the same kernel text: neither gains a kernel)
        assert not [k for k in _device_kernels(built.lib_path(other)) if "lsink" in k[0]]
    # the workspace: one float per (head, slice of 512 rows); at B = 2, H = 32, N = 8192 the first stage is 1024 workgroups
    lib = built.lsink()
    size = lib.fa_mi355x_sink_logits_grad_workspace_bytes
    assert size(2, 32, 8192, 64) == 32 * 32 * 4 and size(2, 4, 300, 32) == 4 * 2 * 4 and size(1, 1, 1, 128) == 4 and size(1, 1, 512, 64) == 4
    assert size(1, 1, 513, 64) == 8 and size(0, 4, 300, 32) == 0 and size(2, 4, -1, 32) == 0


_TGOOD = dict(q=16, k=16, v=16, out=16, lse=16, logits=16, B=2, H=4, Hkv=2, N=300, d=64, layout=1, scale=0.0, window=64, dtype=1)
_TBAD = [
    (dict(logits=0), "null sink_logits"), (dict(q=0), "null"), (dict(out=0), "null"), (dict(lse=0), "null"),
    (dict(window=0), "window"), (dict(window=-1), "window"), (dict(window=-1, logits=0, q=0), "window"),
    (dict(B=0), "positive"), (dict(N=0), "positive"), (dict(H=4, Hkv=3), "Hkv"), (dict(d=48), "d must be"), (dict(layout=2), "layout"),
    (dict(dtype=7), "dtype"), (dict(scale=-1.0), "softmax_scale"), (dict(scale=float("nan")), "softmax_scale"),
]
_GGOOD = dict(out=16, dout=16, lse=16, logits=16, grad=16, ws=16, B=2, H=4, N=300, d=64, layout=1, dtype=1)
_GBAD = [
    (dict(logits=0), "null sink_logits"), (dict(out=0), "null"), (dict(dout=0), "null"), (dict(lse=0), "null"), (dict(grad=0), "null"),
    (dict(ws=0), "null"), (dict(B=0), "positive"), (dict(H=-1), "positive"), (dict(d=48), "d must be"), (dict(layout=3), "layout"),
    (dict(dtype=9), "dtype"), (dict(out=8), "aligned"), (dict(dout=4), "aligned"),
]


@pytest.mark.parametrize("over,msg", _TBAD, ids=[",".join(f"{k}={v}" for k, v in o.items()) for o, _ in _TBAD])
def test_lsink_forward_rejects_each_bad_argument_before_any_hip_call(built, over, msg):
    a = dict(_TGOOD, **over)
    lib = built.lsink()
    rc = lib.fa_mi355x_fwd_window_lsink(*[_VP(a[n]) for n in ("q", "k", "v", "out", "lse", "logits")], a["B"], a["H"], a["Hkv"], a["N"], a["d"],
                                        a["layout"], a["scale"], a["window"], a["dtype"], None)
    err = lib.fa_mi355x_lsink_last_error().decode()
    assert rc == BAD_ARG and msg in err, (rc, err)


@pytest.mark.parametrize("over,msg", _GBAD, ids=[",".join(f"{k}={v}" for k, v in o.items()) for o, _ in _GBAD])
def test_sink_logits_grad_rejects_each_bad_argument_before_any_hip_call(built, over, msg):
    a = dict(_GGOOD, **over)
    lib = built.lsink()
    rc = lib.fa_mi355x_sink_logits_grad(*[_VP(a[n]) for n in ("out", "dout", "lse", "logits", "grad", "ws")], a["B"], a["H"], a["N"], a["d"],
                                        a["layout"], a["dtype"], None)
    err = lib.fa_mi355x_lsink_last_error().decode()
    assert rc == BAD_ARG and msg in err, (rc, err)


def _install_train_recorder(monkeypatch):
    from flash_attention_minitorch_amd import _lib
    from test_device_ops_cpu import install_recorder
    rec = install_recorder(monkeypatch)
    monkeypatch.setattr(_lib, "window", lambda: rec)
    monkeypatch.setattr(_lib, "lsink", lambda: rec)
    return rec


def test_flash_attn_gqa_with_logits_calls_the_lsink_forward_the_window_backward_and_the_grad_only_when_wanted(monkeypatch):
    import inspect
    import torch
    from flash_attention_minitorch_amd import device_ops as dev
    rec = _install_train_recorder(monkeypatch)
    B, N, H, Hkv, d = 2, 40, 4, 2, 64
    assert list(inspect.signature(dev.flash_attn_gqa).parameters)[-1] == "sink_logits"
    mk = lambda: (torch.zeros(B, N, H, d, dtype=torch.bfloat16), torch.zeros(B, N, Hkv, d, dtype=torch.bfloat16),
                  torch.zeros(B, N, Hkv, d, dtype=torch.bfloat16))
    for window, w_sent in ((None, N), (0, N), (16, 16), (500, N)):
        for wants in (True, False):
            q, k, v = (t.requires_grad_() for t in mk())
            a = torch.zeros(H, requires_grad=wants)
            rec.reset(dict(q=q, k=k, v=v, a=a))
            o = dev.flash_attn_gqa(q, k, v, True, None, "bnhd", window, sink_logits=a)
            assert [c.split("(")[0] for c in rec.calls] == ["fa_mi355x_fwd_window_lsink"]
            assert rec.calls[0].endswith(f",a,{B},{H},{Hkv},{N},{d},1,0.0,{w_sent},1,null)") and rec.calls[0].startswith("fa_mi355x_fwd_window_lsink(q,k,v,")
            rec.calls.clear()
            o.sum().backward()
            names = [c.split("(")[0] for c in rec.calls]
            tail = ["fa_mi355x_sink_logits_grad_workspace_bytes", "fa_mi355x_sink_logits_grad"] if wants else []
            assert names == ["fa_mi355x_bwd_window_workspace_bytes", "fa_mi355x_bwd_window"] + tail, names
            assert rec.calls[1].endswith(f",{B},{H},{Hkv},{N},{d},1,0.0,{w_sent},0,1,null)")   # (sink = 0: the plain windowed backward)
            assert (a.grad is not None and a.grad.shape == (H,) and a.grad.dtype == torch.float32) if wants else a.grad is None
            assert q.grad.dtype == torch.bfloat16 and k.grad.shape == k.shape
    # None is today's call; the refusals come by name, before any library call
    q, k, v = mk()
    rec.reset({})
    dev.flash_attn_gqa(q, k, v, True, None, "bnhd", 16)
    today = list(rec.calls)
    rec.reset({})
    dev.flash_attn_gqa(q, k, v, True, None, "bnhd", 16, sink_logits=None)
    assert rec.calls == today and not [c for c in today if "lsink" in c]
    rec.reset({})
    a = torch.zeros(H)
    for kw, msg in ((dict(causal=False), "causal"), (dict(causal=True, softcap=30.0), "softcap"), (dict(causal=True, window=16, sink=4), "sink=")):
        with pytest.raises(ValueError, match="(?s)sink_logits.*" + msg):
            dev.flash_attn_gqa(q, k, v, layout="bnhd", sink_logits=a, **kw)
    for bad in (torch.zeros(H + 1), torch.zeros(H, dtype=torch.float64), 0.5):
        with pytest.raises(ValueError, match="sink_logits"):
            dev.flash_attn_gqa(q, k, v, True, sink_logits=bad)
    assert rec.calls == []


def test_model_functions_hand_each_layer_its_row_of_logits(monkeypatch):
    import torch
    from flash_attention_minitorch_amd import modules_transformer as mt
    rec = _install_train_recorder(monkeypatch)
    B, N, H, Hkv, d, L = 2, 40, 4, 2, 64, 2
    g = torch.Generator().manual_seed(0)
    x = torch.randn((B, N, H * d), generator=g).to(torch.bfloat16)
    wq, wk = (torch.randn(s, generator=g).to(torch.bfloat16) for s in ((H * d, H * d), (H * d, Hkv * d)))
    layers = [(wq, wk, wk, wq)] * L
    logits = torch.zeros(L, H)
    for kw, w_sent in ((dict(), N), (dict(window=16), 16), (dict(window=16, rope=mt.Rotary.table(64, 32)), 16), (dict(fold_scale=True), N)):
        rec.reset({"row0": logits[0], "row1": logits[1]})
        mt.attention_stack(x, layers, H, sink_logits=logits, **kw)
        calls = [c for c in rec.calls if "lsink" in c]
        assert len(calls) == L and len([c for c in rec.calls if c.startswith("fa_mi355x_fwd")]) == L
        for li, c in enumerate(calls):
            args = c[:-1].split(",")
            assert c.startswith("fa_mi355x_fwd_window_lsink(") and args[5] == f"row{li}" and args[-3] == str(w_sent), c
    rec.reset({"row1": logits[1]})
    mt.multi_head_attention(x, wq, wk, wk, wq, H, sink_logits=logits[1], fused_layout=False)
    assert [c.split("(")[0] for c in rec.calls] == ["fa_mi355x_fwd_window_lsink"] and ",row1," in rec.calls[0]
    with pytest.raises(ValueError, match="sink_logits"):
        mt.attention_stack(x, layers, H, sink_logits=logits[0])
    with pytest.raises(ValueError, match="sink_logits"):
        mt.attention_stack(x, layers, H, sink_logits=torch.zeros(L + 1, H))
