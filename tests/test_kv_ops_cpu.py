"""The KV-cache layer of device_ops on the CPU: what flash_attn_decode / _extend / _ragged, decode_ / extend_ / ragged_append and the three
*_workspace functions send to the C library, what they return and which arguments they reject with which message, held against
tests/kv_call_traces.json.  The file was recorded ONCE, on the commit before the layer was given one call path, and the layer has to
reproduce it string for string (``python tests/test_kv_ops_cpu.py --record`` rewrites it: not something a refactor does).

Everything runs under the recorder of tests/test_device_ops_cpu.py (CPU tensors, no library, pointers logged by name).  That recorder
answers 0 to every size query but one; SizedRecorder answers WS_BYTES to all of them, so that a sized workspace and the "workspace too
small" refusal show up.  The last test holds ``_lib.KV_PARAMS``, the table the layer's one dispatch reads every call's positional order
from, against the prototypes under include/ and against the ctypes ABI tables."""
import ctypes
import inspect
import itertools
import json
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]   # (for the --record run: pytest has both on the path already)
from test_device_ops_cpu import _describe, install_recorder  # noqa: E402

from flash_attention_minitorch_amd import _lib, device_ops as dev  # noqa: E402

TRACES = os.path.join(HERE, "kv_call_traces.json")
F32, BF16, F16, I32 = torch.float32, torch.bfloat16, torch.float16, torch.int32
FP8 = torch.float8_e4m3fn
WS_BYTES = 4096
B, H, HKV, NQ, T, NCAP, DP, W, S = 2, 4, 2, 3, 7, 256, 64, 100, 4
PAGES, PAGE, MP = 5, 128, 2
FAMILIES = ("decode", "extend", "ragged")
FUNCS = {("decode", "attend"): dev.flash_attn_decode, ("extend", "attend"): dev.flash_attn_extend, ("ragged", "attend"): dev.flash_attn_ragged,
         ("decode", "append"): dev.decode_append, ("extend", "append"): dev.extend_append, ("ragged", "append"): dev.ragged_append,
         ("decode", "workspace"): dev.decode_workspace, ("extend", "workspace"): dev.extend_workspace,
         ("ragged", "workspace"): dev.ragged_workspace}
PARAMS = {k: set(inspect.signature(f).parameters) for k, f in FUNCS.items()}


class SizedRecorder:
    """The recorder with WS_BYTES as the answer of every *workspace_bytes query (the call is logged as before)."""

    def __init__(self, inner):
        self.inner = inner

    def __getattr__(self, sym):
        got = getattr(self.inner, sym)
        if "workspace_bytes" not in sym:
            return got

        def fn(*args):
            got(*args)
            return WS_BYTES
        return fn


def install(monkeypatch, sized):
    rec = install_recorder(monkeypatch)
    if sized:
        rec = SizedRecorder(rec)
        monkeypatch.setattr(_lib, "decode", lambda: rec)
    return rec


def _rows(layout, b, n, h, d):
    return (b, n, h, d) if layout == "bnhd" else (b, h, n, d)


def make(family, kind, paged=False, fused=False, fp8=False, rope=False, layout="bnhd", d=DP, dtype=BF16, heads=H, ncap=NCAP, **more):
    """The arguments of one call, by parameter name (``more``: further ones, a function of the rest or the value)."""
    ragged = family == "ragged"
    cache = _rows(layout, PAGES, PAGE, HKV, DP) if paged else _rows(layout, B, ncap, HKV, DP)
    a = dict(layout=layout, q=torch.zeros((T, heads, d) if ragged else _rows(layout, B, NQ, heads, d), dtype=dtype),
             k_cache=torch.zeros(cache, dtype=FP8 if fp8 else dtype), v_cache=torch.zeros(cache, dtype=FP8 if fp8 else dtype))
    if ragged:
        a["cu_seqlens_q"] = torch.tensor([0, 3, 7], dtype=I32)
    if paged:
        a["block_table"] = torch.zeros(B, MP, dtype=I32)
    if fused or kind == "append":
        new = (T, HKV, d) if ragged else _rows(layout, B, NQ, HKV, d)
        a["k_new"], a["v_new"] = torch.zeros(new, dtype=dtype), torch.zeros(new, dtype=dtype)
    if fp8:
        a["k_scale"], a["v_scale"] = torch.ones(HKV), torch.ones(HKV)
    if rope:
        a["rotary_cos"], a["rotary_sin"] = dev.rotary_table(512, 32)
    for n, v in more.items():
        a[n] = v(a) if callable(v) else v
    return a


def call(family, kind, a):
    return FUNCS[family, kind](**{n: v for n, v in a.items() if n in PARAMS[family, kind]})


def run_trace(rec, family, kind, opts):
    a = make(family, kind, **opts)
    rec.reset(a)
    r = call(family, kind, a)
    return rec.calls + ["-> " + _describe(rec, r)]


# ---- the calls whose traces are recorded: name -> (sized recorder?, family, kind, make()'s options) ----

FEATURES = {"plain": {}, "window": dict(window=W), "sink": dict(window=W, sink=S), "fp8": dict(fp8=True)}
_out = lambda a: torch.zeros(a["q"].shape)
_lse = lambda a: torch.zeros((a["q"].shape[1], T) if a["q"].dim() == 3 else (B, a["q"].shape[1 if a["layout"] == "bhnd" else 2], NQ))
_ws = lambda a: torch.zeros(WS_BYTES // 4)
_lens = lambda a: torch.full((B,), 9, dtype=I32)
_q_rot = lambda a: torch.zeros_like(a["q"])


def trace_cases():
    c = {}
    for family, paged, fused, (feat, fopts), rope, d, layout in itertools.product(
            FAMILIES, (False, True), (False, True), FEATURES.items(), (False, True), (64, 48), ("bnhd", "bhnd")):
        if family == "ragged" and feat == "fp8":
            continue
        name = "/".join(("matrix", family, "paged" if paged else "slab", "fused" if fused else "attend", feat, "rope" if rope else "norope",
                         f"d{d}", layout))
        c[name] = (False, family, "attend", dict(paged=paged, fused=fused, rope=rope, d=d, layout=layout, **fopts))
    for sized in (False, True):   # Hkv = H: the ungrouped entry point and size query of the plain slab decode
        c[f"top/decode/mha/{'sized' if sized else 'zero'}"] = (sized, "decode", "attend", dict(heads=HKV))
        c[f"top/decode/mha_fused/{'sized' if sized else 'zero'}"] = (sized, "decode", "attend", dict(heads=HKV, fused=True))
    c["top/decode/mha_ncap2048"] = (False, "decode", "attend", dict(heads=HKV, ncap=2048))   # (the stub's size is non-zero there)
    tops = {
        "f32": dict(dtype=F32), "f32_fused_paged": dict(dtype=F32, fused=True, paged=True),
        "buffers": dict(out=_out, lse=_lse, workspace=_ws, cache_seqlens=_lens),
        "buffers_d48": dict(d=48, out=_out, lse=_lse, workspace=_ws, cache_seqlens=_lens),
        "buffers_window_paged_fused": dict(paged=True, fused=True, window=W, out=_out, lse=_lse, workspace=_ws, cache_seqlens=_lens),
        "no_workspace": {}, "no_workspace_sink_paged": dict(paged=True, window=W, sink=S),
        "q_rot": dict(rope=True, fused=True, q_rot=_q_rot, cache_seqlens=_lens), "q_rot_d48": dict(rope=True, fused=True, d=48, q_rot=_q_rot),
        "q_rot_is_q": dict(rope=True, q_rot=lambda a: a["q"]), "q_rot_d48_out": dict(rope=True, d=48, q_rot=_q_rot, out=_out, window=W),
        "scale": dict(softmax_scale=0.125), "scale_d48": dict(d=48, softmax_scale=0.125, fused=True),
        "noncausal": dict(causal=False), "noncausal_paged_fused": dict(causal=False, paged=True, fused=True),
        "window0": dict(window=0), "sink0": dict(window=W, sink=0), "sink0_no_window": dict(sink=0), "window0_sink": dict(window=0, sink=S),
        "interleaved": dict(rope=True, fused=True, rotary_interleaved=True), "bhnd_buffers": dict(layout="bhnd", out=_out, lse=_lse),
    }
    for family, (top, opts) in itertools.product(FAMILIES, tops.items()):
        c[f"top/{family}/{top}"] = (True, family, "attend", opts)
    c["top/decode/fp8_buffers"] = (True, "decode", "attend", dict(fp8=True, fused=True, out=_out, workspace=_ws, cache_seqlens=_lens))
    c["top/extend/fp8_no_scales"] = (True, "extend", "attend", dict(fp8=True, paged=True, k_scale=None, v_scale=None))
    for paged in (False, True):
        c[f"top/ragged/max_pages/{'paged' if paged else 'slab'}"] = (True, "ragged", "attend", dict(paged=paged, max_pages=MP if paged else None))
    for family, paged, feat, layout, d in itertools.product(FAMILIES, (False, True), ("plain", "fp8", "rope"), ("bnhd", "bhnd"), (64, 48)):
        if family == "ragged" and feat == "fp8":
            continue
        c["/".join(("append", family, "paged" if paged else "slab", feat, layout, f"d{d}"))] = (
            False, family, "append", dict(paged=paged, fp8=feat == "fp8", rope=feat == "rope", layout=layout, d=d))
    for family in FAMILIES:
        c[f"append/{family}/lens"] = (False, family, "append", dict(cache_seqlens=_lens))
        c[f"append/{family}/f32_paged_interleaved"] = (False, family, "append", dict(dtype=F32, paged=True, rope=True, rotary_interleaved=True))
    c["append/decode/fp8_no_scales"] = (False, "decode", "append", dict(fp8=True, k_scale=None, v_scale=None))
    where = {"slab": {}, "table": dict(paged=True), "max_pages": dict(paged=True, block_table=None, max_pages=MP)}
    for sized, family, (wn, wopts), (feat, fopts) in itertools.product((False, True), FAMILIES, where.items(), list(FEATURES.items())[:3]):
        c["/".join(("workspace", "sized" if sized else "zero", family, wn, feat))] = (sized, family, "workspace", dict(**wopts, **fopts))
    for family in FAMILIES:
        c[f"workspace/sized/{family}/bhnd_d48_fp8"] = (True, family, "workspace", dict(layout="bhnd", d=48, fp8=family != "ragged"))
    return c


# ---- the calls that are refused: (family, kind) -> name -> (make()'s options, the faulty arguments) ----

def _cpu(t):
    t.on_cpu = True
    return t


_on = lambda n, f: (lambda a: f(a[n]))
_nc = lambda t: torch.zeros(t.shape[:-1] + (2 * t.shape[-1],), dtype=t.dtype)[..., :t.shape[-1]]
_big_tables = lambda i: (lambda a: dev.rotary_table(512, 128)[i])
_both = lambda f: dict(k_cache=_on("k_cache", f), v_cache=_on("v_cache", f))
_new = lambda f: dict(k_new=_on("k_new", f), v_new=_on("v_new", f))
_new_like = lambda *shape: _new(lambda t: torch.zeros(shape, dtype=t.dtype))


def _options():   # window, sink: every function of the layer takes them but the appends
    return {
        "window_type": ({}, dict(window="8")), "window_negative": ({}, dict(window=-1)),
        "sink_type": ({}, dict(window=8, sink=2.0)), "sink_negative": ({}, dict(window=8, sink=-1)),
        "sink_without_window": ({}, dict(sink=4)),
    }


def _rotary(kind):
    c = {
        "rotary_one_table": (dict(rope=True), dict(rotary_sin=None)),
        "rotary_dtype": (dict(rope=True), dict(rotary_cos=_on("rotary_cos", lambda t: t.double()))),
        "rotary_shape": (dict(rope=True), dict(rotary_sin=_on("rotary_sin", lambda t: t[:, :8].contiguous()))),
        "rotary_device": (dict(rope=True), dict(rotary_cos=_on("rotary_cos", lambda t: t.to("meta")))),
        "rotary_noncontiguous": (dict(rope=True), dict(rotary_cos=_on("rotary_cos", lambda t: t.t().contiguous().t()))),
        "rotary_exceeds": ({}, dict(rotary_cos=_big_tables(0), rotary_sin=_big_tables(1))),
    }
    if kind == "attend":
        c["q_rot_without_tables"] = ({}, dict(q_rot=_q_rot))
        c["q_rot_shape"] = (dict(rope=True), dict(q_rot=torch.zeros(3)))
    else:
        c["q_rot"] = (dict(rope=True), dict(q_rot=torch.zeros(3)))
    return c


def _new_tokens(family, kind):
    fused = dict(fused=True) if kind == "attend" else {}
    ragged = family == "ragged"
    c = {
        "new_rank": (fused, _new(lambda t: t[None])),
        "new_dtype": (fused, dict(v_new=_on("v_new", lambda t: t.float()))),
        "new_heads": (fused, _new_like(T, 4, DP) if ragged else _new_like(B, NQ, 4, DP)),
        "new_head_dim": (fused, _new_like(T, HKV, 65) if ragged else _new_like(B, NQ, HKV, 65)),
        "new_device": (fused, dict(k_new=_on("k_new", lambda t: t.to("meta")))),
        "new_noncontiguous": (fused, dict(k_new=_on("k_new", _nc))),
    }
    if kind == "attend":
        c["k_new_alone"] = (fused, dict(v_new=None))
        c["new_count"] = (fused, _new_like(T - 1, HKV, DP) if ragged else _new_like(B, NQ + 1, HKV, DP))
    if not ragged:
        c["fp8_new_dtype"] = (dict(fp8=True, **fused), _new(lambda t: t.float()))
        if kind == "attend":
            c["new_batch"] = (dict(paged=True, **fused), _new_like(3, NQ, HKV, DP))
    return c


def _fp8_scales():
    return {
        "scales_without_fp8": ({}, dict(k_scale=torch.ones(HKV))),
        "scale_dtype": (dict(fp8=True), dict(k_scale=torch.ones(HKV, dtype=torch.float64))),
        "scale_shape": (dict(fp8=True), dict(v_scale=torch.ones(3))),
    }


def single_cases():
    c = {}
    for family in FAMILIES:
        ragged = family == "ragged"
        att = {
            **_options(), "window_noncausal": ({}, dict(window=8, causal=False)), **_rotary("attend"), **_new_tokens(family, "attend"),
            "layout": ({}, dict(layout="nbhd")), "dtype_f16": (dict(dtype=F16), {}),
            "v_cache_dtype": ({}, dict(v_cache=_on("v_cache", lambda t: t.float()))), "q_dtype": ({}, dict(q=_on("q", lambda t: t.float()))),
            "v_cache_shape": ({}, dict(v_cache=_on("v_cache", lambda t: t[:, :128].contiguous()))), "caches_3d": ({}, _both(lambda t: t[0])),
            "q_rank": ({}, dict(q=_on("q", lambda t: t[None]))), "heads": (dict(heads=3), {}), "head_dim": (dict(d=80), {}),
            "cache_seqlens": ({}, dict(cache_seqlens=torch.zeros(B, dtype=torch.int64))),
            "table_type": (dict(paged=True), dict(block_table=[[0, 1], [2, 3]])),
            "table_dtype": (dict(paged=True), dict(block_table=_on("block_table", lambda t: t.long()))),
            "page_size": (dict(paged=True), _both(lambda t: t[:, :64].contiguous())),
            "cpu": ({}, dict(q=_on("q", _cpu))), "device": ({}, _both(lambda t: t.to("meta"))), "noncontiguous": ({}, dict(q=_on("q", _nc))),
            "out": ({}, dict(out=lambda a: torch.zeros(a["q"].shape[:-1] + (32,)))), "lse": ({}, dict(lse=torch.zeros(5))),
            "workspace_small": ({}, dict(workspace=torch.zeros(4))),
        }
        if ragged:
            att.update({"fp8": (dict(fp8=True, k_scale=None, v_scale=None), {}), "cu": ({}, dict(cu_seqlens_q=torch.zeros(4, dtype=I32))),
                        "max_pages": ({}, dict(max_pages=3)), "max_pages_paged": (dict(paged=True), dict(max_pages=3))})
        else:
            att.update({**_fp8_scales(), "batch": ({}, _both(lambda t: torch.zeros((3,) + t.shape[1:], dtype=t.dtype))),
                        "fp8_v_cache": (dict(fp8=True), dict(v_cache=_on("v_cache", lambda t: t.to(BF16)))),
                        "fp8_q_dtype": (dict(fp8=True), dict(q=_on("q", lambda t: t.float()))), "fp8_window": (dict(fp8=True), dict(window=8)),
                        "pool_rank": (dict(paged=True), _both(lambda t: t[0])), "q_rank_paged": (dict(paged=True), dict(q=_on("q", lambda t: t[None]))),
                        "heads_paged": (dict(paged=True, heads=3), {})})
        c[family, "attend"] = att
        app = {
            **_rotary("append"), **_new_tokens(family, "append"), "layout": ({}, dict(layout="nbhd")), "dtype_f16": (dict(dtype=F16), {}),
            "v_cache_dtype": ({}, dict(v_cache=_on("v_cache", lambda t: t.float()))),
            "v_cache_shape": ({}, dict(v_cache=_on("v_cache", lambda t: t[:, :128].contiguous()))), "caches_3d": ({}, _both(lambda t: t[0])),
            "cache_seqlens": ({}, dict(cache_seqlens=torch.zeros(B, dtype=torch.int64))),
            "table_type": (dict(paged=True), dict(block_table=[[0, 1], [2, 3]])),
            "table_dtype": (dict(paged=True), dict(block_table=_on("block_table", lambda t: t.long()))),
            "page_size": (dict(paged=True), _both(lambda t: t[:, :64].contiguous())),
            "cpu": ({}, dict(k_cache=_on("k_cache", _cpu))), "cache_noncontiguous": ({}, dict(v_cache=_on("v_cache", _nc))),
        }
        if ragged:
            app.update({"fp8": (dict(fp8=True, k_scale=None, v_scale=None), {}), "cu": ({}, dict(cu_seqlens_q=torch.zeros(4, dtype=I32))),
                        "cu_type": ({}, dict(cu_seqlens_q=None))})
        else:
            app.update(_fp8_scales())
        if family == "decode":
            app.update({"too_many_fp8": (dict(fp8=True), _new_like(B, 129, HKV, DP)), "too_many_rotary": (dict(rope=True), _new_like(B, 129, HKV, DP))})
        c[family, "append"] = app
        ws = {
            **_options(), "table_type": (dict(paged=True), dict(block_table=[[0, 1]])),
            "table_rank": (dict(paged=True), dict(block_table=torch.zeros(3, dtype=I32))),
            "max_pages_zero": (dict(paged=True), dict(block_table=None, max_pages=0)), "q_rank": ({}, dict(q=_on("q", lambda t: t[None]))),
            "q_rank_paged": (dict(paged=True), dict(q=_on("q", lambda t: t[None]))), "pool_rank": (dict(paged=True), _both(lambda t: t[0])),
            "page_size": (dict(paged=True), _both(lambda t: t[:, :64].contiguous())), "heads": (dict(heads=3), {}),
            "heads_paged": (dict(paged=True, heads=3), {}), "caches_3d": ({}, _both(lambda t: t[0])),
        }
        if ragged:
            ws.update({"layout": ({}, dict(layout="nbhd")), "cu": ({}, dict(cu_seqlens_q=torch.zeros(4, dtype=I32))),
                       "cu_paged": (dict(paged=True), dict(cu_seqlens_q=torch.zeros(3, dtype=torch.int64)))})
        else:
            ws["batch"] = ({}, _both(lambda t: torch.zeros((3,) + t.shape[1:], dtype=t.dtype)))
        c[family, "workspace"] = ws
    return c


# two-fault calls: the missing GPU and the small workspace (the two checks the three families placed differently) beside every other
# fault of the function, and these
EXTRA_PAIRS = [("layout", "v_cache_shape"), ("v_cache_shape", "v_cache_dtype"), ("q_dtype", "v_cache_shape"), ("layout", "window_negative"),
               ("head_dim", "cache_seqlens"), ("out", "lse"), ("noncontiguous", "out"), ("k_new_alone", "layout"), ("new_dtype", "cache_seqlens"),
               ("rotary_exceeds", "out"), ("rotary_exceeds", "lse"), ("fp8_window", "scale_shape"), ("caches_3d", "layout"), ("heads", "lse"),
               ("sink_without_window", "rotary_one_table"), ("q_rot_without_tables", "k_new_alone"), ("table_dtype", "cache_seqlens"),
               ("cu", "cache_seqlens"), ("max_pages", "cu"), ("page_size", "table_dtype"), ("new_heads", "cache_seqlens"), ("device", "out"),
               ("scales_without_fp8", "cache_seqlens"), ("cache_noncontiguous", "cache_seqlens"), ("too_many_fp8", "scale_shape"),
               ("window_type", "max_pages_zero"), ("heads", "sink_negative"), ("q_rank", "window_negative"), ("dtype_f16", "layout"),
               ("dtype_f16", "v_cache_shape"), ("fp8", "layout"), ("fp8", "cu")]


def _merged(x, y):
    """Two faults in one call: (options, arguments), or None where they do not combine (they set the same thing)."""
    (xo, xm), (yo, ym) = x, y
    if set(xm) & set(ym) or any(xo[n] != yo[n] for n in set(xo) & set(yo)):
        return None
    return {**xo, **yo}, {**xm, **ym}


def pair_cases():
    c = {}
    for key, singles in single_cases().items():
        pairs = [(x, y) for x in ("cpu", "workspace_small") for y in singles if y != x] + EXTRA_PAIRS
        for x, y in pairs:
            if x in singles and y in singles and (y, x) not in c.get(key, {}):
                both = _merged(singles[x], singles[y])
                if both is not None:
                    c.setdefault(key, {})[x, y] = both
    return c


def run_error(rec, family, kind, case):
    opts, faults = case
    try:
        a = make(family, kind, **opts, **faults)
    except Exception as e:   # (two faults that cannot be put into one set of arguments)
        return f"unbuildable: {type(e).__name__}"
    rec.reset(a)
    try:
        call(family, kind, a)
    except Exception as e:
        return f"{type(e).__name__}: {e}"
    return "ok: " + ";".join(rec.calls)


def _error_name(key, case):
    return f"{key[0]}_{key[1]}/" + (case if isinstance(case, str) else "+".join(case))


def record():
    out = {"traces": {}, "errors": {}, "pairs": {}}
    with pytest.MonkeyPatch.context() as mp:
        recs = {False: install(mp, False)}
        for name, (sized, family, kind, opts) in trace_cases().items():
            if not sized:
                out["traces"][name] = run_trace(recs[False], family, kind, opts)
    with pytest.MonkeyPatch.context() as mp:
        rec = install(mp, True)
        for name, (sized, family, kind, opts) in trace_cases().items():
            if sized:
                out["traces"][name] = run_trace(rec, family, kind, opts)
        for key, singles in single_cases().items():
            for n, case in singles.items():
                out["errors"][_error_name(key, n)] = run_error(rec, *key, case)
        for key, pairs in pair_cases().items():
            for n, case in pairs.items():
                out["pairs"][_error_name(key, n)] = run_error(rec, *key, case)
    return out


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_kv_ops_cpu.py --record"
    with open(TRACES, "w") as f:
        json.dump(record(), f, indent=1)
        f.write("\n")
    sys.exit(0)

with open(TRACES) as f:
    RECORDED = json.load(f)


@pytest.fixture
def recs(monkeypatch):
    zero = install(monkeypatch, False)
    return {False: zero, True: SizedRecorder(zero)}


def _use(monkeypatch, recs, sized):
    monkeypatch.setattr(_lib, "decode", lambda: recs[sized])
    return recs[sized]


def test_the_recording_covers_every_case():
    assert set(RECORDED["traces"]) == set(trace_cases())
    assert len([n for n in RECORDED["traces"] if n.startswith("matrix/")]) == 352
    assert set(RECORDED["errors"]) == {_error_name(k, n) for k, s in single_cases().items() for n in s}
    assert set(RECORDED["pairs"]) == {_error_name(k, n) for k, p in pair_cases().items() for n in p}
    assert not [n for n, e in RECORDED["errors"].items() if e.startswith(("ok", "unbuildable"))]


@pytest.mark.parametrize("group", sorted({"/".join(n.split("/")[:2]) for n in trace_cases()}))
def test_call_traces(monkeypatch, recs, group):
    """Every recorded call makes the C calls it made, argument for argument, and returns what it returned."""
    for name, (sized, family, kind, opts) in trace_cases().items():
        if name.startswith(group + "/"):
            assert run_trace(_use(monkeypatch, recs, sized), family, kind, opts) == RECORDED["traces"][name], name


@pytest.mark.parametrize("key", sorted(single_cases()), ids="_".join)
def test_single_faults(monkeypatch, recs, key):
    rec = _use(monkeypatch, recs, True)
    for n, case in single_cases()[key].items():
        assert run_error(rec, *key, case) == RECORDED["errors"][_error_name(key, n)], n


# The two-fault calls that report their OTHER fault since the three families share one check order: name -> the message now, and
# below each group the message before (the recorded one).  flash_attn_decode / _extend asked for the GPU before they looked at the
# devices, out, lse and the workspace's size, flash_attn_ragged after; and they read the dtypes before they compared the caches'
# shapes, flash_attn_ragged after.  Both orders are flash_attn_ragged's now, whose two-fault calls the per-feature tests pin.
_GPU_LAST = {"device": "ValueError: q, k_cache and v_cache must live on one device",
             "out": "ValueError: out must be a contiguous float32 tensor of q's shape",
             "lse": "ValueError: lse must be a contiguous float32 tensor of shape (B, H, Nq)",
             "workspace_small": "ValueError: workspace too small: size it with {}_workspace()"}
CHANGED_WINNERS = {
    # before: "FlashAttnLibraryError: flash_attn_decode [flash_attn_extend] needs GPU tensors; there is no CPU fallback"
    **{f"{family}_attend/cpu+{fault}": message.format(family) for family in ("decode", "extend") for fault, message in _GPU_LAST.items()},
    # before: "TypeError: q, k_cache and v_cache must share one dtype"
    "decode_attend/q_dtype+v_cache_shape": "ValueError: k_cache and v_cache must have one shape",
    "extend_attend/q_dtype+v_cache_shape": "ValueError: k_cache and v_cache must have one shape",
    # before: "TypeError: unsupported dtype torch.float16: use float32 or bfloat16"
    "decode_attend/dtype_f16+v_cache_shape": "ValueError: k_cache and v_cache must have one shape",
    "extend_attend/dtype_f16+v_cache_shape": "ValueError: k_cache and v_cache must have one shape",
}


@pytest.mark.parametrize("key", sorted(pair_cases()), ids="_".join)
def test_two_faults(monkeypatch, recs, key):
    """A call with two faults reports one of them, in the words of the call that has that fault alone; which one is recorded, and
    CHANGED_WINNERS lists the calls where it is the other one now."""
    rec = _use(monkeypatch, recs, True)
    for (x, y), case in pair_cases()[key].items():
        name = _error_name(key, (x, y))
        got = run_error(rec, *key, case)
        assert got == CHANGED_WINNERS.get(name, RECORDED["pairs"][name]), name
        assert got in (RECORDED["errors"][_error_name(key, x)], RECORDED["errors"][_error_name(key, y)]), name
    assert all(RECORDED["pairs"][n] != m for n, m in CHANGED_WINNERS.items())


@pytest.mark.parametrize("family", ("decode", "extend"))
def test_workspace_functions_reject_an_unknown_layout(monkeypatch, recs, family):
    """(They read it as "bhnd" before: the one case that is not in the recording.)"""
    _use(monkeypatch, recs, True)
    with pytest.raises(ValueError, match=re.escape("layout must be one of ['bhnd', 'bnhd']")):
        call(family, "workspace", make(family, "workspace", layout="nbhd"))
    assert RECORDED["errors"]["ragged_workspace/layout"] == "ValueError: layout must be one of ['bhnd', 'bnhd']"


# ---- _lib.KV_PARAMS against the headers and the ctypes tables ----

def _prototypes():
    protos = {}
    inc = os.path.join(os.path.dirname(HERE), "include")
    for fname in sorted(os.listdir(inc)):
        text = open(os.path.join(inc, fname)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        text = re.sub(r"//[^\n]*", "", text)
        for sym, params in re.findall(r"\b(fa_mi355x_\w+)\s*\(([^()]*)\)\s*;", text):
            protos[sym] = [re.findall(r"\w+", p)[-1] for p in params.split(",")] if params.strip() not in ("", "void") else []
    return protos


def test_parameter_table_against_headers_and_abi():
    abi = {**_lib.DECODE_ABI, **_lib.PAGED_ABI, **_lib.RAGGED_ABI, **_lib.WINDOW_ABI, **_lib.SINK_ABI, **_lib.FP8_ABI, **_lib.ROPE_ABI}
    protos = _prototypes()
    synonyms = {"k_pool": "k_cache", "v_pool": "v_cache", "T": "Nq"}
    for sym, names in _lib.KV_PARAMS.items():
        assert [synonyms.get(n, n) for n in protos[sym]] == list(names), sym
        restype, argtypes = abi[sym]
        assert len(argtypes) == len(names), sym
        for n, t in zip(names, argtypes):
            want = ctypes.c_void_p if n in _lib.KV_POINTERS else ctypes.c_float if n == "softmax_scale" else ctypes.c_int
            assert t is want, (sym, n)
    reached = {c.split("(")[0] for t in RECORDED["traces"].values() for c in t if not c.startswith("->")}
    assert reached and reached <= set(_lib.KV_PARAMS), sorted(reached - set(_lib.KV_PARAMS))
