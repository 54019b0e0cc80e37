"""The generation half of modules_transformer on the CPU: what KVCache / PagedKVCache and the attention_stack_* functions send to the C
library, what they return, what state they leave in the cache, which torch operators they run and which arguments they reject with
which message, held against tests/model_call_traces.json.  The file was recorded ONCE, on the commit before the layer was given one
cache core, one keyword source and one advance loop, and the layer has to reproduce it (``python tests/test_model_calls_cpu.py
--record`` rewrites it: not something a refactor does).

Everything runs under the recorder of tests/test_device_ops_cpu.py (CPU tensors, no library, pointers logged by name).  Every case
(cache class x feature x kv heads x head dim) runs one script of public calls; a call that raises is recorded as its exception and
the script goes on.  Per call: the C calls (without the prefix every symbol has), the result, the cache's host and device state
on one line (of the workspace keys, the ones the call added) and the aten operators a TorchDispatchMode saw, with counts
(VIEW_OPS dropped).  C calls, results and state must match string for string.  The operators are compared as
a multiset, and only where torch is the recording's version: a call may LOSE the operators ATEN_LOSSES lists for it and may never
gain one (a gained ``_to_copy`` / ``lift_fresh`` / ``_local_scalar_dense`` would be a new host-to-device copy or synchronisation in
a path that GraphedStep captures)."""
import collections
import itertools
import json
import os
import sys

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]   # (for the --record run: pytest has both on the path already)
from test_device_ops_cpu import _describe, install_recorder  # noqa: E402

from flash_attention_minitorch_amd import modules_transformer as mt  # noqa: E402

TRACES = os.path.join(HERE, "model_call_traces.json")
F32, BF16, F16, FP8 = torch.float32, torch.bfloat16, torch.float16, torch.float8_e4m3fn
B, H, LAYERS, CAP, PAGE, POOL = 2, 4, 2, 512, 128, 7   # (POOL < B * max_pages = 8: the sequences share the pool)
W, S, ROT = 33, 4, 32
P, CHUNKED, CHUNK = 40, 300, 150
SYMBOL_PREFIX = "fa_mi355x_"   # of every symbol of the library: left out of the logged C calls, for the file's size

# the operators that only re-describe memory: dropped from the operator lists (fixed: an operator is never added to hide a gain)
VIEW_OPS = ("aten.view.default", "aten._unsafe_view.default", "aten.reshape.default", "aten.expand.default", "aten.slice.Tensor",
            "aten.select.int", "aten.unsqueeze.default", "aten.squeeze.dim", "aten.permute.default", "aten.transpose.int",
            "aten.t.default", "aten.detach.default", "aten.alias.default", "aten.as_strided.default", "aten.split.Tensor",
            "aten.split_with_sizes.default", "aten.unbind.int")

FEATURES = {"plain": {}, "window": dict(window=W), "window_sink": dict(window=W, sink=S), "fp8": dict(fp8=True), "rope": dict(rope=True)}
PAGED_ONLY = {"rope_window_sink": dict(rope=True, window=W, sink=S)}


class OpLog(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.ops = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if str(func) not in VIEW_OPS:   # logged without "aten." and without the overload name ".default"
            self.ops.append(str(func).removeprefix("aten.").removesuffix(".default"))
        return func(*args, **(kwargs or {}))


def _randn(g, *shape):
    return torch.randn(shape, generator=g).to(BF16)


def cases():
    c = {}
    for paged, hkv, d in itertools.product((False, True), (H, H // 2), (64, 48)):
        for feat, opts in {**FEATURES, **(PAGED_ONLY if paged else {})}.items():
            c[f"{'paged' if paged else 'slab'}/{feat}/hkv{hkv}/d{d}"] = dict(paged=paged, hkv=hkv, d=d, **opts)
    return c


def build(paged, hkv, d, window=None, sink=None, fp8=False, rope=False):
    """(the cache, the layers, the inputs by name, every tensor the recorder names)"""
    E, g = H * d, torch.Generator().manual_seed(7 * d + hkv)
    named = {}
    layers = []
    for li in range(LAYERS):
        w = dict(wq=_randn(g, E, E), wk=_randn(g, E, hkv * d), wv=_randn(g, E, hkv * d), wo=_randn(g, E, E))
        named.update({f"{n}{li}": t for n, t in w.items()})
        layers.append((w["wq"], w["wk"], w["wv"], w["wo"]))
    kw = dict(n_kv_head=hkv, window=window, sink=sink)
    if fp8:
        kw.update(kv_dtype=FP8, kv_scale=(torch.full((LAYERS, hkv), 0.5), torch.full((LAYERS, hkv), 2.0)))
    if rope:
        kw["rope"] = mt.Rotary.table(CAP, ROT)
        named.update(cos=kw["rope"].cos, sin=kw["rope"].sin)
    if paged:
        cache = mt.PagedKVCache(LAYERS, B, CAP, H, d, BF16, "cpu", page_size=PAGE, n_pages=POOL, **kw)
        named["table"] = cache.block_table
    else:
        cache = mt.KVCache(LAYERS, B, CAP, H, d, BF16, "cpu", **kw)
    for li in range(LAYERS):
        named.update({f"k{li}": cache.k[li], f"v{li}": cache.v[li]})
    named["lengths"] = cache.lengths
    if cache.kv_scale is not None:
        named.update(k_scale=cache.kv_scale[0], v_scale=cache.kv_scale[1])
    x = dict(prompt=_randn(g, B, P, E), t1=_randn(g, B, 1, E), t5=_randn(g, B, 5, E), t3=_randn(g, B, 3, E), t150=_randn(g, B, 150, E),
             packed=_randn(g, 50, E), long=_randn(g, B, CHUNKED, E))
    named.update({f"x_{n}": t for n, t in x.items()})
    return cache, layers, x, named


def script(cache, layers, x):
    s = [("prefill", lambda: mt.attention_stack_prefill(x["prompt"], layers, H, cache)),
         ("fused_1", lambda: mt.attention_stack_step_fused(x["t1"], layers, H, cache)),
         ("fused_5", lambda: mt.attention_stack_step_fused(x["t5"], layers, H, cache)),
         ("step_3", lambda: mt.attention_stack_step(x["t3"], layers, H, cache)),
         ("extend_150", lambda: mt.attention_stack_extend(x["t150"], layers, H, cache)),
         ("ragged_7_40", lambda: mt.attention_stack_ragged(x["packed"], [7, 40], layers, H, cache)),
         ("chunked_300", lambda: mt.attention_stack_prefill_chunked(x["long"], layers, H, cache, CHUNK))]
    if cache.window is not None and cache.block_table is not None:   # the restart path: leading pages given back, then a new prompt
        s += [("release_behind_window", lambda: cache.release_behind_window([CHUNKED] * B)),
              ("chunked_300_again", lambda: mt.attention_stack_prefill_chunked(x["long"], layers, H, cache, CHUNK))]
    return s


def _state(cache, seen):
    """The cache after a call, on one line; of the workspace keys the ones this call added (``seen``: the keys before it)."""
    st = dict(lengths=cache.lengths.tolist(), length_bound=cache.length_bound,
              new_workspaces=sorted(repr(k) for k in cache._workspaces if k not in seen))
    if cache.block_table is not None:
        st.update(pages=cache.pages, free=cache.free, released=cache.released, block_table=cache.block_table.tolist())
    seen.update(cache._workspaces)
    return " ".join(f"{n}={v}" for n, v in st.items())


def run_case(rec, opts):
    cache, layers, x, named = build(**opts)
    out, seen = {}, set()
    for name, fn in script(cache, layers, x):
        rec.reset(named)
        log = OpLog()
        try:
            with log:
                r = fn()
            result = "-> " + _describe(rec, r)
        except Exception as e:
            result = f"{type(e).__name__}: {e}"
        counts = collections.Counter(log.ops)
        out[name] = dict(result=result, state=_state(cache, seen), aten=" ".join(f"{op}*{counts[op]}" for op in sorted(counts)),
                         c=[c.removeprefix(SYMBOL_PREFIX) for c in rec.calls])
    return out


# ---- the calls that are refused ----
# constructor faults: name -> (the classes that can have it, keywords; ``d`` and ``dtype`` are positional and set apart)

def _scales(*shape):
    return (torch.ones(shape), torch.ones(shape))


CTOR_FAULTS = {
    "window_zero": ("both", dict(window=0)), "window_bool": ("both", dict(window=True)), "window_type": ("both", dict(window="8")),
    "sink_without_window": ("both", dict(sink=4)), "sink_negative": ("both", dict(window=8, sink=-1)),
    "sink_type": ("both", dict(window=8, sink=2.0)),
    "n_kv_head": ("both", dict(n_kv_head=3)), "n_kv_head_zero": ("both", dict(n_kv_head=0)),
    "fp8_on_fp32": ("both", dict(dtype=F32, kv_dtype=FP8)), "fp8_window": ("both", dict(window=8, kv_dtype=FP8)),
    "fp8_scale_single": ("both", dict(kv_dtype=FP8, kv_scale=(torch.ones(LAYERS, H),))),
    "fp8_scale_shape": ("both", dict(kv_dtype=FP8, kv_scale=_scales(LAYERS, H + 1))),
    "kv_dtype_other": ("both", dict(kv_dtype=F16)), "scale_without_fp8": ("both", dict(kv_scale=_scales(LAYERS, H))),
    "rope_type": ("both", dict(rope="rotary")), "rope_short": ("both", dict(rope=lambda: mt.Rotary.table(CAP - 1, ROT))),
    "rope_wide": ("both", dict(d=48, rope=lambda: mt.Rotary.table(CAP, 64))),
    "page_size_odd": ("paged", dict(page_size=100)), "page_size_zero": ("paged", dict(page_size=0)),
    "capacity_zero": ("paged", dict(capacity=0)), "n_pages_zero": ("paged", dict(n_pages=0)),
}


def construct(paged, d=64, dtype=BF16, capacity=CAP, **kw):
    kw = {n: v() if callable(v) else v for n, v in kw.items()}
    return (mt.PagedKVCache if paged else mt.KVCache)(LAYERS, B, capacity, H, d, dtype, "cpu", **kw)


def _message(fn):
    try:
        fn()
    except Exception as e:
        return f"{type(e).__name__}: {e}"
    return "ok"


def ctor_single_cases():
    return {f"{'paged' if paged else 'slab'}/{n}": (paged, kw) for paged in (False, True) for n, (who, kw) in CTOR_FAULTS.items()
            if paged or who == "both"}


def ctor_pair_cases():
    """Every two constructor faults that fit into one call (they set no keyword to two values)."""
    c = {}
    for paged in (False, True):
        names = [n for n, (who, _) in CTOR_FAULTS.items() if paged or who == "both"]
        for x, y in itertools.combinations(names, 2):
            kx, ky = CTOR_FAULTS[x][1], CTOR_FAULTS[y][1]
            if all(kx[n] is ky[n] or (not callable(kx[n]) and not isinstance(kx[n], tuple) and kx[n] == ky[n]) for n in set(kx) & set(ky)):
                c[f"{'paged' if paged else 'slab'}/{x}+{y}"] = (paged, {**kx, **ky})
    return c


def stack_fault_cases():
    """Single faults of the stack functions: name -> a function that makes the faulty call on a fresh cache."""
    d, E = 64, H * 64
    g = torch.Generator().manual_seed(3)
    w, w_half = _randn(g, E, E), _randn(g, E, E // 2)
    layers, grouped = [(w, w, w, w)] * LAYERS, [(w, w_half, w_half, w)] * LAYERS
    x = lambda *shape: torch.zeros(shape, dtype=BF16)
    slab = lambda **kw: mt.KVCache(LAYERS, B, CAP, H, d, BF16, "cpu", **kw)
    paged = lambda **kw: mt.PagedKVCache(LAYERS, B, CAP, H, d, BF16, "cpu", n_pages=POOL, **kw)

    def full(cache):   # a cache whose host bound leaves room for two more tokens
        cache.length_bound = CAP - 2
        return cache

    c = {}
    for cn, make in (("slab", slab), ("paged", paged)):
        c.update({
            f"{cn}/prefill/over_capacity": lambda make=make: mt.attention_stack_prefill(x(B, CAP + 1, E), layers, H, make()),
            f"{cn}/prefill/kv_heads": lambda make=make: mt.attention_stack_prefill(x(B, P, E), grouped, H, make()),
            f"{cn}/prefill_windowed/over_capacity": lambda make=make: mt.attention_stack_prefill(x(B, CAP + 1, E), layers, H, make(window=W)),
            f"{cn}/step_fused/too_many": lambda make=make: mt.attention_stack_step_fused(x(B, 129, E), layers, H, make()),
            f"{cn}/step_fused/capacity": lambda make=make: mt.attention_stack_step_fused(x(B, 3, E), layers, H, full(make())),
            f"{cn}/step_fused/kv_heads": lambda make=make: mt.attention_stack_step_fused(x(B, 3, E), grouped, H, make()),
            f"{cn}/step/too_many": lambda make=make: mt.attention_stack_step(x(B, 129, E), layers, H, make()),
            f"{cn}/step/capacity": lambda make=make: mt.attention_stack_step(x(B, 3, E), layers, H, full(make())),
            f"{cn}/step/kv_heads": lambda make=make: mt.attention_stack_step(x(B, 3, E), grouped, H, make()),
            f"{cn}/extend/capacity": lambda make=make: mt.attention_stack_extend(x(B, 150, E), layers, H, full(make())),
            f"{cn}/extend/capacity_short": lambda make=make: mt.attention_stack_extend(x(B, 3, E), layers, H, full(make())),
            f"{cn}/extend/kv_heads": lambda make=make: mt.attention_stack_extend(x(B, 150, E), grouped, H, make()),
            f"{cn}/ragged/unpacked": lambda make=make: mt.attention_stack_ragged(x(B, 25, E), [7, 40], layers, H, make()),
            f"{cn}/ragged/counts_length": lambda make=make: mt.attention_stack_ragged(x(50, E), [7], layers, H, make()),
            f"{cn}/ragged/counts_negative": lambda make=make: mt.attention_stack_ragged(x(50, E), [7, -1], layers, H, make()),
            f"{cn}/ragged/counts_sum": lambda make=make: mt.attention_stack_ragged(x(50, E), [11, 40], layers, H, make()),
            f"{cn}/ragged/capacity": lambda make=make: mt.attention_stack_ragged(x(50, E), [3, 1], layers, H, full(make())),
            f"{cn}/ragged/kv_heads": lambda make=make: mt.attention_stack_ragged(x(50, E), [7, 40], grouped, H, make()),
            f"{cn}/ragged/fp8": lambda make=make: mt.attention_stack_ragged(x(50, E), [7, 40], layers, H, make(kv_dtype=FP8)),
            f"{cn}/step/fp8": lambda make=make: mt.attention_stack_step(x(B, 3, E), layers, H, make(kv_dtype=FP8)),
            f"{cn}/chunked/chunk_zero": lambda make=make: mt.attention_stack_prefill_chunked(x(B, P, E), layers, H, make(), 0),
            f"{cn}/chunked/over_capacity": lambda make=make: mt.attention_stack_prefill_chunked(x(B, CAP + 1, E), layers, H, make(), CHUNK),
            f"{cn}/chunked/kv_heads": lambda make=make: mt.attention_stack_prefill_chunked(x(B, CHUNKED, E), grouped, H, make(), CHUNK),
        })
    c["paged/step/paged"] = lambda: mt.attention_stack_step(x(B, 3, E), layers, H, paged())
    c["paged/step_fused/pool_exhausted"] = lambda: mt.attention_stack_step_fused(x(B, 3, E), layers, H, mt.PagedKVCache(
        LAYERS, B, CAP, H, d, BF16, "cpu", n_pages=1))
    c["paged/release_behind_window/no_window"] = lambda: paged().release_behind_window([0, 0])
    c["graphed/T_zero"] = lambda: mt.GraphedStep(layers, H, slab(), T=0)
    c["graphed/T_too_many"] = lambda: mt.GraphedStep(layers, H, slab(), T=129)
    c["graphed/step/T_mismatch"] = lambda: mt.GraphedStep(layers, H, slab(), T=1).step(x(B, 3, E))
    c["graphed/step/capacity"] = lambda: mt.GraphedStep(layers, H, full(slab()), T=3).step(x(B, 3, E))
    return c


def record():
    out = {"torch": torch.__version__, "cases": {}, "ctor_errors": {}, "ctor_pairs": {}, "stack_errors": {}}
    with pytest.MonkeyPatch.context() as mp:
        rec = install_recorder(mp)
        for name, opts in cases().items():
            out["cases"][name] = run_case(rec, opts)
        for name, (paged, kw) in ctor_single_cases().items():
            out["ctor_errors"][name] = _message(lambda: construct(paged, **kw))
        for name, (paged, kw) in ctor_pair_cases().items():
            out["ctor_pairs"][name] = _winner(name, _message(lambda: construct(paged, **kw)), out["ctor_errors"])
        for name, fn in stack_fault_cases().items():
            out["stack_errors"][name] = _message(fn)
    return out


def _winner(name, message, singles):
    """What a two-fault call reported, as the name of the fault (the first of the two) whose own message it is; any other outcome
    as it is."""
    cls, pair = name.split("/")
    return next((n for n in pair.split("+") if singles[f"{cls}/{n}"] == message), message)


def _wrapped(table, width=150):
    lines = [""]
    for k, v in table.items():
        item = f"{json.dumps(k)}: {json.dumps(v)}"
        if lines[-1] and len(lines[-1]) + len(item) + 2 > width:
            lines.append("")
        lines[-1] += (", " if lines[-1] else "") + item
    return "{\n  " + ",\n  ".join(lines) + "\n }"


def write(out, f):
    """The recording as JSON laid out for reading and for its size: one line per C call, one for what a public call left behind
    (result, state, operators), one per refused call, the two-fault table wrapped."""
    cases_ = []
    for name, calls in out["cases"].items():
        body = [f'   {json.dumps(call)}: {json.dumps({k: r[k] for k in ("result", "state", "aten")})[:-1]}, "c": ['
                + ",".join("\n    " + json.dumps(c) for c in r["c"]) + "]}" for call, r in calls.items()]
        cases_.append(f"  {json.dumps(name)}: {{\n" + ",\n".join(body) + "\n  }")
    parts = [f' "torch": {json.dumps(out["torch"])}', ' "cases": {\n' + ",\n".join(cases_) + "\n }",
             ' "ctor_errors": ' + _wrapped(out["ctor_errors"], 0), ' "ctor_pairs": ' + _wrapped(out["ctor_pairs"]),
             ' "stack_errors": ' + _wrapped(out["stack_errors"], 0)]
    f.write("{\n" + ",\n".join(parts) + "\n}\n")


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_model_calls_cpu.py --record"
    with open(TRACES, "w") as f:
        write(record(), f)
    with open(TRACES) as f:
        assert json.load(f)["cases"], "the recording is not JSON"
    sys.exit(0)

with open(TRACES) as f:
    RECORDED = json.load(f)


@pytest.fixture
def rec(monkeypatch):
    return install_recorder(monkeypatch)


def test_the_recording_covers_every_case():
    assert set(RECORDED["cases"]) == set(cases()) and len(cases()) == 4 * (2 * len(FEATURES) + len(PAGED_ONLY))
    for name, calls in RECORDED["cases"].items():
        restart = name.startswith("paged/") and "window" in name
        assert len(calls) == (9 if restart else 7), name
        raised = {n for n, c in calls.items() if not c["result"].startswith("->")}
        want = set()
        if name.startswith("paged/") or "/fp8/" in name:
            want.add("step_3")   # (torch indexing into a slab, which does not quantise)
        if "/fp8/" in name:
            want.add("ragged_7_40")
        assert raised == want, (name, raised)
        if restart:   # the release freed pages, so the second chunked prefill took the restart path
            freed, gone = ("-> 2", "released=[1, 1] ") if "sink" in name else ("-> 4", "released=[2, 2] ")   # (a sink keeps the first page)
            assert calls["release_behind_window"]["result"] == freed and gone in calls["release_behind_window"]["state"], name
            assert "released=[0, 0] " in calls["chunked_300_again"]["state"], name
    assert set(RECORDED["ctor_errors"]) == set(ctor_single_cases()) and "ok" not in RECORDED["ctor_errors"].values()
    assert set(RECORDED["ctor_pairs"]) == set(ctor_pair_cases())
    assert all(winner in name.split("/")[1].split("+") for name, winner in RECORDED["ctor_pairs"].items())   # (one of its two faults)
    assert set(RECORDED["stack_errors"]) == set(stack_fault_cases()) and "ok" not in RECORDED["stack_errors"].values()
    # what the parent logged for a two-layer fused step on the plain slab cache: a size query, then append + attend per layer
    fused = RECORDED["cases"]["slab/plain/hkv4/d64"]["fused_1"]
    assert len(fused["c"]) == 5 and sum(_ops(fused["aten"]).values()) == 18   # (30 operators with the VIEW_OPS counted)


# The operators a call runs no more, by call of the script: (operator, how many, which caches, why).
ATEN_LOSSES = {
    "prefill": [("fill_.Scalar", 1, lambda name: "window" not in name and (name.startswith("paged/") or "/fp8/" in name),
                 "the lengths of a prompt that goes through the library's append were filled before the layers and again after them; "
                 "every prompt's lengths are filled once now, before the layers")],
}


def _ops(text):
    return collections.Counter({op: int(n) for op, n in (item.split("*") for item in text.split())})


def _lost(name, call):
    c = collections.Counter()
    for op, n, applies, _ in ATEN_LOSSES.get(call, ()):
        if applies(name):
            c[op] += n
    return c


@pytest.mark.parametrize("name", sorted(cases()))
def test_model_calls(rec, name):
    """Every public call of the script makes the C calls it made, argument for argument, returns what it returned and leaves the
    cache in the state it left it in; it runs the torch operators it ran, less the listed losses and never one more."""
    got, want = run_case(rec, cases()[name]), RECORDED["cases"][name]
    assert list(got) == list(want)
    same_torch = RECORDED["torch"] == torch.__version__
    for call in want:
        assert got[call]["c"] == want[call]["c"], (name, call)
        assert got[call]["result"] == want[call]["result"], (name, call)
        assert got[call]["state"] == want[call]["state"], (name, call)
        if same_torch:
            now, then = _ops(got[call]["aten"]), _ops(want[call]["aten"])
            assert not now - then, (name, call, "gained", dict(now - then))
            assert then - now == _lost(name, call), (name, call, "lost", dict(then - now))
    if not same_torch:
        pytest.skip(f"the operator lists were recorded under torch {RECORDED['torch']}, this is {torch.__version__}: C calls, results and "
                    "state were compared, the operators were not")


def test_constructor_faults(rec):
    for name, (paged, kw) in ctor_single_cases().items():
        assert _message(lambda: construct(paged, **kw)) == RECORDED["ctor_errors"][name], name


def test_stack_function_faults(rec):
    for name, fn in stack_fault_cases().items():
        assert _message(fn) == RECORDED["stack_errors"][name], name


# Both constructors check in ONE order now (KVCache's docstring): window, sink, n_kv_head, the paging arguments, rope, quantisation.
# Before, KVCache looked at rope FIRST, and PagedKVCache looked at rope BEFORE n_pages.  The two-fault calls that report their other
# fault since: every slab pair of a rope fault with a window, sink or n_kv_head fault, and the paged pairs of a rope fault with
# n_pages = 0.
_ROPE = ("rope_type", "rope_short", "rope_wide")
_BEFORE_ROPE = ("window_zero", "window_bool", "window_type", "sink_without_window", "sink_negative", "sink_type", "n_kv_head", "n_kv_head_zero")


def changed_winners():
    c = {}
    for name in ctor_pair_cases():
        cls, pair = name.split("/")
        x, y = pair.split("+")
        first, rope = (x, y) if y in _ROPE else (y, x)
        if rope in _ROPE and ((cls == "slab" and first in _BEFORE_ROPE) or (cls == "paged" and first == "n_pages_zero")):
            c[name] = first
    return c


def test_two_constructor_faults(rec):
    """A constructor call with two faults reports one of them, in the words of the call that has that fault alone; which one is
    recorded (by the fault's name), and changed_winners() lists the calls where it is the other one now."""
    changed = changed_winners()
    assert len(changed) == 3 * len(_BEFORE_ROPE) + 3 and all(RECORDED["ctor_pairs"][n] != m for n, m in changed.items())
    for name, (paged, kw) in ctor_pair_cases().items():
        got = _winner(name, _message(lambda: construct(paged, **kw)), RECORDED["ctor_errors"])
        assert got == changed.get(name, RECORDED["ctor_pairs"][name]), name
        assert got in name.split("/")[1].split("+"), name


def test_restart_forgets_the_sequences():
    """restart() is what a chunked prefill begins with: lengths and bound to zero; a paged cache also takes back the sequences that
    had released leading pages (they own row 0 again), and only those."""
    slab = mt.KVCache(1, B, CAP, H, 64, F32, "cpu")
    slab.lengths.fill_(9)
    slab.length_bound = 9
    slab.restart()
    assert slab.lengths.tolist() == [0, 0] and slab.length_bound == 0
    paged = mt.PagedKVCache(1, B, CAP, H, 64, F32, "cpu", n_pages=POOL, window=W)
    paged.reserve(CHUNKED)
    assert paged.release_behind_window([CHUNKED, 0]) == 2 and paged.released == [2, 0]
    kept = list(paged.pages[1])
    paged.restart()
    assert paged.released == [0, 0] and paged.pages == [[], kept] and len(paged.free) == POOL - len(kept)
    assert paged.lengths.tolist() == [0, 0] and paged.length_bound == 0
