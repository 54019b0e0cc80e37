"""CPU-side checks of grouped-query (GQA / MQA) heads in the forward and backward path: the C ABI of fa_mi355x_*_gqa (symbols, workspace
size, argument validation, kernel plans; no GPU, no HIP call) and what the Python layer (device_ops.flash_attn_*_gqa, grouped
multi_head_attention / attention_stack_prefill) sends to the library, returns and rejects, with the C library replaced by a recorder
(the pattern of tests/test_device_ops_cpu.py)."""
import ctypes
import itertools
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = torch.float32, torch.bfloat16
GQA_SYMBOLS = ("fa_mi355x_bwd_workspace_bytes_gqa", "fa_mi355x_fwd_gqa", "fa_mi355x_bwd_gqa", "fa_mi355x_plan_gqa",
               "fa_mi355x_scale_guard_gqa")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from flash_attention_minitorch_amd import _lib
    return _lib


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_grouped_entry_points(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flash_attn_mi355x.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fa_mi355x_\w+)\s*\(", text))
    core = built.core()
    for s in GQA_SYMBOLS:
        assert s in declared, s
        assert hasattr(core, s), s
        assert s in built.CORE_ABI, s


def test_workspace_bytes(built):
    ws = built.core().fa_mi355x_bwd_workspace_bytes_gqa
    plain = built.core().fa_mi355x_bwd_workspace_bytes
    for B, H, N, d in ((2, 8, 256, 64), (1, 6, 100, 32), (3, 5, 77, 128)):
        vecs = 3 * B * H * N * 4
        assert plain(B * H, N, d) == vecs
        assert ws(B, H, H, N, d) == vecs                       # Hkv == H: no scratch term
        for Hkv in (h for h in range(1, H) if H % h == 0):
            start = (vecs + 255) // 256 * 256                  # the scratch starts on a 256-byte boundary ...
            assert ws(B, H, Hkv, N, d) == start + 2 * B * H * N * d * 4   # ... and holds two q-shaped fp32 tensors
    assert ws(1, 6, 1, 100, 32) - 2 * 6 * 100 * 32 * 4 == 7424 > 3 * 6 * 100 * 4 == 7200   # (a case where the boundary moves the start)
    for bad in ((2, 8, 0, 256, 64), (2, 8, -2, 256, 64), (2, 6, 4, 256, 64), (2, 8, 3, 256, 64), (0, 8, 2, 256, 64), (2, 8, 2, 0, 64),
                (2, 0, 1, 256, 64)):
        assert ws(*bad) == 0, bad


_FWD_ARGS = dict(q=16, k=16, v=16, out=16, l=16, m=16, B=1, H=8, Hkv=2, N=16, d=64, layout=1, scale=0.0, causal=0, variant=2, dtype=1,
                 opts=None, nopts=0, guard=None, produce=0, stream=None)
_BWD_ARGS = dict(q=16, k=16, v=16, out=16, dout=16, dq=16, dk=16, dv=16, l=16, m=16, ws=256, B=1, H=8, Hkv=2, N=16, d=64, layout=1,
                 scale=0.0, causal=0, variant=2, dtype=1, stages=7, opts=None, nopts=0, guard=None, stream=None)
_BAD = [
    (dict(Hkv=0), 1, "Hkv must be positive and divide H"),
    (dict(Hkv=-1), 1, "Hkv must be positive and divide H"),
    (dict(H=6, Hkv=4), 1, "Hkv must be positive and divide H"),
    (dict(k=None), 1, "null pointer argument"),
    (dict(layout=5), 1, "unknown layout"),
    (dict(layout=-1), 1, "unknown layout"),
    (dict(d=48), 2, "device path supports d in {32, 64, 128}"),
    (dict(H=0), 1, "B and H must be positive"),
    (dict(Hkv=0, k=None), 1, "Hkv must be positive and divide H"),      # the first failing check decides
    (dict(H=6, Hkv=4, layout=5), 1, "Hkv must be positive and divide H"),
    (dict(opts=(93,), nopts=1, Hkv=0), 1, "option value not supported"),
]
_BAD_BWD = [   # the scratch of a grouped backward is read in 16-byte pieces: its workspace must be 256-byte aligned (16 is not)
    (dict(ws=16), 1, "256-byte aligned"),
    (dict(ws=16, layout=5), 1, "unknown layout"),
]


def test_bad_arguments_are_rejected_before_any_hip_call(built):
    """Every call below returns before any HIP call (the fake non-null pointers are never dereferenced; no valid call is made)."""
    core = built.core()
    for name, base in (("fa_mi355x_fwd_gqa", _FWD_ARGS), ("fa_mi355x_bwd_gqa", _BWD_ARGS)):
        for over, rc, msg in _BAD + (_BAD_BWD if "ws" in base else []):
            a = dict(base, **over)
            keep = a["opts"] = (ctypes.c_int * len(a["opts"]))(*a["opts"]) if a["opts"] else None
            got = getattr(core, name)(*a.values())
            err = core.fa_mi355x_last_error().decode()
            assert (got, msg in err) == (rc, True), (name, over, got, err)
            del keep


def _plan(core, fn, *args, opts=()):
    arr = (ctypes.c_int * len(opts))(*opts) if opts else None
    buf = ctypes.create_string_buffer(1024)
    rc = fn(*args, arr, len(opts), buf, 1024)
    return rc, buf.value.decode()


def _plan_grid():
    """tests/golden/make_plan_golden.py: the grid whose answers tests/golden/plan_grid.npz records."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_plan_golden", os.path.join(ROOT, "tests", "golden", "make_plan_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plan_of_an_ungrouped_call_is_the_plan_of_its_batch(built):
    """fa_mi355x_plan_gqa(B, H, H, ...) == fa_mi355x_plan(B * H, ...), return code and text, over every case of the plan grid read by
    heads: H the largest of 8, 4, 2, 1 that divides the batch."""
    core = built.core()
    grid = _plan_grid()
    arrays = {o: (ctypes.c_int * len(o))(*o) if o else None for o in grid.OPTIONS}
    a, b = ctypes.create_string_buffer(1024), ctypes.create_string_buffer(1024)
    plan, plan_gqa = core.fa_mi355x_plan, core.fa_mi355x_plan_gqa
    n = 0
    for dtype, d, N, batch, causal, variant, st, o in grid.cases():
        H = 8 if batch % 8 == 0 else (2 if batch % 2 == 0 else 1)
        a.value = b.value = b""
        want = (plan(batch, N, d, causal, variant, dtype, st, arrays[o], len(o), a, 1024), a.value)
        got = (plan_gqa(batch // H, H, H, N, d, causal, variant, dtype, st, arrays[o], len(o), b, 1024), b.value)
        assert got == want, (dtype, d, N, batch, causal, variant, st, o, got, want)
        n += 1
    assert n == grid.N_CASES


def test_plan_of_a_grouped_call_adds_one_group_sum_behind_the_dkdv_stage(built):
    core = built.core()
    n = onepass = 0
    for dtype, d, N, (B, H, Hkv), causal, st, o in itertools.product(
            (0, 1), (32, 64, 128), (40, 100, 200, 256, 1024, 4096), ((2, 8, 2), (1, 6, 1), (8, 64, 16), (8, 32, 8)), (0, 1),
            (0, 1, 2, 3, 4, 5, 6, 7), ((), (0, 3, 3), (5, 3, 3), (0,) * 8 + (1,))):
        # the ungrouped call that names the same kernels: where that would be the fp32 one-pass backward, what option 4 = 4 selects
        rc0, want = _plan(core, core.fa_mi355x_plan, B * H, N, d, causal, 2, dtype, st, opts=o)
        if "bwd_onepass_f32_kernel" in want:
            onepass += 1
            rc0, want = _plan(core, core.fa_mi355x_plan, B * H, N, d, causal, 2, dtype, st, opts=(tuple(o) + (0,) * 9)[:4] + (4,) + tuple(o[5:]))
        rc, got = _plan(core, core.fa_mi355x_plan_gqa, B, H, Hkv, N, d, causal, 2, dtype, st, opts=o)
        assert rc == rc0 == 0, (rc, rc0, core.fa_mi355x_last_error())
        names, ref = got.split(";"), want.split(";")
        if st & 2:   # a backward that includes dK/dV: exactly one group_sum_kernel, directly behind the stage's launches
            assert names.count("group_sum_kernel") == 1, got
            i = names.index("group_sum_kernel")
            assert names[:i] + names[i + 1:] == ref, (got, want)
            assert i > 0 and names[i - 1].startswith("bwd_dkdv"), got
        else:        # the forward, the preprocess, a dQ-only stage mask: none
            assert "group_sum_kernel" not in names and names == ref, (got, want)
        n += 1
    assert n > 1000 and onepass > 10
    assert built.plan_gqa(2, 8, 2, 256, 64, False, 2, 1, 7) == ["bwd_dq_slot_kernel", "bwd_dkdv_slot_kernel", "group_sum_kernel"]
    assert built.plan_gqa(2, 8, 8, 256, 64, False, 2, 1, 7) == built.plan(16, 256, 64, False, 2, 1, 7)


def test_every_plan_the_gpu_edge_tests_assert(built):
    """tests/test_gpu_gqa_edges.py asserts the kernel plan of each of its cases, so that a policy change cannot move a case off its
    kernel unnoticed; plan_pins() lists every one of them.  Held here against fa_mi355x_plan_gqa of the CPU build, which plans for the
    256 CUs of an MI355X: the table is proved without a GPU.  Below that, the rows the table rests on, spelled out."""
    import test_gpu_gqa_edges as edges
    pins = edges.plan_pins()
    assert len(pins) > 150
    for (B, H, Hkv, N, d, causal, variant, dtype, stages, opts), want in pins:
        got = ";".join(built.plan_gqa(B, H, Hkv, N, d, causal, variant, 1 if dtype == "bf16" else 0, stages, opts or None))
        assert got == want, ((B, H, Hkv, N, d, causal, variant, dtype, stages, opts), got, want)
    guarded = (0,) * 8 + (3,)
    slot = ["bwd_dq_slot_kernel", "bwd_dkdv_slot_kernel", "group_sum_kernel"]
    phased_causal = ["bwd_dq_kernel", "bwd_dq_kernel", "bwd_dkdv_kernel", "group_sum_kernel"]
    # bf16, d = 64, N = 512, causal: batch * (N / 256) >= 128 takes the causal slot builds by default, 32 heads do not
    assert built.plan_gqa(8, 16, 4, 512, 64, True, 2, 1, 7, guarded) == slot
    assert built.plan_gqa(8, 16, 4, 512, 64, True, 2, 1, 0, guarded) == ["fwd_slot_kernel", "fwd_kernel"]
    assert built.plan_gqa(2, 8, 2, 512, 64, True, 2, 1, 7, guarded) == phased_causal
    assert built.plan_gqa(2, 12, 3, 768, 64, True, 2, 1, 7, guarded) == phased_causal
    assert built.plan_gqa(2, 12, 3, 768, 64, False, 2, 1, 7, guarded) == slot
    assert built.plan_gqa(3, 24, 8, 1024, 64, True, 2, 1, 7, (5, 3, 3, 0, 0, 0, 0, 2, 3)) == slot
    # fp32, d = 64: the ungrouped call of these sizes takes the one-pass backward, the grouped one what option 4 = 4 selects
    for B, H, Hkv, N in edges.ONEPASS_SHAPES:
        for causal in (False, True):
            assert built.plan(B * H, N, 64, causal, 2, 0, 7) == ["bwd_prep_kernel", "bwd_onepass_f32_kernel"]
            assert built.plan_gqa(B, H, Hkv, N, 64, causal, 2, 0, 7) == ["bwd_prep_kernel", "bwd_dkdv_kernel", "group_sum_kernel",
                                                                         "bwd_dq_kernel"]
    # a stage mask runs the group sum behind the dK/dV stage alone
    assert built.plan_gqa(2, 8, 2, 600, 64, False, 2, 1, 2) == ["bwd_dkdv_slot_kernel", "group_sum_kernel"]
    assert built.plan_gqa(2, 8, 2, 600, 64, False, 2, 1, 4) == ["bwd_dq_slot_kernel"]
    assert built.plan_gqa(2, 8, 2, 600, 64, False, 2, 1, 1) == ["bwd_prep_kernel"]


# ---- the Python layer, against a recorder ----------------------------------------------------------------------------------------------

from flash_attention_minitorch_amd import _lib, device_ops as dev, modules_transformer as mt   # noqa: E402

GUARD_BYTES = 2048


class Recorder:
    """Stands in for the ctypes handle of the core library: every attribute is a C function that logs (symbol, arguments) and returns
    0, or a size for the *_bytes queries.  Pointers are logged by name: the caller's tensors by their own names, the rest by order of
    first use (new0, new1, ...)."""

    def __init__(self):
        self.calls, self.names, self.alive = [], {}, []

    def reset(self, named):
        self.calls, self.alive = [], []
        self.names = {t.data_ptr(): n for n, t in named.items() if isinstance(t, torch.Tensor)}

    def name(self, ptr):
        if not ptr:
            return "null"
        if ptr not in self.names:
            self.names[ptr] = f"new{sum(n.startswith('new') for n in self.names.values())}"
        return self.names[ptr]

    def arg(self, a):
        if a is None:
            return "null"
        if isinstance(a, ctypes.c_void_p):
            return self.name(a.value)
        if isinstance(a, int) and a >= 1 << 32:
            return self.name(a)
        if isinstance(a, ctypes.Array):
            return "[" + ",".join(str(x) for x in a) + "]"
        if isinstance(a, float):
            return repr(a)
        return str(int(a))

    def __getattr__(self, sym):
        def fn(*args):
            self.calls.append(f"{sym}({','.join(self.arg(a) for a in args)})")
            if sym == "fa_mi355x_guard_bytes":
                return GUARD_BYTES
            if sym == "fa_mi355x_bwd_workspace_bytes_ex":
                return 12 * args[0] * args[1]
            if sym == "fa_mi355x_bwd_workspace_bytes_gqa":
                B, H, Hkv, N, d = args
                return 12 * B * H * N if Hkv == H else (12 * B * H * N + 255) // 256 * 256 + 8 * B * H * N * d
            return 0
        return fn


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    data_ptr = torch.Tensor.data_ptr

    def kept_data_ptr(t):   # every tensor whose address is taken lives until the next reset: no address is reused
        r.alive.append(t)
        return data_ptr(t)
    monkeypatch.setattr(torch.Tensor, "data_ptr", kept_data_ptr)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: not getattr(self, "on_cpu", False)))
    monkeypatch.setattr(dev, "_stream_ptr", lambda: ctypes.c_void_p(0))
    monkeypatch.setattr(_lib, "core", lambda: r)
    monkeypatch.setattr(_lib, "decode", lambda: r)
    monkeypatch.setattr(_lib, "guard_elems", lambda: GUARD_BYTES // 4, raising=False)
    return r


def _t(*shape, dtype=F32):
    return torch.randn(shape, generator=torch.Generator().manual_seed(len(shape) + shape[-1])).to(dtype)


B, N, H, HKV, D = 2, 16, 6, 2, 64
WS = (12 * B * H * N + 255) // 256 * 256 + 8 * B * H * N * D


def _tensors(layout="bnhd", dtype=BF16, d=D):
    qs, ks = ((B, N, H, d), (B, N, HKV, d)) if layout == "bnhd" else ((B, H, N, d), (B, HKV, N, d))
    return dict(q=_t(*qs, dtype=dtype), k=_t(*ks, dtype=dtype), v=_t(*ks, dtype=dtype), do=_t(*qs, dtype=dtype), o=_t(*qs),
                l=_t(B, H, N))


def test_forward_call(rec):
    a = _tensors()
    rec.reset(a)
    out, l, m = dev.flash_attn_fwd_gqa(a["q"], a["k"], a["v"], causal=True)
    assert rec.calls == ["fa_mi355x_guard_bytes()",
                         f"fa_mi355x_fwd_gqa(q,k,v,new0,new1,null,{B},{H},{HKV},{N},{D},1,0.0,1,2,1,null,0,new2,1,null)"]
    assert out.shape == a["q"].shape and out.dtype is F32 and l.shape == (B, H, N) and m is None
    # [B][H][N][d], FA-1 statistics, a caller's scale, options, out buffer and no guard; fp32 asks for no guard at all
    a = _tensors("bhnd", F32)
    rec.reset(a)
    out, l, m = dev.flash_attn_fwd_gqa(a["q"], a["k"], a["v"], variant=_lib.FA_VARIANT_FA1, softmax_scale=0.25, layout="bhnd",
                                       opts=(0, 2), out=a["o"])
    assert rec.calls == [f"fa_mi355x_fwd_gqa(q,k,v,o,new0,new1,{B},{H},{HKV},{N},{D},0,0.25,0,1,0,[0,2],2,null,0,null)"]
    assert out is a["o"] and m.shape == (B, H, N)
    g = torch.empty(GUARD_BYTES // 4)
    a = dict(_tensors(), g=g)
    rec.reset(a)
    dev.flash_attn_fwd_gqa(a["q"], a["k"], a["v"], guard=g)
    assert rec.calls == [f"fa_mi355x_fwd_gqa(q,k,v,new0,new1,null,{B},{H},{HKV},{N},{D},1,0.0,0,2,1,null,0,g,0,null)"]


def test_backward_call(rec):
    a = _tensors()
    rec.reset(a)
    dq, dk, dv = dev.flash_attn_bwd_gqa(a["q"], a["k"], a["v"], a["o"], a["do"], a["l"], causal=True)
    assert rec.calls == [
        f"fa_mi355x_bwd_workspace_bytes_gqa({B},{H},{HKV},{N},{D})",
        f"fa_mi355x_scale_guard_gqa(q,k,{B * N * H},{B * N * HKV},{D},1,new0,null)",
        f"fa_mi355x_bwd_gqa(q,k,v,o,do,new1,new2,new3,l,null,new4,{B},{H},{HKV},{N},{D},1,0.0,1,2,1,7,null,0,new0,null)"]
    assert dq.shape == a["q"].shape and dk.shape == a["k"].shape and dv.shape == a["v"].shape
    assert dq.dtype is dk.dtype is dv.dtype is F32
    assert rec.alive and any(t.numel() * 4 >= WS for t in rec.alive)   # the workspace it allocated holds the scratch
    # a caller's workspace, gradient buffers and guard, [B][H][N][d], fp32
    a = _tensors("bhnd", F32)
    ws = torch.empty(WS // 4 + 64)
    ws = ws[(-ws.data_ptr() % 256) // 4:][:WS // 4]
    a.update(ws=ws, gq=torch.empty_like(a["q"]), gk=torch.empty_like(a["k"]), gv=torch.empty_like(a["v"]))
    rec.reset(a)
    dq, dk, dv = dev.flash_attn_bwd_gqa(a["q"], a["k"], a["v"], a["o"], a["do"], a["l"], layout="bhnd", guard=None, workspace=ws,
                                        grads=(a["gq"], a["gk"], a["gv"]), opts=(0, 0, 0, 0, 4))
    assert rec.calls == [
        f"fa_mi355x_bwd_workspace_bytes_gqa({B},{H},{HKV},{N},{D})",
        f"fa_mi355x_bwd_gqa(q,k,v,o,do,gq,gk,gv,l,null,ws,{B},{H},{HKV},{N},{D},0,0.0,0,2,0,7,[0,0,0,0,4],5,null,null)"]
    assert dk is a["gk"] and dv is a["gv"]
    w = dev.bwd_workspace_gqa(a["q"], a["k"], "bhnd")
    assert w.numel() * 4 == WS and w.dtype is F32


def test_autograd_call(rec):
    a = _tensors()
    q, k, v = (a[n].clone().requires_grad_() for n in "qkv")
    a.update(q=q, k=k, v=v)
    rec.reset(a)
    o = dev.flash_attn_gqa(q, k, v, causal=True)
    o.sum().backward()
    assert rec.calls == [
        "fa_mi355x_guard_bytes()",
        f"fa_mi355x_fwd_gqa(q,k,v,new0,new1,null,{B},{H},{HKV},{N},{D},1,0.0,1,2,1,null,0,new2,1,null)",
        f"fa_mi355x_bwd_workspace_bytes_gqa({B},{H},{HKV},{N},{D})",
        # the backward reads the guard the forward filled and the unexpanded k and v
        f"fa_mi355x_bwd_gqa(q,k,v,new0,new3,new4,new5,new6,new1,null,new7,{B},{H},{HKV},{N},{D},1,0.0,1,2,1,7,null,0,new2,null)"]
    assert o.shape == q.shape and o.dtype is F32
    assert q.grad.shape == q.shape and k.grad.shape == k.shape and v.grad.shape == v.shape
    assert q.grad.dtype is k.grad.dtype is v.grad.dtype is BF16


def _layers(E, d, hkv, dtype):
    return _t(E, E, dtype=dtype), _t(E, hkv * d, dtype=dtype), _t(E, hkv * d, dtype=dtype), _t(E, E, dtype=dtype)


def test_grouped_multi_head_attention_calls_the_grouped_operator(rec):
    E, heads, hkv = 256, 4, 2
    d = E // heads
    x = _t(B, N, E, dtype=BF16).requires_grad_()
    wq, wk, wv, wo = _layers(E, d, hkv, BF16)
    wk.requires_grad_()
    rec.reset({})
    y = mt.multi_head_attention(x, wq, wk, wv, wo, heads)
    y.sum().backward()
    syms = [c.split("(")[0] for c in rec.calls]
    assert syms == ["fa_mi355x_guard_bytes", "fa_mi355x_fwd_gqa", "fa_mi355x_bwd_workspace_bytes_gqa", "fa_mi355x_bwd_gqa"]
    assert f",{B},{heads},{hkv},{N},{d},1,0.0,1,2,1," in rec.calls[1] and f",{B},{heads},{hkv},{N},{d},1,0.0,1,2,1,7," in rec.calls[3]
    assert y.shape == (B, N, E) and wk.grad.shape == wk.shape
    # the folded scale: softmax_scale = ln 2, no guard
    rec.reset({})
    mt.multi_head_attention(x, wq, wk, wv, wo, heads, fold_scale=True)
    assert [c.split("(")[0] for c in rec.calls] == ["fa_mi355x_fwd_gqa"] and f",1,{mt.LN2!r},1,2,1,null,0,null,0,null)" in rec.calls[0]
    # the unfused layout keeps the reference's data flow: k and v expanded in front of the ungrouped operator
    rec.reset({})
    mt.multi_head_attention(x, wq, wk, wv, wo, heads, fused_layout=False)
    assert [c.split("(")[0] for c in rec.calls] == ["fa_mi355x_guard_bytes", "fa_mi355x_fwd_guarded"]
    # an ungrouped stack makes the calls it made before
    rec.reset({})
    mt.multi_head_attention(x, wq, _t(E, E, dtype=BF16), _t(E, E, dtype=BF16), wo, heads)
    assert [c.split("(")[0] for c in rec.calls] == ["fa_mi355x_guard_bytes", "fa_mi355x_fwd_guarded"]


@pytest.mark.parametrize("d", [64, 48])
def test_grouped_prefill_hands_the_cache_shaped_k_and_v_to_the_grouped_forward(rec, d):
    heads, hkv, P, cap = 4, 2, 16, 32
    E = heads * d
    dp = dev.padded_head_dim(d)
    x = _t(B, P, E, dtype=BF16)
    layers = [_layers(E, d, hkv, BF16)] * 2
    cache = mt.KVCache(2, B, cap, heads, d, BF16, x.device, n_kv_head=hkv)
    rec.reset({})
    y = mt.attention_stack_prefill(x, layers, heads, cache)
    scale = "0.0" if d == dp else repr(float(d ** -0.5))
    fwd = [c for c in rec.calls if c.startswith("fa_mi355x_fwd")]
    assert len(fwd) == 2 and all(c.startswith("fa_mi355x_fwd_gqa(") and f",{B},{heads},{hkv},{P},{dp},1,{scale},1,2,1," in c for c in fwd)
    assert y.shape == (B, P, E) and cache.k[0].shape == (B, cap, hkv, dp) and cache.length_bound == P
    # ungrouped: flash_attn_fwd_bnhd, as before
    cache = mt.KVCache(1, B, cap, heads, d, BF16, x.device)
    rec.reset({})
    mt.attention_stack_prefill(x, [_layers(E, d, heads, BF16)], heads, cache)
    assert [c.split("(")[0] for c in rec.calls if c.startswith("fa_mi355x_fwd")] == ["fa_mi355x_fwd_guarded"]


def _cpu(t):
    t = t.clone()
    t.on_cpu = True
    return t


_REJECTED = {
    "layout": (lambda a: dict(a, layout="nbhd"), "layout must be one of ['bhnd', 'bnhd']"),
    "rank": (lambda a: dict(a, q=a["q"][0]), "expected 4-d tensors"),
    "batch": (lambda a: dict(a, k=_t(B + 1, N, HKV, D, dtype=BF16), v=_t(B + 1, N, HKV, D, dtype=BF16)), "q and k disagree on (B, N, d)"),
    "length": (lambda a: dict(a, k=_t(B, N + 1, HKV, D, dtype=BF16), v=_t(B, N + 1, HKV, D, dtype=BF16)), "q and k disagree on (B, N, d)"),
    "head_dim": (lambda a: dict(a, k=_t(B, N, HKV, 32, dtype=BF16), v=_t(B, N, HKV, 32, dtype=BF16)), "q and k disagree on (B, N, d)"),
    "dtype": (lambda a: dict(a, k=a["k"].float()), "q, k, v must be GPU tensors of one dtype on one device"),
    "device": (lambda a: dict(a, v=_cpu(a["v"])), "q, k, v must be GPU tensors of one dtype on one device"),
    "v_shape": (lambda a: dict(a, v=_t(B, N, 1, D, dtype=BF16)), "k and v must have one shape"),
    "contiguous": (lambda a: dict(a, k=a["k"].transpose(1, 2).contiguous().transpose(1, 2)), "tensors must be contiguous"),
    "group": (lambda a: dict(a, k=_t(B, N, 4, D, dtype=BF16), v=_t(B, N, 4, D, dtype=BF16)), "q's 6 heads must be a multiple of k's 4"),
    "native_d": (lambda a: {n: (t[..., :48].contiguous() if n in "qkvdo" else t) for n, t in a.items()}, "need a native head dim (32, 64, 128)"),
}


@pytest.mark.parametrize("name", sorted(_REJECTED))
def test_rejected_arguments(rec, name):
    change, msg = _REJECTED[name]
    a = change(_tensors())
    layout = a.pop("layout", "bnhd")
    calls = [lambda: dev.flash_attn_fwd_gqa(a["q"], a["k"], a["v"], layout=layout),
             lambda: dev.flash_attn_bwd_gqa(a["q"], a["k"], a["v"], a["o"], a["do"], a["l"], layout=layout),
             lambda: dev.flash_attn_gqa(a["q"], a["k"], a["v"], layout=layout)]
    if name not in ("device", "v_shape"):   # (bwd_workspace_gqa takes q and k alone)
        calls.append(lambda: dev.bwd_workspace_gqa(a["q"], a["k"], layout))
    for call in calls:
        rec.reset(a)
        with pytest.raises(ValueError) as e:
            call()
        assert msg in str(e.value), (name, str(e.value))
        assert rec.calls == []   # rejected before any C call


def test_rejected_backward_buffers(rec):
    a = _tensors()
    bad = [(dict(out=a["o"].to(BF16)), "out must be the forward's contiguous float32 output"),
           (dict(out_grad=a["do"][:, :8].contiguous()), "out_grad must share q's shape, dtype and device"),
           (dict(workspace=torch.empty(16)), "workspace too small"),
           (dict(grads=(a["o"], a["o"], torch.empty(4))), "each of grads must be a contiguous float32 tensor"),
           (dict(l=torch.empty(5)), "l must be a contiguous float32 tensor")]
    for over, msg in bad:
        kw = dict(out=a["o"], out_grad=a["do"], l=a["l"])
        kw.update(over)
        rec.reset(a)
        with pytest.raises(ValueError) as e:
            dev.flash_attn_bwd_gqa(a["q"], a["k"], a["v"], **kw)
        assert msg in str(e.value), str(e.value)
        assert not any(c.startswith("fa_mi355x_bwd_gqa") for c in rec.calls)
    # the ungrouped entry points keep their own checks: a k of another shape is still rejected there
    with pytest.raises(ValueError) as e:
        dev.flash_attn_fwd_bnhd(a["q"], a["k"], a["v"])
    assert "one shape and dtype" in str(e.value)
