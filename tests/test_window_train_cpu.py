"""Sliding-window / attention-sink training calls (include/flash_attn_mi355x_window.h, libflash_attn_mi355x_window.so), the checks
that need no GPU: the fp64 reference the GPU tests compare against, the C ABI against _lib.WINDOW_TRAIN_ABI, every argument error
before any HIP call, the Python checks, the calls device_ops and the model functions make (under the recorder of
tests/test_device_ops_cpu.py), and the new library's kernels (no scratch) beside an unchanged core library."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
from test_abi_cpu import ROOT, _device_kernels, built  # noqa: F401  (built: the module-scoped build fixture)

HEADER = "flash_attn_mi355x_window.h"
SYMBOLS = ["fa_mi355x_fwd_window", "fa_mi355x_bwd_window", "fa_mi355x_bwd_window_workspace_bytes", "fa_mi355x_window_last_error"]


# ---- the fp64 reference: a dense masked softmax and its analytic backward ----

def admitted(N, W, S):
    """(N, N) bool: row i admits key j iff j <= i and (j > i - W or j < S)."""
    i, j = np.arange(N)[:, None], np.arange(N)[None, :]
    return (j <= i) & ((j > i - W) | (j < S))


def window_train_reference(q, k, v, do, W, S, scale=None):
    """q, do (B, H, N, d); k, v (B, Hkv, N, d), H a multiple of Hkv (query head h reads kv head h // G).  Returns fp64
    out (B, H, N, d), lse (B, H, N), dq (B, H, N, d), dk, dv (B, Hkv, N, d): the group's gradients summed."""
    q, k, v, do = (np.asarray(a, dtype=np.float64) for a in (q, k, v, do))
    B, H, N, d = q.shape
    Hkv = k.shape[1]
    G = H // Hkv
    ke, ve = np.repeat(k, G, axis=1), np.repeat(v, G, axis=1)
    tau = 1.0 / np.sqrt(d) if scale is None else scale
    s = np.where(admitted(N, W, S), tau * (q @ ke.swapaxes(-1, -2)), -np.inf)
    mx = s.max(axis=-1, keepdims=True)
    e = np.exp(s - mx)
    l = e.sum(axis=-1, keepdims=True)
    p = e / l
    out = p @ ve
    dp = do @ ve.swapaxes(-1, -2)
    ds = p * (dp - (do * out).sum(axis=-1, keepdims=True))
    dq = tau * (ds @ ke)
    dk = (tau * (ds.swapaxes(-1, -2) @ q)).reshape(B, Hkv, G, N, d).sum(axis=2)
    dv = (p.swapaxes(-1, -2) @ do).reshape(B, Hkv, G, N, d).sum(axis=2)
    return out, (mx + np.log(l))[..., 0], dq, dk, dv


def test_reference_with_a_window_over_everything_is_the_causal_oracle():
    rng = np.random.default_rng(7)
    B, H, N, d = 2, 3, 37, 16
    q, k, v, do = (rng.uniform(-1, 1, (B, H, N, d)) for _ in range(4))
    ro, rL, _, _ = oracle.dense_attention_fw(q, k, v, causal=True)
    rdq, rdk, rdv = oracle.dense_attention_bw(q, k, v, do, causal=True)
    for W, S in ((N, 0), (N + 5, 0), (3, N), (1000, 1000)):
        got = window_train_reference(q, k, v, do, W, S)
        for g, r in zip(got, (ro, rL, rdq, rdk, rdv)):
            assert np.max(np.abs(g - r)) < 1e-12, (W, S)


def test_reference_mask_and_group_sum_by_hand():
    assert admitted(6, 2, 1).astype(int).tolist() == [[1, 0, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0], [1, 1, 1, 0, 0, 0], [1, 0, 1, 1, 0, 0],
                                                      [1, 0, 0, 1, 1, 0], [1, 0, 0, 0, 1, 1]]
    rng = np.random.default_rng(3)
    B, H, Hkv, N, d, W, S = 1, 4, 2, 9, 8, 3, 1
    q, do = (rng.uniform(-1, 1, (B, H, N, d)) for _ in range(2))
    k, v = (rng.uniform(-1, 1, (B, Hkv, N, d)) for _ in range(2))
    out, lse, dq, dk, dv = window_train_reference(q, k, v, do, W, S)
    # row 5 of head 3 admits keys 0, 3, 4, 5 of kv head 1
    keys = [0, 3, 4, 5]
    s = (k[0, 1, keys] @ q[0, 3, 5]) / np.sqrt(d)
    p = np.exp(s - s.max())
    assert np.allclose(out[0, 3, 5], p @ v[0, 1, keys] / p.sum(), atol=1e-13) and np.isclose(lse[0, 3, 5], s.max() + np.log(p.sum()))
    # the grouped call is the expanded call with the group's dk, dv added
    eo, el, edq, edk, edv = window_train_reference(q, np.repeat(k, 2, 1), np.repeat(v, 2, 1), do, W, S)
    assert np.array_equal(out, eo) and np.array_equal(dq, edq)
    assert np.allclose(dk, edk.reshape(B, Hkv, 2, N, d).sum(2), atol=1e-14) and np.allclose(dv, edv.reshape(B, Hkv, 2, N, d).sum(2), atol=1e-14)


# ---- the C ABI ----

def test_header_declares_what_the_abi_table_binds_and_the_library_exports(built):
    from test_lib_cpu import _ctypes_kind, _prototypes
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(fa_mi355x_\w+)\s*\(", text))) == sorted(SYMBOLS) == sorted(built.WINDOW_TRAIN_ABI)
    core_text = open(os.path.join(ROOT, "include", "flash_attn_mi355x.h")).read()
    assert HEADER not in core_text and "fa_mi355x_fwd_window" not in core_text   # (the core library exports what ITS header declares)
    protos = _prototypes(HEADER)
    lib = built.window()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        res, args = built.WINDOW_TRAIN_ABI[s]
        ret, kinds = protos[s]
        assert [_ctypes_kind(a) for a in args] == kinds and _ctypes_kind(res) == ret, s
        assert getattr(lib, s).argtypes == args and getattr(lib, s).restype is res, s
    needed = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "-d", built.lib_path(built.WINDOW_NAME)], capture_output=True,
                            text=True, check=True).stdout
    assert "libflash_attn_mi355x" not in needed   # a library of its own: it loads without the other two


_ONE = 16   # a fake non-null device pointer: a launch would fail, so any code but the expected one shows a HIP call
_GOOD = dict(q=_ONE, k=_ONE, v=_ONE, out=_ONE, dout=_ONE, dq=_ONE, dk=_ONE, dv=_ONE, lse=_ONE, ws=256, B=2, H=4, Hkv=2, N=100, d=64,
             layout=1, scale=0.0, window=8, sink=2, dtype=1)


def _call(lib, bwd, **over):
    a = dict(_GOOD, **over)
    p = lambda n: ctypes.c_void_p(a[n]) if a[n] else None
    tail = (a["B"], a["H"], a["Hkv"], a["N"], a["d"], a["layout"], a["scale"], a["window"], a["sink"], a["dtype"], None)
    if bwd:
        rc = lib.fa_mi355x_bwd_window(p("q"), p("k"), p("v"), p("out"), p("dout"), p("dq"), p("dk"), p("dv"), p("lse"), p("ws"), *tail)
    else:
        rc = lib.fa_mi355x_fwd_window(p("q"), p("k"), p("v"), p("out"), p("lse"), *tail)
    return rc, lib.fa_mi355x_window_last_error().decode()


_BAD = [
    (dict(window=0), "window must be at least 1"), (dict(window=-3), "window must be at least 1"),
    (dict(sink=-1), "sink must not be negative"),
    (dict(H=4, Hkv=3), "Hkv must be positive and divide H"), (dict(Hkv=0), "Hkv must be positive and divide H"),
    (dict(d=80), "d must be 32, 64 or 128"), (dict(d=256), "d must be 32, 64 or 128"),
    (dict(B=0), "must be positive"), (dict(N=0), "must be positive"), (dict(H=0), "must be positive"), (dict(d=0), "must be positive"),
    (dict(dtype=2), "unknown dtype"), (dict(layout=2), "unknown layout"),
    (dict(scale=-1.0), "softmax_scale"), (dict(scale=float("nan")), "softmax_scale"), (dict(scale=float("inf")), "softmax_scale"),
    (dict(N=1 << 22, d=128), "under 2 GiB"), (dict(N=1 << 20, H=16, Hkv=16, d=128, layout=1), "under 2 GiB"),
] + [(dict({n: 0}), "null pointer argument") for n in ("q", "k", "v", "out", "lse")]
_BAD_BWD = [(dict({n: 0}), "null pointer argument") for n in ("dout", "dq", "dk", "dv", "ws")] + [(dict(ws=128), "256-byte aligned")]


@pytest.mark.parametrize("bwd,over,msg", [(b, o, m) for b in (False, True) for o, m in _BAD] + [(True, o, m) for o, m in _BAD_BWD],
                         ids=lambda x: "-".join(f"{k}={v}" for k, v in x.items()) if isinstance(x, dict) else None)
def test_each_bad_argument_is_rejected_before_any_hip_call(built, bwd, over, msg):
    """The window library alone (it does not link the core library, see above), no GPU: FA_ERR_BAD_ARG = 1 and the message; the fake
    pointers would make any launch fail with FA_ERR_HIP = 3."""
    rc, err = _call(built.window(), bwd, **over)
    assert rc == 1 and msg in err, (rc, err)


def test_workspace_bytes(built):
    f = built.window().fa_mi355x_bwd_window_workspace_bytes
    assert f(2, 4, 4, 100, 64) == 3 * 2 * 4 * 100 * 4
    vecs = 3 * 2 * 8 * 100 * 4
    assert f(2, 8, 2, 100, 64) == (vecs + 255) // 256 * 256 + 2 * 2 * 8 * 100 * 64 * 4
    assert f(2, 8, 2, 100, 64) == built.core().fa_mi355x_bwd_workspace_bytes_gqa(2, 8, 2, 100, 64)
    assert f(0, 8, 2, 100, 64) == f(2, 8, 3, 100, 64) == f(2, 8, 2, 0, 64) == 0


# ---- the kernels ----

def test_every_kernel_of_the_window_library_has_no_scratch_and_the_core_library_keeps_its_kernels(built):
    kernels = _device_kernels(built.lib_path(built.WINDOW_NAME))
    names = [k[0] for k in kernels]
    for stem in ("win_fwd_kernel", "win_dq_kernel", "win_dkdv_kernel", "bwd_prep_kernel"):
        assert sum(stem in n for n in names) == 6, (stem, names)   # bf16 and fp32 at d = 32, 64, 128
    assert sum("group_sum_kernel" in n for n in names) == 1
    for name, scratch, vgpr in kernels:
        assert scratch == 0, (name, scratch)
        assert vgpr <= 512, (name, vgpr)
    core = _device_kernels(built.lib_path(built.CORE_NAME))
    assert len(core) == 97 and not [k for k in core if "win_" in k[0]]   # profiles/rope_isa_identity.txt: 97 before this library


# ---- Python: the checks, and the calls under the recorder ----

@pytest.fixture
def rec(monkeypatch):
    from flash_attention_minitorch_amd import _lib
    from test_device_ops_cpu import install_recorder
    r = install_recorder(monkeypatch)
    log = r.fa_mi355x_bwd_window_workspace_bytes
    r.__dict__["fa_mi355x_bwd_window_workspace_bytes"] = lambda *a: log(*a) or 4096   # (logged like the others, with a size)
    monkeypatch.setattr(_lib, "window", lambda: r)
    return r


def _qkv(B=2, N=200, H=4, Hkv=2, d=64, layout="bnhd", dtype=None):
    import torch
    g = torch.Generator().manual_seed(N)
    shape = (lambda h: (B, N, h, d)) if layout == "bnhd" else (lambda h: (B, h, N, d))
    return [torch.randn(shape(h), generator=g).to(dtype or torch.bfloat16) for h in (H, Hkv, Hkv)]


def test_python_checks_raise_before_any_launch(rec):
    from flash_attention_minitorch_amd import device_ops as dev
    q, k, v = _qkv()
    for kw, msg in ((dict(window=-1), "negative"), (dict(window=1.5), "int"), (dict(window=True), "int"), (dict(window=8, sink=-2), "negative"),
                    (dict(sink=2), "needs window"), (dict(window=8, sink="a"), "int")):
        with pytest.raises(ValueError, match=msg):
            dev.flash_attn_gqa(q, k, v, causal=True, **kw)
    with pytest.raises(ValueError, match="causal"):
        dev.flash_attn_gqa(q, k, v, causal=False, window=8)
    with pytest.raises(ValueError, match="window >= 1"):
        dev.flash_attn_fwd_window(q, k, v, 0)
    with pytest.raises(ValueError, match="window >= 1"):
        dev.flash_attn_fwd_window(q, k, v, None)
    with pytest.raises(ValueError, match="native head dim"):
        dev.flash_attn_fwd_window(*_qkv(d=80), 8)
    with pytest.raises(ValueError, match="multiple"):
        dev.flash_attn_fwd_window(*_qkv(H=4, Hkv=3), 8)
    o, lse = q.float(), q.float()[..., 0].transpose(1, 2).contiguous()
    with pytest.raises(ValueError, match="out_grad"):
        dev.flash_attn_bwd_window(q, k, v, o, k, lse, 8)
    with pytest.raises(ValueError, match="workspace too small"):
        dev.flash_attn_bwd_window(q, k, v, o, q, lse, 8, workspace=o.new_empty(16))
    assert not [c for c in rec.calls if c.startswith(("fa_mi355x_fwd", "fa_mi355x_bwd_window(", "fa_mi355x_bwd_gqa"))], rec.calls


def _names(rec):
    return [c.split("(")[0] for c in rec.calls if "bytes" not in c]


@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
def test_flash_attn_gqa_with_a_window_calls_the_window_library_forward_and_backward(rec, layout):
    from flash_attention_minitorch_amd import device_ops as dev
    B, N, H, Hkv, d, W, S = 2, 200, 4, 2, 64, 48, 3
    q, k, v = (t.requires_grad_() for t in _qkv(B, N, H, Hkv, d, layout))
    rec.reset(dict(q=q, k=k, v=v))
    o = dev.flash_attn_gqa(q, k, v, causal=True, layout=layout, window=W, sink=S)
    lay = 1 if layout == "bnhd" else 0
    assert rec.calls == [f"fa_mi355x_fwd_window(q,k,v,new0,new1,{B},{H},{Hkv},{N},{d},{lay},0.0,{W},{S},1,null)"], rec.calls
    assert o.shape == q.shape and o.dtype.is_floating_point and o.element_size() == 4
    o.sum().backward()
    assert rec.calls[1] == f"fa_mi355x_bwd_window_workspace_bytes({B},{H},{Hkv},{N},{d})"
    assert re.fullmatch(rf"fa_mi355x_bwd_window\(q,k,v,new0,new\d,new\d,new\d,new\d,new1,new\d,{B},{H},{Hkv},{N},{d},{lay},0.0,{W},{S},1,null\)",
                        rec.calls[2]), rec.calls
    assert len(rec.calls) == 3
    assert q.grad.shape == q.shape and k.grad.shape == k.shape and v.grad.dtype == v.dtype
    # no sink: S = 0; a softmax_scale reaches the library
    rec.reset(dict(q=q, k=k, v=v))
    dev.flash_attn_gqa(q, k, v, True, 0.25, layout, window=W)
    assert rec.calls[0].endswith(f",{lay},0.25,{W},0,1,null)")


def test_no_window_and_windows_over_the_whole_sequence_make_the_calls_they_made_before(rec):
    from flash_attention_minitorch_amd import device_ops as dev
    N = 200

    def trace(**kw):
        q, k, v = (t.requires_grad_() for t in _qkv(N=N))
        rec.reset(dict(q=q, k=k, v=v))
        dev.flash_attn_gqa(q, k, v, causal=True, **kw).sum().backward()
        return list(rec.calls)
    before = trace()
    assert _names(rec) == ["fa_mi355x_fwd_gqa", "fa_mi355x_bwd_gqa"]
    for kw in (dict(window=None), dict(window=0), dict(window=N), dict(window=N + 1), dict(window=5, sink=N), dict(window=0, sink=0),
               dict(window=None, sink=None)):
        assert trace(**kw) == before, kw
    assert _names(rec) == ["fa_mi355x_fwd_gqa", "fa_mi355x_bwd_gqa"]
    trace(window=N - 1)
    assert _names(rec) == ["fa_mi355x_fwd_window", "fa_mi355x_bwd_window"]
    trace(window=5, sink=N - 1)
    assert _names(rec) == ["fa_mi355x_fwd_window", "fa_mi355x_bwd_window"]


@pytest.mark.parametrize("Hkv", [4, 2])
@pytest.mark.parametrize("fused", [True, False])
def test_attention_stack_passes_window_and_sink_to_every_layer(rec, monkeypatch, fused, Hkv):
    import torch
    from flash_attention_minitorch_amd import device_ops as dev, modules_transformer as mt
    B, N, H, d, W, S, L = 2, 200, 4, 64, 48, 3, 3
    g = torch.Generator().manual_seed(1)
    x = torch.randn((B, N, H * d), generator=g).to(torch.bfloat16)
    wq, wk = (torch.randn(s, generator=g).to(torch.bfloat16) / 16 for s in ((H * d, H * d), (H * d, Hkv * d)))
    layers = [(wq, wk, wk, wq)] * L
    rope = mt.Rotary(*(torch.zeros(N, d // 2) for _ in range(2)))
    order = []
    monkeypatch.setattr(mt.Rotary, "apply", lambda self, t, off=None: order.append("rope") or t)
    fwd = dev.flash_attn_fwd_window
    monkeypatch.setattr(dev, "flash_attn_fwd_window", lambda *a, **kw: order.append("attn") or fwd(*a, **kw))
    rec.reset({})
    xg = x.clone().requires_grad_()
    mt.attention_stack(xg, layers, H, fused_layout=fused, rope=rope, window=W, sink=S).sum().backward()
    hk, lay = (Hkv, 1) if fused else (H, 0)   # (the unfused layer expands k and v and permutes to (B, H, N, d))
    fw = [c for c in rec.calls if c.startswith("fa_mi355x_fwd_window(")]
    bw = [c for c in rec.calls if c.startswith("fa_mi355x_bwd_window(")]
    assert len(fw) == len(bw) == L and _names(rec) == ["fa_mi355x_fwd_window"] * L + ["fa_mi355x_bwd_window"] * L, rec.calls
    assert all(c.endswith(f",{B},{H},{hk},{N},{d},{lay},0.0,{W},{S},1,null)") for c in fw + bw), rec.calls
    assert order == ["rope", "rope", "attn"] * L   # the rotation comes first
    assert xg.grad is not None
    # without a window, or with one over the whole sequence: the calls of the stack as it was
    for kw in (dict(), dict(window=N, sink=S), dict(window=0)):
        rec.reset({})
        mt.attention_stack(x, layers, H, fused_layout=fused, rope=rope, **kw)
        assert not [n for n in _names(rec) if "window" in n] and len(_names(rec)) >= L, rec.calls
    with pytest.raises(ValueError, match="causal"):
        mt.attention_stack(x, layers, H, causal=False, window=W)
