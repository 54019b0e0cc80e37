"""Logit soft-capping in the training forward and backward (include/flash_attn_mi355x_window_softcap.h, exported by
libflash_attn_mi355x_window.so), the checks that need no GPU: the fp64 reference the GPU tests compare against, pinned three ways;
the header against _lib.WINDOW_TRAIN_SOFTCAP_ABI and the library's exports; every bad cap and every inherited bad argument before
any HIP call; the cap builds of the three kernels (no scratch) beside unchanged uncapped builds and an unchanged packed library;
and the calls device_ops and the model functions make, under the recorder of tests/test_device_ops_cpu.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from test_abi_cpu import ROOT, _device_kernels, built  # noqa: F401  (built: the module-scoped build fixture)
from test_window_train_cpu import _BAD, _BAD_BWD, _GOOD, _names, _qkv, admitted, rec, window_train_reference  # noqa: F401

HEADER = "flash_attn_mi355x_window_softcap.h"
SYMBOLS = ["fa_mi355x_fwd_window_softcap", "fa_mi355x_bwd_window_softcap"]


# ---- the fp64 reference: the dense masked softmax of the capped scores and its analytic backward ----

def softcap_train_reference(q, k, v, do, W, S, scale=None, softcap=0.0, chain=True):
    """window_train_reference with every score capped BEFORE the mask: z = softcap * tanh(tau * q.k / softcap), P the softmax of z
    over the admitted keys, lse = ln sum exp z; dZ = P * (dP - delta), dS = dZ * (1 - tanh^2) * tau.  softcap = 0: no cap.
    ``chain=False`` leaves the 1 - tanh^2 factor out (what a backward that forgot the cap would return).  Shapes as there."""
    q, k, v, do = (np.asarray(a, dtype=np.float64) for a in (q, k, v, do))
    B, H, N, d = q.shape
    Hkv = k.shape[1]
    G = H // Hkv
    ke, ve = np.repeat(k, G, axis=1), np.repeat(v, G, axis=1)
    tau = 1.0 / np.sqrt(d) if scale is None else scale
    raw = tau * (q @ ke.swapaxes(-1, -2))
    if softcap:
        th = np.tanh(raw / softcap)
        z, slope = softcap * th, 1.0 - th * th
    else:
        z, slope = raw, 1.0
    s = np.where(admitted(N, W, S), z, -np.inf)
    mx = s.max(axis=-1, keepdims=True)
    e = np.exp(s - mx)
    l = e.sum(axis=-1, keepdims=True)
    p = e / l
    out = p @ ve
    dp = do @ ve.swapaxes(-1, -2)
    ds = p * (dp - (do * out).sum(axis=-1, keepdims=True))
    if chain:
        ds = ds * slope
    dq = tau * (ds @ ke)
    dk = (tau * (ds.swapaxes(-1, -2) @ q)).reshape(B, Hkv, G, N, d).sum(axis=2)
    dv = (p.swapaxes(-1, -2) @ do).reshape(B, Hkv, G, N, d).sum(axis=2)
    return out, (mx + np.log(l))[..., 0], dq, dk, dv


def _small(seed=3, B=2, H=4, Hkv=2, N=23, d=8, amp=1.0):
    rng = np.random.default_rng(seed)
    q, do = (rng.uniform(-amp, amp, (B, H, N, d)) for _ in range(2))
    k, v = (rng.uniform(-amp, amp, (B, Hkv, N, d)) for _ in range(2))
    return q, k, v, do


def test_reference_without_a_cap_is_the_window_reference_and_a_huge_cap_changes_nothing():
    q, k, v, do = _small(amp=3.0)
    for W, S, scale in ((5, 2, None), (23, 0, 0.3), (1, 0, None)):
        want = window_train_reference(q, k, v, do, W, S, scale)
        for g, w in zip(softcap_train_reference(q, k, v, do, W, S, scale, 0.0), want):
            assert np.array_equal(g, w), (W, S)
        for g, w in zip(softcap_train_reference(q, k, v, do, W, S, scale, 1e6), want):
            assert np.max(np.abs(g - w)) < 1e-9, (W, S)
        # and a real cap is another function, forward and backward, whose backward needs the chain rule
        capped = softcap_train_reference(q, k, v, do, W, S, scale, 0.5)
        if W > 1:
            assert all(np.max(np.abs(g - w)) > 1e-3 for g, w in zip(capped, want))
            loose = softcap_train_reference(q, k, v, do, W, S, scale, 0.5, chain=False)
            assert np.max(np.abs(loose[2] - capped[2])) > 1e-3 and np.max(np.abs(loose[3] - capped[3])) > 1e-3
            assert all(np.array_equal(a, b) for a, b in zip(loose[:2] + loose[4:], capped[:2] + capped[4:]))


def test_reference_gradients_are_torch_autograd_in_float64():
    import torch
    B, H, Hkv, N, d, W, S, C, scale = 2, 4, 2, 23, 8, 6, 2, 0.7, 0.4
    q, k, v, do = _small(seed=5, amp=2.0)
    tq, tk, tv = (torch.from_numpy(a).requires_grad_() for a in (q, k, v))
    G = H // Hkv
    s = scale * (tq @ tk.repeat_interleave(G, 1).transpose(-1, -2))
    z = C * torch.tanh(s / C)
    z = z.masked_fill(~torch.from_numpy(admitted(N, W, S)), float("-inf"))
    o = torch.softmax(z, dim=-1) @ tv.repeat_interleave(G, 1)
    lse = torch.logsumexp(z, dim=-1)
    o.backward(torch.from_numpy(do))
    got = softcap_train_reference(q, k, v, do, W, S, scale, C)
    for g, w in zip(got, (o, lse, tq.grad, tk.grad, tv.grad)):
        assert g.shape == tuple(w.shape) and np.max(np.abs(g - w.detach().numpy())) < 1e-12


def test_reference_lse_is_bounded_by_the_cap_and_the_admitted_keys():
    q, k, v, do = _small(seed=9, amp=30.0)   # saturated: most scores sit at +-softcap
    N = q.shape[2]
    for W, S, C in ((5, 2, 0.5), (N, 0, 3.0), (1, 0, 0.25)):
        lse = softcap_train_reference(q, k, v, do, W, S, None, C)[1]
        bound = C + np.log(admitted(N, W, S).sum(axis=1))
        assert np.all(np.abs(lse) <= bound + 1e-12), (W, S, C)


# ---- the C ABI ----

def test_header_declares_what_the_table_binds_and_the_window_library_exports(built):
    from test_lib_cpu import _ctypes_kind, _prototypes
    raw = open(os.path.join(ROOT, "include", HEADER)).read()
    assert "varlen" not in raw and "bidir" not in raw   # (the packed libraries' headers alone hold those words)
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert sorted(set(re.findall(r"\b(fa_mi355x_\w+)\s*\(", text))) == sorted(SYMBOLS) == sorted(built.WINDOW_TRAIN_SOFTCAP_ABI)
    assert '#include "flash_attn_mi355x_window.h"' in text
    assert not set(SYMBOLS) & set(built.WINDOW_TRAIN_ABI)   # a table of its own: the window header's set stays what it was
    protos, base = _prototypes(HEADER), _prototypes("flash_attn_mi355x_window.h")
    lib = built.window()
    exported = subprocess.run(["nm", "-D", "--defined-only", built.lib_path(built.WINDOW_NAME)], capture_output=True, text=True,
                              check=True).stdout
    assert sorted(re.findall(r" T (fa_mi355x_\w+)\n", exported)) == sorted(list(built.WINDOW_TRAIN_ABI) + SYMBOLS)
    for s in SYMBOLS:
        res, args = built.WINDOW_TRAIN_SOFTCAP_ABI[s]
        ret, kinds = protos[s]
        assert [_ctypes_kind(a) for a in args] == kinds and _ctypes_kind(res) == ret, s
        assert getattr(lib, s).argtypes == args and getattr(lib, s).restype is res, s
        # the _window prototype with one float directly behind `int window`
        bret, bkinds = base[s[:-len("_softcap")]]
        at = len(bkinds) - 4   # ..., window | sink, dtype, stream
        assert ret == bret and kinds == bkinds[:at + 1] + [_ctypes_kind(ctypes.c_float)] + bkinds[at + 1:], s
    decl = re.sub(r"\s+", " ", text)
    assert decl.count("int window, float softcap, int sink, int dtype, void* stream)") == 2
    for s in built.WINDOW_TRAIN_ABI:   # window() binds both tables
        assert getattr(lib, s).argtypes == built.WINDOW_TRAIN_ABI[s][1], s


def _call(lib, bwd, **over):
    a = {**_GOOD, "softcap": 0.25, **over}
    p = lambda n: ctypes.c_void_p(a[n]) if a[n] else None
    tail = (a["B"], a["H"], a["Hkv"], a["N"], a["d"], a["layout"], a["scale"], a["window"], a["softcap"], a["sink"], a["dtype"], None)
    if bwd:
        rc = lib.fa_mi355x_bwd_window_softcap(p("q"), p("k"), p("v"), p("out"), p("dout"), p("dq"), p("dk"), p("dv"), p("lse"), p("ws"),
                                              *tail)
    else:
        rc = lib.fa_mi355x_fwd_window_softcap(p("q"), p("k"), p("v"), p("out"), p("lse"), *tail)
    return rc, lib.fa_mi355x_window_last_error().decode()


_BAD_CAP = [(dict(softcap=c), "softcap must be finite and not negative") for c in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf"))]


@pytest.mark.parametrize("bwd,over,msg", [(b, o, m) for b in (False, True) for o, m in _BAD_CAP + _BAD] + [(True, o, m) for o, m in _BAD_BWD],
                         ids=lambda x: "-".join(f"{k}={v}" for k, v in x.items()) if isinstance(x, dict) else None)
def test_each_bad_cap_and_each_inherited_bad_argument_is_rejected_before_any_hip_call(built, bwd, over, msg):
    """No GPU: FA_ERR_BAD_ARG = 1 and the message; the fake pointers would make any launch fail with FA_ERR_HIP = 3.  The inherited
    faults are reported beside a good cap, and beside softcap = 0 (the _window call) as well."""
    rc, err = _call(built.window(), bwd, **over)
    assert rc == 1 and msg in err, (rc, err)
    if "softcap" not in over:
        rc, err = _call(built.window(), bwd, softcap=0.0, **over)
        assert rc == 1 and msg in err, (rc, err)


# ---- the kernels ----

def test_six_cap_builds_of_each_kernel_without_scratch_beside_the_kernels_that_were_there(built):
    kernels = _device_kernels(built.lib_path(built.WINDOW_NAME))
    names = [k[0] for k in kernels]
    for stem in ("win_fwd_softcap_kernel", "win_dq_softcap_kernel", "win_dkdv_softcap_kernel"):
        assert sum(stem in n for n in names) == 6, (stem, names)   # bf16 and fp32 at d = 32, 64, 128
    for stem in ("win_fwd_kernel", "win_dq_kernel", "win_dkdv_kernel", "bwd_prep_kernel"):
        assert sum(stem in n for n in names) == 6, (stem, names)
    assert sum("group_sum_kernel" in n for n in names) == 1 and len(names) == 26 + 18   # 26 before the cap builds
    for name, scratch, vgpr in kernels:
        assert scratch == 0 and vgpr <= 512, (name, scratch, vgpr)
    packed = [k[0] for k in _device_kernels(built.lib_path(built.VARLEN_NAME))]
    assert not [n for n in packed if "softcap" in n]   # fa_varlen.h includes fa_window.h as text: it gains no kernel
    for stem in ("varlen_fwd_kernel", "varlen_dq_kernel", "varlen_dkdv_kernel"):
        assert sum(stem in n for n in packed) == 6, (stem, packed)
    assert len(packed) == 36   # profiles/softcap_train_isa_identity.txt: 36 before this change, instruction for instruction


# ---- Python: the checks, and the calls under the recorder ----

def _trace(rec, N=200, **kw):
    from flash_attention_minitorch_amd import device_ops as dev
    q, k, v = (t.requires_grad_() for t in _qkv(N=N))
    rec.reset(dict(q=q, k=k, v=v))
    dev.flash_attn_gqa(q, k, v, causal=True, **kw).sum().backward()
    return list(rec.calls)


def test_no_cap_and_a_cap_of_zero_make_the_calls_made_today(rec):
    from flash_attention_minitorch_amd import device_ops as dev
    N = 200
    plain, windowed = _trace(rec), _trace(rec, window=48, sink=3)
    assert [c.split("(")[0] for c in windowed if "bytes" not in c] == ["fa_mi355x_fwd_window", "fa_mi355x_bwd_window"]
    for cap in (None, 0, 0.0):
        assert _trace(rec, softcap=cap) == plain and _trace(rec, window=48, sink=3, softcap=cap) == windowed, cap
        assert _trace(rec, window=N, softcap=cap) == plain
    q, k, v = _qkv(N=N)
    o, lse = q.float(), q.float()[..., 0].transpose(1, 2).contiguous()
    for cap in (None, 0):
        rec.reset(dict(q=q, k=k, v=v))
        dev.flash_attn_fwd_window(q, k, v, 48, 3, softcap=cap)
        dev.flash_attn_bwd_window(q, k, v, o, q, lse, 48, 3, softcap=cap)
        assert _names(rec) == ["fa_mi355x_fwd_window", "fa_mi355x_bwd_window"]
        assert rec.calls[0].endswith(",2,4,2,200,64,1,0.0,48,3,1,null)") and rec.calls[-1].endswith(",2,4,2,200,64,1,0.0,48,3,1,null)")


@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
def test_a_cap_routes_forward_and_backward_to_the_softcap_symbols(rec, layout):
    from flash_attention_minitorch_amd import device_ops as dev
    B, N, H, Hkv, d, C = 2, 200, 4, 2, 64, 30.0
    lay = 1 if layout == "bnhd" else 0
    for kw, W, S in ((dict(), N, 0), (dict(window=48), 48, 0), (dict(window=48, sink=3), 48, 3), (dict(window=N + 7), N + 7, 0),
                     (dict(window=0, sink=0), N, 0)):
        q, k, v = (t.requires_grad_() for t in _qkv(B, N, H, Hkv, d, layout))
        rec.reset(dict(q=q, k=k, v=v))
        o = dev.flash_attn_gqa(q, k, v, causal=True, layout=layout, softcap=C, **kw)
        tail = f"{B},{H},{Hkv},{N},{d},{lay},0.0,{W},{C!r},{S},1,null)"
        assert rec.calls == [f"fa_mi355x_fwd_window_softcap(q,k,v,new0,new1,{tail}"], (kw, rec.calls)
        o.sum().backward()
        assert rec.calls[1] == f"fa_mi355x_bwd_window_workspace_bytes({B},{H},{Hkv},{N},{d})"
        assert re.fullmatch(r"fa_mi355x_bwd_window_softcap\(q,k,v,new0,new\d,new\d,new\d,new\d,new1,new\d," + re.escape(tail), rec.calls[2]), rec.calls
        assert len(rec.calls) == 3 and q.grad.shape == q.shape and k.grad.shape == k.shape
    # a caller's scale and an int cap reach the library (the cap as a float)
    rec.reset({})
    dev.flash_attn_gqa(*_qkv(B, N, H, Hkv, d, layout), True, 0.25, layout, softcap=50)
    assert rec.calls[0].endswith(f",{lay},0.25,{N},50.0,0,1,null)")


def test_python_checks_raise_before_any_launch(rec):
    from flash_attention_minitorch_amd import device_ops as dev, modules_transformer as mt
    q, k, v = _qkv()
    with pytest.raises(ValueError, match=r"softcap= with causal=False"):
        dev.flash_attn_gqa(q, k, v, causal=False, softcap=30.0)
    for bad in (-1.0, float("nan"), float("inf"), "30", True):
        with pytest.raises(ValueError, match="softcap must be"):
            dev.flash_attn_gqa(q, k, v, causal=True, softcap=bad)
        with pytest.raises(ValueError, match="softcap must be"):
            dev.flash_attn_fwd_window(q, k, v, 8, softcap=bad)
        with pytest.raises(ValueError, match="softcap must be"):
            dev.flash_attn_bwd_window(q, k, v, q.float(), q, q.float()[..., 0].transpose(1, 2).contiguous(), 8, softcap=bad)
    with pytest.raises(ValueError, match="needs window"):
        dev.flash_attn_gqa(q, k, v, causal=True, sink=2, softcap=30.0)
    with pytest.raises(ValueError, match="window >= 1"):
        dev.flash_attn_fwd_window(q, k, v, 0, softcap=30.0)
    import torch
    x = torch.zeros(2, 200, 256, dtype=torch.bfloat16)
    w = torch.zeros(256, 256, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match=r"softcap= with causal=False"):
        mt.attention_stack(x, [(w, w, w, w)], 4, causal=False, softcap=30.0)
    assert not [c for c in rec.calls if c.startswith(("fa_mi355x_fwd", "fa_mi355x_bwd_window(", "fa_mi355x_bwd_window_softcap"))], rec.calls


@pytest.mark.parametrize("Hkv", [4, 2])
@pytest.mark.parametrize("fused,fold", [(True, False), (True, True), (False, False)])
def test_attention_stack_hands_the_cap_to_every_layer(rec, monkeypatch, fused, fold, Hkv):
    import torch
    from flash_attention_minitorch_amd import modules_transformer as mt
    B, N, H, d, W, S, L, C = 2, 200, 4, 64, 48, 3, 3, 30.0
    g = torch.Generator().manual_seed(1)
    x = torch.randn((B, N, H * d), generator=g).to(torch.bfloat16)
    wq, wk = (torch.randn(s, generator=g).to(torch.bfloat16) / 16 for s in ((H * d, H * d), (H * d, Hkv * d)))
    layers = [(wq, wk, wk, wq)] * L
    rope = mt.Rotary(*(torch.zeros(N, d // 2) for _ in range(2)))
    monkeypatch.setattr(mt.Rotary, "apply", lambda self, t, off=None: t)
    hk, lay = (Hkv, 1) if fused else (H, 0)   # (the unfused layer expands k and v and permutes to (B, H, N, d))
    scale = repr(mt.LN2) if fold else "0.0"
    for kw, Wc, Sc in ((dict(window=W, sink=S), W, S), (dict(), N, 0)):
        rec.reset({})
        xg = x.clone().requires_grad_()
        mt.attention_stack(xg, layers, H, fused_layout=fused, fold_scale=fold, rope=rope, softcap=C, **kw).sum().backward()
        assert _names(rec) == ["fa_mi355x_fwd_window_softcap"] * L + ["fa_mi355x_bwd_window_softcap"] * L, rec.calls
        calls = [c for c in rec.calls if "bytes" not in c]
        want = f",{B},{H},{hk},{N},{d},{lay},{scale},{Wc},{C!r},{Sc},1,null)"
        assert all(c.endswith(want) for c in calls), (want, rec.calls)
        assert xg.grad is not None
    # no cap, or a cap of 0: the calls of the stack as it was
    rec.reset({})
    mt.attention_stack(x, layers, H, fused_layout=fused, rope=rope, window=W, sink=S)
    before = list(rec.calls)
    rec.reset({})
    mt.attention_stack(x, layers, H, fused_layout=fused, rope=rope, window=W, sink=S, softcap=0)
    strip = lambda calls: [re.sub(r"new\d+", "new", c) for c in calls]
    assert strip(rec.calls) == strip(before) and not [n for n in _names(rec) if "softcap" in n]

