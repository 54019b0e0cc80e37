"""Causal packed attention with separate cu_seqlens for q and k (include/flash_attn_mi355x_prefix.h, libflash_attn_mi355x_prefix.so),
the checks that need no GPU: the C ABI against _lib.PREFIX_ABI, every argument error of tests/test_bidir_cpu.py's lists before any
HIP call, the workspace formula, the library's kernels (no scratch, names of their own), the Python checks, the calls device_ops and
the model functions make under the recorder of tests/test_device_ops_cpu.py, and the gather index of the model layer against a
NumPy model."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from test_abi_cpu import ROOT, _device_kernels, built  # noqa: F401  (built: the module-scoped build fixture)
from test_bidir_cpu import _BAD, _BAD_BWD, _GOOD, QBLOCK, _align, _cu, _qkv, key_block
from test_varlen_cpu import pack, seq_rows

HEADER = "flash_attn_mi355x_prefix.h"
SYMBOLS = ["fa_mi355x_fwd_prefix", "fa_mi355x_bwd_prefix", "fa_mi355x_fwd_prefix_workspace_bytes", "fa_mi355x_bwd_prefix_workspace_bytes",
           "fa_mi355x_prefix_last_error"]


# ---- the C ABI ----

def test_header_declares_what_the_abi_table_binds_and_the_library_exports(built):
    from test_lib_cpu import _ctypes_kind, _prototypes
    raw = open(os.path.join(ROOT, "include", HEADER)).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert sorted(set(re.findall(r"\b(fa_mi355x_\w+)\s*\(", text))) == sorted(SYMBOLS) == sorted(built.PREFIX_ABI)
    assert "varlen" not in raw and "bidir" not in raw   # (the other libraries' tests hold every other header to that)
    for other in os.listdir(os.path.join(ROOT, "include")):   # no other header gained a declaration
        if other != HEADER:
            assert "_prefix" not in open(os.path.join(ROOT, "include", other)).read(), other
    for said in ("0 <= j <= i + D", "bottom-right", "admit no key", "Not in this library", "windows, sinks or a logit cap", "fp8",
                 "host-pointer reference ABI", "MFMA-slot"):
        assert said in raw, said
    protos = _prototypes(HEADER)
    lib = built.prefix()
    exported = subprocess.run(["nm", "-D", "--defined-only", built.lib_path(built.PREFIX_NAME)], capture_output=True, text=True, check=True).stdout
    assert sorted(re.findall(r" T (fa_mi355x_\w+)\n", exported)) == sorted(SYMBOLS)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        res, args = built.PREFIX_ABI[s]
        ret, kinds = protos[s]
        assert [_ctypes_kind(a) for a in args] == kinds and _ctypes_kind(res) == ret, s
        assert getattr(lib, s).argtypes == args and getattr(lib, s).restype is res, s
        twin = s.replace("prefix", "bidir")   # argument for argument the two-array bidirectional prototypes
        assert built.BIDIR_ABI[twin] == built.PREFIX_ABI[s] and _prototypes("flash_attn_mi355x_bidir.h")[twin] == protos[s], s
    needed = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "-d", built.lib_path(built.PREFIX_NAME)], capture_output=True,
                            text=True, check=True).stdout
    assert "libflash_attn_mi355x" not in needed   # a library of its own: it loads without the other five


def _call(lib, bwd, **over):
    a = dict(_GOOD, **over)
    p = lambda n: ctypes.c_void_p(a[n]) if a[n] else None
    tail = (p("cu_q"), p("cu_k"), p("ws"), a["nseq"], a["Tq"], a["Tk"], a["H"], a["Hkv"], a["d"], a["scale"], a["dtype"], None)
    if bwd:
        rc = lib.fa_mi355x_bwd_prefix(p("q"), p("k"), p("v"), p("out"), p("dout"), p("dq"), p("dk"), p("dv"), p("lse"), *tail)
    else:
        rc = lib.fa_mi355x_fwd_prefix(p("q"), p("k"), p("v"), p("out"), p("lse"), *tail)
    return rc, lib.fa_mi355x_prefix_last_error().decode()


@pytest.mark.parametrize("bwd,over,msg", [(b, o, m) for b in (False, True) for o, m in _BAD] + [(True, o, m) for o, m in _BAD_BWD],
                         ids=lambda x: "-".join(f"{k}={v}" for k, v in x.items()) if isinstance(x, dict) else None)
def test_each_bad_argument_is_rejected_before_any_hip_call(built, bwd, over, msg):
    """The prefix library alone, no GPU: FA_ERR_BAD_ARG = 1 and the bidirectional library's message; the fake pointers would make any
    launch fail with FA_ERR_HIP = 3.  A call that passes the checks must not be made here."""
    rc, err = _call(built.prefix(), bwd, **over)
    assert rc == 1 and msg in err, (rc, err)


def test_workspace_bytes_are_the_headers_formula(built):
    fwd, bwd = built.prefix().fa_mi355x_fwd_prefix_workspace_bytes, built.prefix().fa_mi355x_bwd_prefix_workspace_bytes
    for nseq, Tq, Tk, H, Hkv, d in ((1, 1, 1, 1, 1, 32), (7, 612, 622, 4, 4, 64), (7, 612, 622, 4, 2, 64), (40, 552, 1080, 4, 1, 128),
                                    (1, 300, 700, 4, 2, 32), (8, 2048, 65536, 32, 8, 128), (256, 32768, 32768, 32, 32, 128)):
        mq, mk = (_align(32 * (T // QBLOCK + nseq)) for T in (Tq, Tk))
        assert fwd(nseq, Tq, Tk, H, Hkv, d) == mq
        vecs = 3 * H * Tq * 4
        assert bwd(nseq, Tq, Tk, H, Hkv, d) == (mq + mk + vecs if Hkv == H else mq + mk + _align(vecs) + 2 * H * Tk * d * 4)
        assert bwd(nseq, Tq, Tk, H, Hkv, d) >= fwd(nseq, Tq, Tk, H, Hkv, d)
        for dt, dd in ((True, 32), (True, 64), (True, 128), (False, 64)):   # every build's key-block map fits the MAP(Tk) it is given
            assert 32 * (Tk // key_block(dt, dd) + nseq) <= mk
    for f in (fwd, bwd):
        assert (f(0, 100, 100, 4, 2, 64) == f(2, 0, 100, 4, 2, 64) == f(2, 100, 0, 4, 2, 64) == f(2, 100, 100, 0, 2, 64)
                == f(2, 100, 100, 4, 3, 64) == f(2, 100, 100, 4, 0, 64) == f(2, 100, 100, 4, 2, 0) == 0)
        assert f(-1, 100, 100, 4, 2, 64) == f(2, -5, 100, 4, 2, 64) == f(2, 100, -5, 4, 2, 64) == 0


# ---- the kernels ----

def test_every_kernel_of_the_prefix_library_has_no_scratch_and_a_name_of_its_own(built):
    kernels = _device_kernels(built.lib_path(built.PREFIX_NAME))
    names = [k[0] for k in kernels]
    for stem in ("prefix_fwd_kernel", "prefix_dq_kernel", "prefix_dkdv_kernel", "bwd_prep_kernel"):
        assert sum(stem in n for n in names) == 6, (stem, names)   # bf16 and fp32 at d = 32, 64, 128
    assert sum("bidir_schedule_kernel" in n for n in names) == 1 and sum("group_sum_kernel" in n for n in names) == 1
    # no kernel of another library: what is left is mfma_peak_kernel, which comes along with fa_aux.h and is not launched
    stems = ("prefix_fwd_kernel", "prefix_dq_kernel", "prefix_dkdv_kernel", "bidir_schedule_kernel", "bwd_prep_kernel", "group_sum_kernel")
    assert [n for n in names if not any(s in n for s in stems)] == [n for n in names if "mfma_peak_kernel" in n]
    assert not [n for n in names if "bidir_fwd" in n or "bidir_dq" in n or "bidir_dkdv" in n or "win_" in n or "varlen_" in n]
    assert len(names) == 27, names
    for name, scratch, vgpr in kernels:
        assert scratch == 0, (name, scratch)
        assert vgpr <= 512, (name, vgpr)


# ---- Python: the checks, and the calls under the recorder ----

@pytest.fixture
def rec(monkeypatch):
    from flash_attention_minitorch_amd import _lib
    from test_device_ops_cpu import install_recorder
    r = install_recorder(monkeypatch)
    for sym in ("fa_mi355x_fwd_prefix_workspace_bytes", "fa_mi355x_bwd_prefix_workspace_bytes"):
        log = getattr(r, sym)
        r.__dict__[sym] = lambda *a, log=log: log(*a) or 4096   # (logged like the others, with a size)
    monkeypatch.setattr(_lib, "prefix", lambda: r)
    return r


def test_python_checks_raise_before_any_launch(rec):
    import torch
    from flash_attention_minitorch_amd import device_ops as dev
    q, k, v = _qkv()
    cq, ck = _cu(0, 100, 300), _cu(0, 150, 200)
    with pytest.raises(ValueError, match="native head dim.*flash_attn_varlen_prefix pads"):
        dev.flash_attn_varlen_prefix_fwd(*_qkv(d=80), cq, ck)
    with pytest.raises(ValueError, match="multiple"):
        dev.flash_attn_varlen_prefix_fwd(*_qkv(H=4, Hkv=3), cq, ck)
    with pytest.raises(ValueError, match="3-d"):
        dev.flash_attn_varlen_prefix_fwd(q[None], k[None], v[None], cq, ck)
    with pytest.raises(ValueError, match="disagree on the head dim"):
        dev.flash_attn_varlen_prefix_fwd(q, k[..., :32].contiguous(), v[..., :32].contiguous(), cq, ck)
    with pytest.raises(ValueError, match="one shape"):
        dev.flash_attn_varlen_prefix_fwd(q, k, v[:, :1].contiguous(), cq, ck)
    with pytest.raises(ValueError, match="one dtype"):
        dev.flash_attn_varlen_prefix_fwd(q, k.float(), v.float(), cq, ck)
    with pytest.raises(TypeError):
        dev.flash_attn_varlen_prefix_fwd(q.half(), k.half(), v.half(), cq, ck)
    with pytest.raises(ValueError, match="contiguous"):
        dev.flash_attn_varlen_prefix_fwd(q.transpose(0, 1).contiguous().transpose(0, 1), k, v, cq, ck)
    with pytest.raises(ValueError, match="self-attention: k must have q's 300 rows"):
        dev.flash_attn_varlen_prefix_fwd(q, k, v, cq)
    with pytest.raises(ValueError, match="self-attention"):
        dev.flash_attn_varlen_prefix(q, k, v, cq)
    with pytest.raises(ValueError, match="one length"):
        dev.flash_attn_varlen_prefix_fwd(q, k, v, cq, _cu(0, 50, 150, 200))
    for bad in (cq.long(), cq[:1], cq[None], [0, 100, 300]):
        with pytest.raises(ValueError, match="cu_seqlens"):
            dev.flash_attn_varlen_prefix_fwd(q, k, v, bad, ck)
        with pytest.raises(ValueError, match="cu_seqlens"):
            dev.flash_attn_varlen_prefix_fwd(q, k, v, cq, bad)
    o, lse = q.float(), q.float()[..., 0].transpose(0, 1).contiguous()
    with pytest.raises(ValueError, match="out_grad"):
        dev.flash_attn_varlen_prefix_bwd(q, k, v, o, k, lse, cq, ck)
    with pytest.raises(ValueError, match="lse"):
        dev.flash_attn_varlen_prefix_bwd(q, k, v, o, q, lse[:, :10], cq, ck)
    with pytest.raises(ValueError, match=r"workspace too small.*prefix_workspace\("):
        dev.flash_attn_varlen_prefix_bwd(q, k, v, o, q, lse, cq, ck, workspace=o.new_empty(16))
    with pytest.raises(ValueError, match="workspace too small"):
        dev.flash_attn_varlen_prefix_fwd(q, k, v, cq, ck, workspace=o.new_empty(16))
    with pytest.raises(ValueError, match="out must be"):
        dev.flash_attn_varlen_prefix_fwd(q, k, v, cq, ck, out=q)
    with pytest.raises(ValueError, match="grads"):
        dev.flash_attn_varlen_prefix_bwd(q, k, v, o, q, lse, cq, ck, grads=(o, o[:10], o))
    q4, k4 = torch.zeros(2, 5, 4, 64).bfloat16(), torch.zeros(2, 7, 2, 64).bfloat16()
    with pytest.raises(ValueError, match="flash_attn_prefix expects 4-d"):
        dev.flash_attn_prefix(q, k, v)
    with pytest.raises(ValueError, match="one shape"):
        dev.flash_attn_prefix(q4, k4, k4[:, :3].contiguous())
    with pytest.raises(ValueError, match="disagree on the batch"):
        dev.flash_attn_prefix(q4, k4[:1].contiguous(), k4[:1].contiguous())
    with pytest.raises(ValueError, match="contiguous"):
        dev.flash_attn_prefix(q4.transpose(1, 2), k4, k4)
    assert not [c for c in rec.calls if "bytes" not in c], rec.calls


def test_flash_attn_varlen_prefix_calls_the_prefix_library_forward_and_backward_on_two_arrays(rec):
    from flash_attention_minitorch_amd import device_ops as dev
    Tq, Tk, H, Hkv, d = 300, 200, 4, 2, 64
    q, k, v = (t.requires_grad_() for t in _qkv(Tq, Tk, H, Hkv, d))
    cq, ck = _cu(0, 100, 100, 300), _cu(0, 0, 150, 200)
    rec.reset(dict(q=q, k=k, v=v, cq=cq, ck=ck))
    o = dev.flash_attn_varlen_prefix(q, k, v, cq, ck)
    assert rec.calls == [f"fa_mi355x_fwd_prefix_workspace_bytes(3,{Tq},{Tk},{H},{Hkv},{d})",
                         f"fa_mi355x_fwd_prefix(q,k,v,new0,new1,cq,ck,new2,3,{Tq},{Tk},{H},{Hkv},{d},0.0,1,null)"], rec.calls
    assert o.shape == q.shape and o.dtype.is_floating_point and o.element_size() == 4
    o.sum().backward()
    assert rec.calls[2] == f"fa_mi355x_bwd_prefix_workspace_bytes(3,{Tq},{Tk},{H},{Hkv},{d})"
    assert re.fullmatch(rf"fa_mi355x_bwd_prefix\(q,k,v,new0,new\d,new\d,new\d,new\d,new1,cq,ck,new\d,3,{Tq},{Tk},{H},{Hkv},{d},0.0,1,null\)",
                        rec.calls[3]), rec.calls
    assert len(rec.calls) == 4
    assert q.grad.shape == q.shape and q.grad.dtype == q.dtype and k.grad.shape == k.shape and v.grad.dtype == v.dtype
    # a softmax_scale reaches the library; fp32 is dtype 0
    rec.reset(dict(q=q, k=k, v=v, cq=cq, ck=ck))
    dev.flash_attn_varlen_prefix(q, k, v, cq, ck, 0.25)
    assert rec.calls[1] == f"fa_mi355x_fwd_prefix(q,k,v,new0,new1,cq,ck,new2,3,{Tq},{Tk},{H},{Hkv},{d},0.25,1,null)", rec.calls
    qf, kf, vf = (t.detach().float() for t in (q, k, v))
    rec.reset(dict(q=qf, k=kf, v=vf, cq=cq, ck=ck))
    dev.flash_attn_varlen_prefix(qf, kf, vf, cq, ck)
    assert rec.calls[1].endswith(f",3,{Tq},{Tk},{H},{Hkv},{d},0.0,0,null)"), rec.calls


def test_cu_seqlens_k_none_is_causal_self_attention_on_one_array(rec):
    from flash_attention_minitorch_amd import device_ops as dev
    T, H, Hkv, d = 300, 4, 1, 128
    q, k, v = (t.requires_grad_() for t in _qkv(T, T, H, Hkv, d))
    cu = _cu(0, 100, 300)
    rec.reset(dict(q=q, k=k, v=v, cu=cu))
    o = dev.flash_attn_varlen_prefix(q, k, v, cu)
    o.sum().backward()
    assert rec.calls[:2] == [f"fa_mi355x_fwd_prefix_workspace_bytes(2,{T},{T},{H},{Hkv},{d})",
                             f"fa_mi355x_fwd_prefix(q,k,v,new0,new1,cu,cu,new2,2,{T},{T},{H},{Hkv},{d},0.0,1,null)"], rec.calls
    assert rec.calls[2] == f"fa_mi355x_bwd_prefix_workspace_bytes(2,{T},{T},{H},{Hkv},{d})"
    assert re.fullmatch(rf"fa_mi355x_bwd_prefix\(q,k,v,new0,new\d,new\d,new\d,new\d,new1,cu,cu,new\d,2,{T},{T},{H},{Hkv},{d},0.0,1,null\)",
                        rec.calls[3]) and len(rec.calls) == 4, rec.calls


def test_a_head_dim_of_80_runs_through_zero_padded_columns(rec):
    from flash_attention_minitorch_amd import device_ops as dev
    Tq, Tk, H, Hkv, d = 300, 200, 4, 2, 80
    q, k, v = (t.requires_grad_() for t in _qkv(Tq, Tk, H, Hkv, d))
    cq, ck = _cu(0, 100, 300), _cu(0, 150, 200)
    rec.reset(dict(cq=cq, ck=ck))
    o = dev.flash_attn_varlen_prefix(q, k, v, cq, ck)
    assert o.shape == (Tq, H, d)
    assert rec.calls[1] == f"fa_mi355x_fwd_prefix(new0,new1,new2,new3,new4,cq,ck,new5,2,{Tq},{Tk},{H},{Hkv},128,{80 ** -0.5!r},1,null)", rec.calls
    o.sum().backward()
    assert [c.split("(")[0] for c in rec.calls if "bytes" not in c] == ["fa_mi355x_fwd_prefix", "fa_mi355x_bwd_prefix"]
    assert ",cq,ck,new" in rec.calls[-1] and rec.calls[-1].endswith(f",2,{Tq},{Tk},{H},{Hkv},128,{80 ** -0.5!r},1,null)")
    assert q.grad.shape == q.shape and k.grad.shape == k.shape and q.grad.dtype == q.dtype


def test_flash_attn_prefix_views_the_batch_as_packed_and_builds_both_arrays(rec):
    import torch
    from flash_attention_minitorch_amd import device_ops as dev
    B, Nq, Nk, H, Hkv, d = 3, 50, 70, 4, 2, 64
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn((B, n, h, d), generator=g).bfloat16().requires_grad_() for n, h in ((Nq, H), (Nk, Hkv), (Nk, Hkv)))
    rec.reset(dict(q=q, k=k, v=v))
    o = dev.flash_attn_prefix(q, k, v, 0.5)
    assert o.shape == (B, Nq, H, d) and o.dtype == torch.float32
    assert rec.calls == [f"fa_mi355x_fwd_prefix_workspace_bytes({B},{B * Nq},{B * Nk},{H},{Hkv},{d})",
                         f"fa_mi355x_fwd_prefix(q,k,v,new0,new1,new2,new3,new4,{B},{B * Nq},{B * Nk},{H},{Hkv},{d},0.5,1,null)"], rec.calls
    cu = [t for t in rec.alive if t.dtype == torch.int32]   # the two arrays whose addresses the call took
    assert [t.tolist() for t in cu[:2]] == [[0, 50, 100, 150], [0, 70, 140, 210]]
    o.sum().backward()
    assert rec.calls[3].startswith("fa_mi355x_bwd_prefix(q,k,v,new0,") and ",new1,new2,new3,new" in rec.calls[3] and len(rec.calls) == 4
    assert q.grad.shape == q.shape and k.grad.shape == k.shape and v.grad.shape == v.shape


# ---- the model functions ----

def gather_model(cu, cup, T, Tp):
    """NumPy model of modules_transformer.prefix_gather_index on well-formed arrays: for every row a sequence owns under cu + cup,
    its source row in cat(prefix rows, token rows); -1 for the rows no sequence owns."""
    src = np.full(Tp + T, -1, dtype=np.int64)
    cuk = np.asarray(cu, dtype=np.int64) + np.asarray(cup, dtype=np.int64)
    for b in range(len(cu) - 1):
        n_p, n = int(cup[b + 1] - cup[b]), int(cu[b + 1] - cu[b])
        src[cuk[b]:cuk[b] + n_p] = np.arange(cup[b], cup[b] + n_p)
        src[cuk[b] + n_p:cuk[b] + n_p + n] = Tp + np.arange(cu[b], cu[b] + n)
    return src


@pytest.mark.parametrize("lens,plens,leads", [([5, 3, 9], [0, 4, 2], ((0, 0), (0, 0))), ([1, 130, 64, 7], [37, 0, 130, 1], ((3, 2), (4, 5))),
                                              ([4], [0], ((0, 0), (0, 0))), ([0, 6, 0], [3, 0, 0], ((1, 0), (0, 2)))])
def test_the_gather_index_puts_each_sequences_prefix_rows_in_front_of_its_tokens(lens, plens, leads):
    import torch
    from flash_attention_minitorch_amd import modules_transformer as mt
    (cu, T), (cup, Tp) = pack(lens, *leads[0]), pack(plens, *leads[1])
    got = mt.prefix_gather_index(torch.from_numpy(cu), torch.from_numpy(cup), T, Tp).numpy()
    want = gather_model(cu, cup, T, Tp)
    assert got.shape == want.shape == (Tp + T,) and got.dtype == np.int64
    assert np.array_equal(got[want >= 0], want[want >= 0])
    assert got.min() >= 0 and got.max() < Tp + T   # (the rows no sequence owns stay inside the buffer)
    owned = sum(n for _, n in seq_rows(cu + cup, T + Tp))
    assert (want >= 0).sum() == owned == sum(lens) + sum(plens) and len(set(want[want >= 0])) == owned   # every source row once


@pytest.mark.parametrize("Hkv", [4, 2])
def test_the_prefix_stack_makes_one_attention_call_per_layer_on_cu_plus_cu_prefix(rec, Hkv):
    import torch
    from flash_attention_minitorch_amd import modules_transformer as mt
    T, Tp, H, d, L = 300, 90, 4, 64, 3
    g = torch.Generator().manual_seed(1)
    x = torch.randn((T, H * d), generator=g).to(torch.bfloat16)
    wq, wk = (torch.randn(s, generator=g).to(torch.bfloat16) / 16 for s in ((H * d, H * d), (H * d, Hkv * d)))
    layers = [(wq, wk, wk, wq)] * L
    prefixes = [tuple(torch.randn((Tp, Hkv, d), generator=g).to(torch.bfloat16).requires_grad_() for _ in range(2)) for _ in range(L)]
    cu, cup = _cu(0, 100, 300), _cu(0, 60, 90)
    rec.reset(dict(cu=cu))
    xg = x.clone().requires_grad_()
    y = mt.attention_stack_packed_prefix(xg, cu, prefixes, cup, layers, H)
    assert y.shape == x.shape and y.dtype == x.dtype
    calls = [c for c in rec.calls if "bytes" not in c]
    assert [c.split("(")[0] for c in calls] == ["fa_mi355x_fwd_prefix"] * L
    for c in calls:   # q's array is THE cu_seqlens tensor, k's a new one; the keys have Tp + T rows
        assert re.fullmatch(rf"fa_mi355x_fwd_prefix\(new\d+,new\d+,new\d+,new\d+,new\d+,cu,new\d+,new\d+,2,{T},{T + Tp},{H},{Hkv},{d},0.0,1,null\)", c), c
    cuk = [t for t in rec.alive if t.dtype == torch.int32 and t is not cu and t.shape == cu.shape]
    assert cuk and all(t.tolist() == [0, 160, 390] for t in cuk)
    y.sum().backward()
    names = [c.split("(")[0] for c in rec.calls if "bytes" not in c]
    assert names == ["fa_mi355x_fwd_prefix"] * L + ["fa_mi355x_bwd_prefix"] * L
    assert xg.grad is not None and xg.grad.shape == x.shape
    for pk, pv in prefixes:   # the gradient flows into the prefix rows through the gather
        assert pk.grad is not None and pk.grad.shape == pk.shape and pv.grad is not None and pv.grad.dtype == pv.dtype
    with pytest.raises(ValueError, match="one .prefix_k, prefix_v. per layer"):
        mt.attention_stack_packed_prefix(x, cu, prefixes[:1], cup, layers, H)
    with pytest.raises(ValueError, match="prefix_k and prefix_v must both be"):
        mt.multi_head_attention_packed_prefix(x, cu, prefixes[0][0][:, :1], prefixes[0][1][:, :1], cup, wq, wk, wk, wq, H)
    with pytest.raises(ValueError, match="one length"):
        mt.multi_head_attention_packed_prefix(x, cu, *prefixes[0], _cu(0, 90), wq, wk, wk, wq, H)
