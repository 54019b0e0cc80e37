"""Packed variable-length training calls (include/flash_attn_mi355x_varlen.h, libflash_attn_mi355x_varlen.so), the checks that need
no GPU: the C ABI against _lib.VARLEN_ABI, every argument error before any HIP call, the workspace formula, the library's kernels
(no scratch, names of their own), a NumPy model of the block map (the GPU test holds varlen_schedule_kernel to it), the Python
checks, and the calls device_ops and the model functions make under the recorder of tests/test_device_ops_cpu.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from test_abi_cpu import ROOT, _device_kernels, built  # noqa: F401  (built: the module-scoped build fixture)

HEADER = "flash_attn_mi355x_varlen.h"
SYMBOLS = ["fa_mi355x_fwd_varlen", "fa_mi355x_bwd_varlen", "fa_mi355x_fwd_varlen_workspace_bytes", "fa_mi355x_bwd_varlen_workspace_bytes",
           "fa_mi355x_rope_varlen", "fa_mi355x_varlen_last_error"]
QBLOCK = 128   # query rows per block of the forward and of dQ


def key_block(dtype_is_bf16, d):
    """Key rows per block of dK/dV: NW * 32 of fa_varlen.hip's run."""
    return 256 if dtype_is_bf16 and d <= 64 else 128


# ---- the model of the block map ----

def seq_rows(cu, T):
    """[(s_b, n_b)]: the header's rule (seq_rows of fa_decode.h)."""
    out = []
    for b in range(len(cu) - 1):
        s = min(max(int(cu[b]), 0), T)
        out.append((s, min(max(int(cu[b + 1]), s), T) - s))
    return out


def block_map_model(cu, T, bs):
    """(cap, 4) int32: what varlen_schedule_kernel writes for block size bs.  One entry (s_b, n_b, block, 0) per block of every
    sequence, in order; unused entries (0, 0, -1, 0) up to cap = T // bs + nseq; entries past cap are dropped."""
    cap = T // bs + len(cu) - 1
    ent = [(s, n, blk, 0) for s, n in seq_rows(cu, T) for blk in range((n + bs - 1) // bs)][:cap]
    return np.array(ent + [(0, 0, -1, 0)] * (cap - len(ent)), dtype=np.int32).reshape(cap, 4)


def pack(lengths, lead=0, tail=0):
    """(cu, T) of these lengths with `lead` unowned rows in front and `tail` behind."""
    cu = lead + np.concatenate([[0], np.cumsum(lengths)])
    return cu.astype(np.int32), int(cu[-1]) + tail


_LENGTHS = (0, 1, 31, 32, 33, 127, 128, 129, 255, 256, 257)


@pytest.mark.parametrize("bs", [128, 256])
def test_block_map_partitions_the_owned_rows(bs):
    rng = np.random.default_rng(bs)
    cases = [pack(rng.choice(_LENGTHS, size=n), lead, tail) for n in (1, 2, 5, 11, 40) for lead, tail in ((0, 0), (5, 19), (300, 0))]
    cases += [pack(list(_LENGTHS), 3, 7), pack([0, 0, 0], 2, 2), pack([bs] * 4), pack([bs - 1, bs + 1] * 3)]
    for cu, T in cases:
        m = block_map_model(cu, T, bs)
        used = m[m[:, 2] >= 0]
        assert len(m) == T // bs + len(cu) - 1 and (m[len(used):, 2] == -1).all()   # the bound holds, the unused tail is marked
        owner = np.full(T, -1)
        rows = seq_rows(cu, T)
        for b, (s, n) in enumerate(rows):
            owner[s:s + n] = b
        covered = np.zeros(T, dtype=int)
        for s, n, blk, _ in used:
            lo, hi = s + blk * bs, s + min(n, (blk + 1) * bs)
            assert lo < hi <= T and len(set(owner[lo:hi])) == 1 and owner[lo] >= 0 and rows[owner[lo]] == (s, n)   # no straddle
            covered[lo:hi] += 1
        assert np.array_equal(covered, (owner >= 0).astype(int))   # exactly the owned rows, once
        assert sum((n + bs - 1) // bs for _, n in rows) == len(used) <= T // bs + len(rows)


@pytest.mark.parametrize("bs", [128, 256])
def test_block_map_of_a_bad_cu_stays_inside_the_buffers_and_the_bound(bs):
    T = 300
    for cu in ([0, 200, 9999], [-7, 100, 300], [-50, -20, -1], [500, 600], [300, 0, 300, 0, 300, 0, 300], [0, 2 ** 31 - 1],
               [-2 ** 31, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1]):
        m = block_map_model(np.array(cu, dtype=np.int64), T, bs)
        assert len(m) == T // bs + len(cu) - 1
        for s, n, blk, _ in m[m[:, 2] >= 0]:
            assert 0 <= s and n >= 1 and s + n <= T and 0 <= blk * bs < n
    assert [tuple(r) for r in block_map_model(np.array([0, 200, 9999]), T, 128)] == [(0, 200, 0, 0), (0, 200, 1, 0), (200, 100, 0, 0), (0, 0, -1, 0)]
    assert seq_rows([-7, 100, 300], T) == [(0, 100), (100, 200)]


# ---- the C ABI ----

def test_header_declares_what_the_abi_table_binds_and_the_library_exports(built):
    from test_lib_cpu import _ctypes_kind, _prototypes
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(fa_mi355x_\w+)\s*\(", text))) == sorted(SYMBOLS) == sorted(built.VARLEN_ABI)
    for other in os.listdir(os.path.join(ROOT, "include")):   # no other header gained a declaration
        if other != HEADER:
            assert "varlen" not in open(os.path.join(ROOT, "include", other)).read(), other
    protos = _prototypes(HEADER)
    lib = built.varlen()
    exported = subprocess.run(["nm", "-D", "--defined-only", built.lib_path(built.VARLEN_NAME)], capture_output=True, text=True, check=True).stdout
    for s in SYMBOLS:
        assert hasattr(lib, s) and f" T {s}\n" in exported, s
        res, args = built.VARLEN_ABI[s]
        ret, kinds = protos[s]
        assert [_ctypes_kind(a) for a in args] == kinds and _ctypes_kind(res) == ret, s
        assert getattr(lib, s).argtypes == args and getattr(lib, s).restype is res, s
    needed = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "-d", built.lib_path(built.VARLEN_NAME)], capture_output=True,
                            text=True, check=True).stdout
    assert "libflash_attn_mi355x" not in needed   # a library of its own: it loads without the other three


_ONE = 16   # a fake non-null device pointer: a launch would fail, so any code but the expected one shows a HIP call
_GOOD = dict(q=_ONE, k=_ONE, v=_ONE, out=_ONE, dout=_ONE, dq=_ONE, dk=_ONE, dv=_ONE, lse=_ONE, cu=_ONE, ws=256, nseq=3, T=100, H=4, Hkv=2,
             d=64, scale=0.0, window=8, sink=2, dtype=1)


def _call(lib, bwd, **over):
    a = dict(_GOOD, **over)
    p = lambda n: ctypes.c_void_p(a[n]) if a[n] else None
    tail = (p("cu"), p("ws"), a["nseq"], a["T"], a["H"], a["Hkv"], a["d"], a["scale"], a["window"], a["sink"], a["dtype"], None)
    if bwd:
        rc = lib.fa_mi355x_bwd_varlen(p("q"), p("k"), p("v"), p("out"), p("dout"), p("dq"), p("dk"), p("dv"), p("lse"), *tail)
    else:
        rc = lib.fa_mi355x_fwd_varlen(p("q"), p("k"), p("v"), p("out"), p("lse"), *tail)
    return rc, lib.fa_mi355x_varlen_last_error().decode()


_BAD = [
    (dict(window=-3), "window must not be negative"), (dict(sink=-1), "sink must not be negative"),
    (dict(window=0, sink=2), "sink tokens need a window"),
    (dict(H=4, Hkv=3), "Hkv must be positive and divide H"), (dict(Hkv=0), "Hkv must be positive and divide H"),
    (dict(d=80), "d must be 32, 64 or 128"), (dict(d=256), "d must be 32, 64 or 128"),
    (dict(nseq=0), "must be positive"), (dict(nseq=-2), "must be positive"), (dict(T=0), "must be positive"), (dict(H=0), "must be positive"),
    (dict(d=0), "must be positive"),
    (dict(dtype=2), "unknown dtype"),
    (dict(scale=-1.0), "softmax_scale"), (dict(scale=float("nan")), "softmax_scale"), (dict(scale=float("inf")), "softmax_scale"),
    (dict(T=1 << 22, d=128), "under 2 GiB"), (dict(T=1 << 20, H=16, Hkv=16, d=128), "under 2 GiB"),
    (dict(ws=128), "256-byte aligned"),
] + [(dict({n: 0}), "null pointer argument") for n in ("q", "k", "v", "out", "lse", "cu", "ws")]
_BAD_BWD = [(dict({n: 0}), "null pointer argument") for n in ("dout", "dq", "dk", "dv")]


@pytest.mark.parametrize("bwd,over,msg", [(b, o, m) for b in (False, True) for o, m in _BAD] + [(True, o, m) for o, m in _BAD_BWD],
                         ids=lambda x: "-".join(f"{k}={v}" for k, v in x.items()) if isinstance(x, dict) else None)
def test_each_bad_argument_is_rejected_before_any_hip_call(built, bwd, over, msg):
    """The varlen library alone, no GPU: FA_ERR_BAD_ARG = 1 and the message; the fake pointers would make any launch fail with
    FA_ERR_HIP = 3.  A call that passes the checks must not be made here."""
    rc, err = _call(built.varlen(), bwd, **over)
    assert rc == 1 and msg in err, (rc, err)


_ROPE_GOOD = dict(x=_ONE, y=_ONE, cos=_ONE, sin=_ONE, cu=_ONE, nseq=3, T=100, H=4, d=64, rot=32, max_pos=512, interleaved=0, inverse=0, dtype=1)


@pytest.mark.parametrize("over,msg", [
    (dict(nseq=0), "must be positive"), (dict(T=0), "must be positive"), (dict(H=-1), "must be positive"), (dict(d=0), "must be positive"),
    (dict(dtype=3), "unknown dtype"), (dict(x=0), "null pointer"), (dict(y=0), "null pointer"), (dict(cu=0), "null pointer"),
    (dict(cos=0), "null cos or sin"), (dict(sin=0), "null cos or sin"), (dict(interleaved=2), "interleaved must be"),
    (dict(inverse=-1), "inverse must be"), (dict(rot=0), "must be even"), (dict(rot=7), "must be even"), (dict(rot=66), "must be even"),
    (dict(max_pos=0), "max_pos must be positive"), (dict(T=1 << 30, H=64, d=128), "too many elements"),
], ids=lambda x: "-".join(f"{k}={v}" for k, v in x.items()) if isinstance(x, dict) else None)
def test_each_bad_rope_argument_is_rejected_before_any_hip_call(built, over, msg):
    a = dict(_ROPE_GOOD, **over)
    p = lambda n: ctypes.c_void_p(a[n]) if a[n] else None
    lib = built.varlen()
    rc = lib.fa_mi355x_rope_varlen(p("x"), p("y"), p("cos"), p("sin"), p("cu"), a["nseq"], a["T"], a["H"], a["d"], a["rot"], a["max_pos"],
                                   a["interleaved"], a["inverse"], a["dtype"], None)
    err = lib.fa_mi355x_varlen_last_error().decode()
    assert rc == 1 and msg in err, (rc, err)


def _align(x):
    return (x + 255) // 256 * 256


def test_workspace_bytes_are_the_headers_formula(built):
    fwd, bwd = built.varlen().fa_mi355x_fwd_varlen_workspace_bytes, built.varlen().fa_mi355x_bwd_varlen_workspace_bytes
    for nseq, T, H, Hkv, d in ((1, 1, 1, 1, 32), (6, 572, 4, 4, 64), (6, 572, 4, 2, 64), (40, 552, 4, 1, 128), (256, 32768, 32, 8, 128)):
        mp = _align(16 * (T // QBLOCK + nseq))
        assert fwd(nseq, T, H, Hkv, d) == mp
        vecs = 3 * H * T * 4
        assert bwd(nseq, T, H, Hkv, d) == (2 * mp + vecs if Hkv == H else 2 * mp + _align(vecs) + 2 * H * T * d * 4)
        assert bwd(nseq, T, H, Hkv, d) >= fwd(nseq, T, H, Hkv, d)
    for f in (fwd, bwd):
        assert f(0, 100, 4, 2, 64) == f(2, 0, 4, 2, 64) == f(2, 100, 0, 2, 64) == f(2, 100, 4, 3, 64) == f(2, 100, 4, 0, 64) == f(2, 100, 4, 2, 0) == 0
        assert f(-1, 100, 4, 2, 64) == f(2, -5, 4, 2, 64) == 0


# ---- the kernels ----

def test_every_kernel_of_the_varlen_library_has_no_scratch_and_a_name_of_its_own(built):
    kernels = _device_kernels(built.lib_path(built.VARLEN_NAME))
    names = [k[0] for k in kernels]
    for stem in ("varlen_fwd_kernel", "varlen_dq_kernel", "varlen_dkdv_kernel", "bwd_prep_kernel"):
        assert sum(stem in n for n in names) == 6, (stem, names)   # bf16 and fp32 at d = 32, 64, 128
    assert sum("rope_varlen_kernel" in n for n in names) == 8      # bf16 and fp32, 16-byte and element lanes, NeoX and GPT-J pairs
    assert sum("varlen_schedule_kernel" in n for n in names) == 1 and sum("group_sum_kernel" in n for n in names) == 1
    assert not [n for n in names if "win_fwd_kernel" in n or "win_dq_kernel" in n or "win_dkdv_kernel" in n]
    for name, scratch, vgpr in kernels:
        assert scratch == 0, (name, scratch)
        assert vgpr <= 512, (name, vgpr)


# ---- Python: the checks, and the calls under the recorder ----

@pytest.fixture
def rec(monkeypatch):
    from flash_attention_minitorch_amd import _lib
    from test_device_ops_cpu import install_recorder
    r = install_recorder(monkeypatch)
    for sym in ("fa_mi355x_fwd_varlen_workspace_bytes", "fa_mi355x_bwd_varlen_workspace_bytes"):
        log = getattr(r, sym)
        r.__dict__[sym] = lambda *a, log=log: log(*a) or 4096   # (logged like the others, with a size)
    monkeypatch.setattr(_lib, "varlen", lambda: r)
    monkeypatch.setattr(_lib, "window", lambda: r)
    return r


def _qkv(T=300, H=4, Hkv=2, d=64, dtype=None):
    import torch
    g = torch.Generator().manual_seed(T)
    return [torch.randn((T, h, d), generator=g).to(dtype or torch.bfloat16) for h in (H, Hkv, Hkv)]


def _cu(*entries):
    import torch
    return torch.tensor(entries, dtype=torch.int32)


def test_python_checks_raise_before_any_launch(rec):
    import torch
    from flash_attention_minitorch_amd import device_ops as dev
    q, k, v = _qkv()
    cu = _cu(0, 100, 300)
    for kw, msg in ((dict(window=-1), "negative"), (dict(window=1.5), "int"), (dict(window=True), "int"), (dict(window=8, sink=-2), "negative"),
                    (dict(sink=2), "needs window"), (dict(window=0, sink=2), "needs window"), (dict(window=8, sink="a"), "int")):
        with pytest.raises(ValueError, match=msg):
            dev.flash_attn_varlen(q, k, v, cu, **kw)
        with pytest.raises(ValueError, match=msg):
            dev.flash_attn_varlen_fwd(q, k, v, cu, **kw)
    with pytest.raises(ValueError, match="non-causal packed attention is not built"):
        dev.flash_attn_varlen(q, k, v, cu, causal=False)
    with pytest.raises(ValueError, match="native head dim"):
        dev.flash_attn_varlen_fwd(*_qkv(d=80), cu)
    with pytest.raises(ValueError, match="multiple"):
        dev.flash_attn_varlen_fwd(*_qkv(H=4, Hkv=3), cu)
    with pytest.raises(ValueError, match="3-d"):
        dev.flash_attn_varlen_fwd(q[None], k[None], v[None], cu)
    with pytest.raises(ValueError, match="disagree"):
        dev.flash_attn_varlen_fwd(q, k[:200].contiguous(), v[:200].contiguous(), cu)
    with pytest.raises(ValueError, match="one shape"):
        dev.flash_attn_varlen_fwd(q, k, v[:, :1].contiguous(), cu)
    with pytest.raises(ValueError, match="contiguous"):
        dev.flash_attn_varlen_fwd(q.transpose(0, 1).contiguous().transpose(0, 1), k, v, cu)
    for bad in (cu.long(), cu[:1], cu[None], [0, 100, 300], None):
        with pytest.raises(ValueError, match="cu_seqlens"):
            dev.flash_attn_varlen_fwd(q, k, v, bad)
        with pytest.raises(ValueError, match="cu_seqlens"):
            dev.apply_rotary_varlen(q, torch.zeros(8, 16), torch.zeros(8, 16), bad)
    o, lse = q.float(), q.float()[..., 0].transpose(0, 1).contiguous()
    with pytest.raises(ValueError, match="out_grad"):
        dev.flash_attn_varlen_bwd(q, k, v, o, k, lse, cu)
    with pytest.raises(ValueError, match="lse"):
        dev.flash_attn_varlen_bwd(q, k, v, o, q, lse[:, :10], cu)
    with pytest.raises(ValueError, match="workspace too small"):
        dev.flash_attn_varlen_bwd(q, k, v, o, q, lse, cu, workspace=o.new_empty(16))
    with pytest.raises(ValueError, match="workspace too small"):
        dev.flash_attn_varlen_fwd(q, k, v, cu, workspace=o.new_empty(16))
    with pytest.raises(ValueError, match="out must be"):
        dev.flash_attn_varlen_fwd(q, k, v, cu, out=q)
    with pytest.raises(ValueError, match="rotary dimension"):
        dev.apply_rotary_varlen(q, torch.zeros(8, 64), torch.zeros(8, 64), cu)
    with pytest.raises(ValueError, match="3-d"):
        dev.apply_rotary_varlen(q[None], torch.zeros(8, 16), torch.zeros(8, 16), cu)
    assert not [c for c in rec.calls if "bytes" not in c], rec.calls


def test_flash_attn_varlen_calls_the_varlen_library_forward_and_backward(rec):
    from flash_attention_minitorch_amd import device_ops as dev
    T, H, Hkv, d, W, S = 300, 4, 2, 64, 48, 3
    q, k, v = (t.requires_grad_() for t in _qkv(T, H, Hkv, d))
    cu = _cu(0, 100, 100, 300)
    rec.reset(dict(q=q, k=k, v=v, cu=cu))
    o = dev.flash_attn_varlen(q, k, v, cu, window=W, sink=S)
    assert rec.calls == [f"fa_mi355x_fwd_varlen_workspace_bytes(3,{T},{H},{Hkv},{d})",
                         f"fa_mi355x_fwd_varlen(q,k,v,new0,new1,cu,new2,3,{T},{H},{Hkv},{d},0.0,{W},{S},1,null)"], rec.calls
    assert o.shape == q.shape and o.dtype.is_floating_point and o.element_size() == 4
    o.sum().backward()
    assert rec.calls[2] == f"fa_mi355x_bwd_varlen_workspace_bytes(3,{T},{H},{Hkv},{d})"
    assert re.fullmatch(rf"fa_mi355x_bwd_varlen\(q,k,v,new0,new\d,new\d,new\d,new\d,new1,cu,new\d,3,{T},{H},{Hkv},{d},0.0,{W},{S},1,null\)",
                        rec.calls[3]), rec.calls
    assert len(rec.calls) == 4
    assert q.grad.shape == q.shape and k.grad.shape == k.shape and v.grad.dtype == v.dtype
    # no window: W = S = 0 (the library's "every j <= i"), whatever the lengths; a softmax_scale reaches the library
    for kw in (dict(), dict(window=None, sink=None), dict(window=0), dict(window=0, sink=0)):
        rec.reset(dict(q=q, k=k, v=v, cu=cu))
        dev.flash_attn_varlen(q, k, v, cu, True, 0.25, **kw)
        assert rec.calls[1] == f"fa_mi355x_fwd_varlen(q,k,v,new0,new1,cu,new2,3,{T},{H},{Hkv},{d},0.25,0,0,1,null)", (kw, rec.calls)
    # a window wider than everything stays the caller's window: the kernels clamp it per sequence
    rec.reset(dict(q=q, k=k, v=v, cu=cu))
    dev.flash_attn_varlen(q, k, v, cu, window=4096)
    assert rec.calls[1].endswith(",0.0,4096,0,1,null)")


def test_a_head_dim_of_80_runs_through_zero_padded_columns(rec):
    from flash_attention_minitorch_amd import device_ops as dev
    T, H, Hkv, d = 300, 4, 2, 80
    q, k, v = (t.requires_grad_() for t in _qkv(T, H, Hkv, d))
    cu = _cu(0, 100, 300)
    rec.reset(dict(cu=cu))
    o = dev.flash_attn_varlen(q, k, v, cu, window=48)
    assert o.shape == (T, H, d)
    assert rec.calls[1] == f"fa_mi355x_fwd_varlen(new0,new1,new2,new3,new4,cu,new5,2,{T},{H},{Hkv},128,{80 ** -0.5!r},48,0,1,null)", rec.calls
    o.sum().backward()
    assert [c.split("(")[0] for c in rec.calls if "bytes" not in c] == ["fa_mi355x_fwd_varlen", "fa_mi355x_bwd_varlen"]
    assert f",2,{T},{H},{Hkv},128,{80 ** -0.5!r},48,0,1,null)" in rec.calls[-1]
    assert q.grad.shape == q.shape and k.grad.shape == k.shape and q.grad.dtype == q.dtype


@pytest.mark.parametrize("Hkv", [4, 2])
def test_the_packed_stack_hands_cu_seqlens_to_every_call_of_every_layer(rec, Hkv):
    import torch
    from flash_attention_minitorch_amd import modules_transformer as mt
    T, H, d, W, S, L = 300, 4, 64, 48, 3, 3
    g = torch.Generator().manual_seed(1)
    x = torch.randn((T, H * d), generator=g).to(torch.bfloat16)
    wq, wk = (torch.randn(s, generator=g).to(torch.bfloat16) / 16 for s in ((H * d, H * d), (H * d, Hkv * d)))
    layers = [(wq, wk, wk, wq)] * L
    rope = mt.Rotary(*(torch.zeros(T, d // 4) for _ in range(2)))
    cu = _cu(0, 100, 300)
    rec.reset(dict(cu=cu, cos=rope.cos, sin=rope.sin))
    xg = x.clone().requires_grad_()
    y = mt.attention_stack_packed(xg, cu, layers, H, rope=rope, window=W, sink=S)
    assert y.shape == x.shape
    names = [c.split("(")[0] for c in rec.calls if "bytes" not in c]
    assert names == ["fa_mi355x_rope_varlen", "fa_mi355x_rope_varlen", "fa_mi355x_fwd_varlen"] * L   # the rotation comes first
    y.sum().backward()
    calls = [c for c in rec.calls if "bytes" not in c]
    names = [c.split("(")[0] for c in calls]
    assert sorted(names[3 * L:]) == sorted(["fa_mi355x_rope_varlen", "fa_mi355x_rope_varlen", "fa_mi355x_bwd_varlen"] * L), names
    for c in calls:   # every call takes THE cu_seqlens tensor, and its shapes
        if c.startswith("fa_mi355x_rope_varlen("):
            heads = re.fullmatch(rf"fa_mi355x_rope_varlen\(\w+,\w+,cos,sin,cu,2,{T},(\d+),{d},{d // 2},{T},0,([01]),1,null\)", c)
            assert heads and int(heads.group(1)) in (H, Hkv), c
        else:
            assert f",cu,new" in c and c.endswith(f",2,{T},{H},{Hkv},{d},0.0,{W},{S},1,null)"), c
    inverse = [c for c in calls[3 * L:] if c.startswith("fa_mi355x_rope_varlen(")]
    assert all(c.endswith(",0,1,1,null)") for c in inverse) and len(inverse) == 2 * L   # the backward is the inverse rotation
    assert xg.grad is not None and xg.grad.shape == x.shape
    # one layer, unwindowed, with the scale folded into wq: softmax_scale = ln 2
    rec.reset(dict(cu=cu))
    mt.multi_head_attention_packed(x, cu, wq, wk, wk, wq, H, fold_scale=True)
    call = [c for c in rec.calls if c.startswith("fa_mi355x_fwd_varlen(")]
    assert len(call) == 1 and ",cu,new" in call[0] and call[0].endswith(f",2,{T},{H},{Hkv},{d},{mt.LN2!r},0,0,1,null)"), rec.calls
