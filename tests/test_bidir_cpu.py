"""Bidirectional packed attention with separate cu_seqlens for q and k (include/flash_attn_mi355x_bidir.h,
libflash_attn_mi355x_bidir.so), the checks that need no GPU: the C ABI against _lib.BIDIR_ABI, every argument error before any HIP
call, the workspace formula, the library's kernels (no scratch, names of their own), a NumPy model of the two block maps (the GPU
test holds bidir_schedule_kernel to it), the Python checks, and the calls device_ops and the model functions make under the recorder
of tests/test_device_ops_cpu.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from test_abi_cpu import ROOT, _device_kernels, built  # noqa: F401  (built: the module-scoped build fixture)
from test_varlen_cpu import pack, seq_rows

HEADER = "flash_attn_mi355x_bidir.h"
SYMBOLS = ["fa_mi355x_fwd_bidir", "fa_mi355x_bwd_bidir", "fa_mi355x_fwd_bidir_workspace_bytes", "fa_mi355x_bwd_bidir_workspace_bytes",
           "fa_mi355x_bidir_last_error"]
QBLOCK = 128   # query rows per block of the forward and of dQ; the rows both maps are sized for
UNUSED = (0, 0, 0, 0, -1, 0, 0, 0)


def key_block(dtype_is_bf16, d):
    """Key rows per block of dK/dV: NW * 32 of fa_bidir.hip's run."""
    return 256 if dtype_is_bf16 and d <= 64 else 128


# ---- the model of the two block maps ----

def block_map_model(cu_q, Tq, cu_k, Tk, bs, keys):
    """(cap, 8) int32: what bidir_schedule_kernel writes for the query blocks (keys=False: counted in cu_q against Tq) or the key
    blocks (keys=True: cu_k, Tk) at block size bs.  One entry (s_q, n_q, s_k, n_k, block, sequence, 0, 0) per block of every
    sequence that has a row on that side, in order; unused entries (0, 0, 0, 0, -1, 0, 0, 0) up to cap = T // bs + nseq; entries past
    cap are dropped."""
    rq, rk = seq_rows(cu_q, Tq), seq_rows(cu_k, Tk)
    cap = (Tk if keys else Tq) // bs + len(rq)
    ent = [(*rq[b], *rk[b], blk, b, 0, 0) for b in range(len(rq)) for blk in range(((rk if keys else rq)[b][1] + bs - 1) // bs)][:cap]
    return np.array(ent + [UNUSED] * (cap - len(ent)), dtype=np.int32).reshape(cap, 8)


_LENGTHS = (0, 1, 31, 32, 33, 127, 128, 129, 255, 256, 257)


@pytest.mark.parametrize("bs", [128, 256])
def test_block_maps_partition_the_owned_rows_of_their_side_and_carry_the_other(bs):
    rng = np.random.default_rng(bs)
    cases = []
    for n in (1, 2, 5, 11, 40):
        for (lq, tq), (lk, tk) in (((0, 0), (0, 0)), ((5, 19), (3, 0)), ((300, 0), (0, 7))):
            cases.append((pack(rng.choice(_LENGTHS, size=n), lq, tq), pack(rng.choice(_LENGTHS, size=n), lk, tk)))
    cases += [(pack(list(_LENGTHS), 3, 7), pack(list(_LENGTHS)[::-1], 1, 0)), (pack([0, 0, 0], 2, 2), pack([5, 0, 300])),
              (pack([bs] * 4), pack([bs - 1, bs + 1] * 2))]
    for (cu_q, Tq), (cu_k, Tk) in cases:
        rq, rk = seq_rows(cu_q, Tq), seq_rows(cu_k, Tk)
        for keys, T, mine in ((False, Tq, rq), (True, Tk, rk)):
            m = block_map_model(cu_q, Tq, cu_k, Tk, bs, keys)
            assert np.array_equal(m, block_map_model(cu_q.copy(), Tq, cu_k.copy(), Tk, bs, keys))   # a function of the arrays alone
            used = m[m[:, 4] >= 0]
            assert len(m) == T // bs + len(rq) and all(tuple(r) == UNUSED for r in m[len(used):])   # the cap holds, the tail is marked
            owner = np.full(T, -1)
            for b, (s, n) in enumerate(mine):
                owner[s:s + n] = b
            covered = np.zeros(T, dtype=int)
            for sq, nq, sk, nk, blk, b, z0, z1 in used:
                assert (sq, nq) == rq[b] and (sk, nk) == rk[b] and z0 == z1 == 0   # both sides of the block's sequence
                s, n = (sk, nk) if keys else (sq, nq)
                lo, hi = s + blk * bs, s + min(n, (blk + 1) * bs)
                assert lo < hi <= T and set(owner[lo:hi]) == {b}   # no straddle
                covered[lo:hi] += 1
            assert np.array_equal(covered, (owner >= 0).astype(int))   # exactly the owned rows, once
            assert sum((n + bs - 1) // bs for _, n in mine) == len(used) <= T // bs + len(mine)


@pytest.mark.parametrize("bs", [128, 256])
def test_block_maps_of_bad_arrays_stay_inside_the_buffers_and_the_caps(bs):
    Tq, Tk = 300, 500
    bad = ([0, 200, 9999], [-7, 100, 300], [-50, -20, -1], [500, 600, 700], [300, 0, 300], [0, 2 ** 31 - 1, -2 ** 31],
           [-2 ** 31, 2 ** 31 - 1, -2 ** 31])
    for cu_q in bad:
        for cu_k in bad:
            for keys, T in ((False, Tq), (True, Tk)):
                m = block_map_model(np.array(cu_q, dtype=np.int64), Tq, np.array(cu_k, dtype=np.int64), Tk, bs, keys)
                assert len(m) == T // bs + 2
                for sq, nq, sk, nk, blk, b, _, _ in m[m[:, 4] >= 0]:
                    assert 0 <= sq and nq >= 0 and sq + nq <= Tq and 0 <= sk and nk >= 0 and sk + nk <= Tk
                    assert 0 <= blk * bs < (nk if keys else nq) and 0 <= b < 2
    m = block_map_model(np.array([0, 200, 9999]), 300, np.array([-7, 0, 40]), 500, 128, False)
    assert [tuple(r) for r in m] == [(0, 200, 0, 0, 0, 0, 0, 0), (0, 200, 0, 0, 1, 0, 0, 0), (200, 100, 0, 40, 0, 1, 0, 0), UNUSED]
    # cu saturating the cap: every sequence claims all 300 rows, three blocks each, and the map holds 300 // 128 + 3 = 5 of the 6
    m = block_map_model(np.array([0, 300, 0, 300]), 300, np.array([0, 1, 2, 3]), 500, 128, False)
    assert [tuple(r[[0, 1, 4, 5]]) for r in m] == [(0, 300, 0, 0), (0, 300, 1, 0), (0, 300, 2, 0), (0, 300, 0, 2), (0, 300, 1, 2)]


# ---- the C ABI ----

def test_header_declares_what_the_abi_table_binds_and_the_library_exports(built):
    from test_lib_cpu import _ctypes_kind, _prototypes
    raw = open(os.path.join(ROOT, "include", HEADER)).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert sorted(set(re.findall(r"\b(fa_mi355x_\w+)\s*\(", text))) == sorted(SYMBOLS) == sorted(built.BIDIR_ABI)
    for other in os.listdir(os.path.join(ROOT, "include")):   # no other header gained a declaration
        if other != HEADER:
            assert "bidir" not in open(os.path.join(ROOT, "include", other)).read(), other
    for scope in ("Not in this library", "causal mask under two different arrays", "windows and sinks", "dropout", "fp8",
                  "host-pointer reference ABI", "MFMA-slot"):   # what is out of scope is stated as such
        assert scope in raw, scope
    protos = _prototypes(HEADER)
    lib = built.bidir()
    exported = subprocess.run(["nm", "-D", "--defined-only", built.lib_path(built.BIDIR_NAME)], capture_output=True, text=True, check=True).stdout
    assert sorted(re.findall(r" T (fa_mi355x_\w+)\n", exported)) == sorted(SYMBOLS)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        res, args = built.BIDIR_ABI[s]
        ret, kinds = protos[s]
        assert [_ctypes_kind(a) for a in args] == kinds and _ctypes_kind(res) == ret, s
        assert getattr(lib, s).argtypes == args and getattr(lib, s).restype is res, s
    needed = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "-d", built.lib_path(built.BIDIR_NAME)], capture_output=True,
                            text=True, check=True).stdout
    assert "libflash_attn_mi355x" not in needed   # a library of its own: it loads without the other four


_ONE = 16   # a fake non-null device pointer: a launch would fail, so any code but the expected one shows a HIP call
_GOOD = dict(q=_ONE, k=_ONE, v=_ONE, out=_ONE, dout=_ONE, dq=_ONE, dk=_ONE, dv=_ONE, lse=_ONE, cu_q=_ONE, cu_k=_ONE, ws=256, nseq=3, Tq=100,
             Tk=70, H=4, Hkv=2, d=64, scale=0.0, dtype=1)


def _call(lib, bwd, **over):
    a = dict(_GOOD, **over)
    p = lambda n: ctypes.c_void_p(a[n]) if a[n] else None
    tail = (p("cu_q"), p("cu_k"), p("ws"), a["nseq"], a["Tq"], a["Tk"], a["H"], a["Hkv"], a["d"], a["scale"], a["dtype"], None)
    if bwd:
        rc = lib.fa_mi355x_bwd_bidir(p("q"), p("k"), p("v"), p("out"), p("dout"), p("dq"), p("dk"), p("dv"), p("lse"), *tail)
    else:
        rc = lib.fa_mi355x_fwd_bidir(p("q"), p("k"), p("v"), p("out"), p("lse"), *tail)
    return rc, lib.fa_mi355x_bidir_last_error().decode()


_BAD = [
    (dict(H=4, Hkv=3), "Hkv must be positive and divide H"), (dict(Hkv=0), "Hkv must be positive and divide H"),
    (dict(d=80), "d must be 32, 64 or 128"), (dict(d=256), "d must be 32, 64 or 128"),
    (dict(nseq=0), "must be positive"), (dict(nseq=-2), "must be positive"), (dict(Tq=0), "must be positive"), (dict(Tk=0), "must be positive"),
    (dict(Tk=-4), "must be positive"), (dict(H=0), "must be positive"), (dict(d=0), "must be positive"),
    (dict(dtype=2), "unknown dtype"),
    (dict(scale=-1.0), "softmax_scale"), (dict(scale=float("nan")), "softmax_scale"), (dict(scale=float("inf")), "softmax_scale"),
    (dict(Tq=1 << 22, d=128), "Tq too large"), (dict(Tk=1 << 22, d=128), "Tk too large"),
    (dict(Tq=1 << 20, H=16, Hkv=16, d=128), "queries must stay under 2 GiB"), (dict(Tk=1 << 20, H=16, Hkv=16, d=128), "keys must stay under 2 GiB"),
    (dict(ws=128), "256-byte aligned"),
] + [(dict({n: 0}), "null pointer argument") for n in ("q", "k", "v", "out", "lse", "cu_q", "cu_k", "ws")]
_BAD_BWD = [(dict({n: 0}), "null pointer argument") for n in ("dout", "dq", "dk", "dv")]


@pytest.mark.parametrize("bwd,over,msg", [(b, o, m) for b in (False, True) for o, m in _BAD] + [(True, o, m) for o, m in _BAD_BWD],
                         ids=lambda x: "-".join(f"{k}={v}" for k, v in x.items()) if isinstance(x, dict) else None)
def test_each_bad_argument_is_rejected_before_any_hip_call(built, bwd, over, msg):
    """The bidir library alone, no GPU: FA_ERR_BAD_ARG = 1 and the message; the fake pointers would make any launch fail with
    FA_ERR_HIP = 3.  A call that passes the checks must not be made here."""
    rc, err = _call(built.bidir(), bwd, **over)
    assert rc == 1 and msg in err, (rc, err)


def _align(x):
    return (x + 255) // 256 * 256


def test_workspace_bytes_are_the_headers_formula(built):
    fwd, bwd = built.bidir().fa_mi355x_fwd_bidir_workspace_bytes, built.bidir().fa_mi355x_bwd_bidir_workspace_bytes
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

def test_every_kernel_of_the_bidir_library_has_no_scratch_and_a_name_of_its_own(built):
    kernels = _device_kernels(built.lib_path(built.BIDIR_NAME))
    names = [k[0] for k in kernels]
    for stem in ("bidir_fwd_kernel", "bidir_dq_kernel", "bidir_dkdv_kernel", "bwd_prep_kernel"):
        assert sum(stem in n for n in names) == 6, (stem, names)   # bf16 and fp32 at d = 32, 64, 128
    assert sum("bidir_schedule_kernel" in n for n in names) == 1 and sum("group_sum_kernel" in n for n in names) == 1
    # no kernel of another library: what is left is mfma_peak_kernel, which comes along with fa_aux.h and is not launched
    stems = ("bidir_fwd_kernel", "bidir_dq_kernel", "bidir_dkdv_kernel", "bidir_schedule_kernel", "bwd_prep_kernel", "group_sum_kernel")
    assert [n for n in names if not any(s in n for s in stems)] == [n for n in names if "mfma_peak_kernel" in n]
    assert not [n for n in names if "win_" in n or "varlen_" in n or "decode" in n or "ragged" in n]
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
    for sym in ("fa_mi355x_fwd_bidir_workspace_bytes", "fa_mi355x_bwd_bidir_workspace_bytes"):
        log = getattr(r, sym)
        r.__dict__[sym] = lambda *a, log=log: log(*a) or 4096   # (logged like the others, with a size)
    monkeypatch.setattr(_lib, "bidir", lambda: r)
    monkeypatch.setattr(_lib, "varlen", lambda: r)
    return r


def _qkv(Tq=300, Tk=200, H=4, Hkv=2, d=64, dtype=None):
    import torch
    g = torch.Generator().manual_seed(Tq + Tk)
    return [torch.randn((t, h, d), generator=g).to(dtype or torch.bfloat16) for t, h in ((Tq, H), (Tk, Hkv), (Tk, Hkv))]


def _cu(*entries):
    import torch
    return torch.tensor(entries, dtype=torch.int32)


def test_python_checks_raise_before_any_launch(rec):
    from flash_attention_minitorch_amd import device_ops as dev
    q, k, v = _qkv()
    cq, ck = _cu(0, 100, 300), _cu(0, 150, 200)
    with pytest.raises(ValueError, match="native head dim"):
        dev.flash_attn_varlen_bidir_fwd(*_qkv(d=80), cq, ck)
    with pytest.raises(ValueError, match="multiple"):
        dev.flash_attn_varlen_bidir_fwd(*_qkv(H=4, Hkv=3), cq, ck)
    with pytest.raises(ValueError, match="3-d"):
        dev.flash_attn_varlen_bidir_fwd(q[None], k[None], v[None], cq, ck)
    with pytest.raises(ValueError, match="disagree on the head dim"):
        dev.flash_attn_varlen_bidir_fwd(q, k[..., :32].contiguous(), v[..., :32].contiguous(), cq, ck)
    with pytest.raises(ValueError, match="one shape"):
        dev.flash_attn_varlen_bidir_fwd(q, k, v[:, :1].contiguous(), cq, ck)
    with pytest.raises(ValueError, match="one dtype"):
        dev.flash_attn_varlen_bidir_fwd(q, k.float(), v.float(), cq, ck)
    with pytest.raises(TypeError):
        dev.flash_attn_varlen_bidir_fwd(q.half(), k.half(), v.half(), cq, ck)
    with pytest.raises(ValueError, match="contiguous"):
        dev.flash_attn_varlen_bidir_fwd(q.transpose(0, 1).contiguous().transpose(0, 1), k, v, cq, ck)
    with pytest.raises(ValueError, match="self-attention: k must have q's 300 rows"):
        dev.flash_attn_varlen_bidir_fwd(q, k, v, cq)
    with pytest.raises(ValueError, match="self-attention"):
        dev.flash_attn_varlen_bidir(q, k, v, cq)
    with pytest.raises(ValueError, match="one length"):
        dev.flash_attn_varlen_bidir_fwd(q, k, v, cq, _cu(0, 50, 150, 200))
    for bad in (cq.long(), cq[:1], cq[None], [0, 100, 300]):
        with pytest.raises(ValueError, match="cu_seqlens"):
            dev.flash_attn_varlen_bidir_fwd(q, k, v, bad, ck)
        with pytest.raises(ValueError, match="cu_seqlens"):
            dev.flash_attn_varlen_bidir_fwd(q, k, v, cq, bad)
    with pytest.raises(ValueError, match="cu_seqlens"):
        dev.flash_attn_varlen_bidir_fwd(q, k, v, None, ck)
    o, lse = q.float(), q.float()[..., 0].transpose(0, 1).contiguous()
    with pytest.raises(ValueError, match="out_grad"):
        dev.flash_attn_varlen_bidir_bwd(q, k, v, o, k, lse, cq, ck)
    with pytest.raises(ValueError, match="lse"):
        dev.flash_attn_varlen_bidir_bwd(q, k, v, o, q, lse[:, :10], cq, ck)
    with pytest.raises(ValueError, match="workspace too small"):
        dev.flash_attn_varlen_bidir_bwd(q, k, v, o, q, lse, cq, ck, workspace=o.new_empty(16))
    with pytest.raises(ValueError, match="workspace too small"):
        dev.flash_attn_varlen_bidir_fwd(q, k, v, cq, ck, workspace=o.new_empty(16))
    with pytest.raises(ValueError, match="out must be"):
        dev.flash_attn_varlen_bidir_fwd(q, k, v, cq, ck, out=q)
    with pytest.raises(ValueError, match="grads"):
        dev.flash_attn_varlen_bidir_bwd(q, k, v, o, q, lse, cq, ck, grads=(o, o[:10], o))
    import torch
    q4, k4 = torch.zeros(2, 5, 4, 64).bfloat16(), torch.zeros(2, 7, 2, 64).bfloat16()
    with pytest.raises(ValueError, match="4-d"):
        dev.flash_attn_cross(q, k, v)
    with pytest.raises(ValueError, match="one shape"):
        dev.flash_attn_cross(q4, k4, k4[:, :3].contiguous())
    with pytest.raises(ValueError, match="disagree on the batch"):
        dev.flash_attn_cross(q4, k4[:1].contiguous(), k4[:1].contiguous())
    with pytest.raises(ValueError, match="contiguous"):
        dev.flash_attn_cross(q4.transpose(1, 2), k4, k4)
    assert not [c for c in rec.calls if "bytes" not in c], rec.calls


def test_the_causal_packed_call_still_refuses_causal_false(rec):
    from flash_attention_minitorch_amd import device_ops as dev
    q, k, v = _qkv(300, 300)
    with pytest.raises(ValueError, match="non-causal packed attention is not built"):
        dev.flash_attn_varlen(q, k, v, _cu(0, 100, 300), causal=False)
    assert not rec.calls


def test_flash_attn_varlen_bidir_calls_the_bidir_library_forward_and_backward(rec):
    from flash_attention_minitorch_amd import device_ops as dev
    Tq, Tk, H, Hkv, d = 300, 200, 4, 2, 64
    q, k, v = (t.requires_grad_() for t in _qkv(Tq, Tk, H, Hkv, d))
    cq, ck = _cu(0, 100, 100, 300), _cu(0, 0, 150, 200)
    rec.reset(dict(q=q, k=k, v=v, cq=cq, ck=ck))
    o = dev.flash_attn_varlen_bidir(q, k, v, cq, ck)
    assert rec.calls == [f"fa_mi355x_fwd_bidir_workspace_bytes(3,{Tq},{Tk},{H},{Hkv},{d})",
                         f"fa_mi355x_fwd_bidir(q,k,v,new0,new1,cq,ck,new2,3,{Tq},{Tk},{H},{Hkv},{d},0.0,1,null)"], rec.calls
    assert o.shape == q.shape and o.dtype.is_floating_point and o.element_size() == 4
    o.sum().backward()
    assert rec.calls[2] == f"fa_mi355x_bwd_bidir_workspace_bytes(3,{Tq},{Tk},{H},{Hkv},{d})"
    assert re.fullmatch(rf"fa_mi355x_bwd_bidir\(q,k,v,new0,new\d,new\d,new\d,new\d,new1,cq,ck,new\d,3,{Tq},{Tk},{H},{Hkv},{d},0.0,1,null\)",
                        rec.calls[3]), rec.calls
    assert len(rec.calls) == 4
    assert q.grad.shape == q.shape and q.grad.dtype == q.dtype and k.grad.shape == k.shape and v.grad.dtype == v.dtype
    # a softmax_scale reaches the library; fp32 is dtype 0
    rec.reset(dict(q=q, k=k, v=v, cq=cq, ck=ck))
    dev.flash_attn_varlen_bidir(q, k, v, cq, ck, 0.25)
    assert rec.calls[1] == f"fa_mi355x_fwd_bidir(q,k,v,new0,new1,cq,ck,new2,3,{Tq},{Tk},{H},{Hkv},{d},0.25,1,null)", rec.calls
    qf, kf, vf = (t.detach().float() for t in (q, k, v))
    rec.reset(dict(q=qf, k=kf, v=vf, cq=cq, ck=ck))
    dev.flash_attn_varlen_bidir(qf, kf, vf, cq, ck)
    assert rec.calls[1].endswith(f",3,{Tq},{Tk},{H},{Hkv},{d},0.0,0,null)"), rec.calls


def test_cu_seqlens_k_none_is_self_attention_on_one_array(rec):
    from flash_attention_minitorch_amd import device_ops as dev
    T, H, Hkv, d = 300, 4, 1, 128
    q, k, v = (t.requires_grad_() for t in _qkv(T, T, H, Hkv, d))
    cu = _cu(0, 100, 300)
    rec.reset(dict(q=q, k=k, v=v, cu=cu))
    o = dev.flash_attn_varlen_bidir(q, k, v, cu)
    o.sum().backward()
    assert rec.calls[:2] == [f"fa_mi355x_fwd_bidir_workspace_bytes(2,{T},{T},{H},{Hkv},{d})",
                             f"fa_mi355x_fwd_bidir(q,k,v,new0,new1,cu,cu,new2,2,{T},{T},{H},{Hkv},{d},0.0,1,null)"], rec.calls
    assert rec.calls[2] == f"fa_mi355x_bwd_bidir_workspace_bytes(2,{T},{T},{H},{Hkv},{d})"
    assert re.fullmatch(rf"fa_mi355x_bwd_bidir\(q,k,v,new0,new\d,new\d,new\d,new\d,new1,cu,cu,new\d,2,{T},{T},{H},{Hkv},{d},0.0,1,null\)",
                        rec.calls[3]) and len(rec.calls) == 4, rec.calls


def test_a_head_dim_of_80_runs_through_zero_padded_columns(rec):
    from flash_attention_minitorch_amd import device_ops as dev
    Tq, Tk, H, Hkv, d = 300, 200, 4, 2, 80
    q, k, v = (t.requires_grad_() for t in _qkv(Tq, Tk, H, Hkv, d))
    cq, ck = _cu(0, 100, 300), _cu(0, 150, 200)
    rec.reset(dict(cq=cq, ck=ck))
    o = dev.flash_attn_varlen_bidir(q, k, v, cq, ck)
    assert o.shape == (Tq, H, d)
    assert rec.calls[1] == f"fa_mi355x_fwd_bidir(new0,new1,new2,new3,new4,cq,ck,new5,2,{Tq},{Tk},{H},{Hkv},128,{80 ** -0.5!r},1,null)", rec.calls
    o.sum().backward()
    assert [c.split("(")[0] for c in rec.calls if "bytes" not in c] == ["fa_mi355x_fwd_bidir", "fa_mi355x_bwd_bidir"]
    assert f",cq,ck,new" in rec.calls[-1] and rec.calls[-1].endswith(f",2,{Tq},{Tk},{H},{Hkv},128,{80 ** -0.5!r},1,null)")
    assert q.grad.shape == q.shape and k.grad.shape == k.shape and q.grad.dtype == q.dtype


def test_flash_attn_cross_views_the_batch_as_packed_and_builds_both_arrays(rec):
    import torch
    from flash_attention_minitorch_amd import device_ops as dev
    B, Nq, Nk, H, Hkv, d = 3, 50, 70, 4, 2, 64
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn((B, n, h, d), generator=g).bfloat16().requires_grad_() for n, h in ((Nq, H), (Nk, Hkv), (Nk, Hkv)))
    rec.reset(dict(q=q, k=k, v=v))
    o = dev.flash_attn_cross(q, k, v, 0.5)
    assert o.shape == (B, Nq, H, d) and o.dtype == torch.float32
    assert rec.calls == [f"fa_mi355x_fwd_bidir_workspace_bytes({B},{B * Nq},{B * Nk},{H},{Hkv},{d})",
                         f"fa_mi355x_fwd_bidir(q,k,v,new0,new1,new2,new3,new4,{B},{B * Nq},{B * Nk},{H},{Hkv},{d},0.5,1,null)"], rec.calls
    cu = [t for t in rec.alive if t.dtype == torch.int32]   # the two arrays whose addresses the call took
    assert [t.tolist() for t in cu[:2]] == [[0, 50, 100, 150], [0, 70, 140, 210]]
    o.sum().backward()
    assert rec.calls[3].startswith("fa_mi355x_bwd_bidir(q,k,v,new0,") and f",new1,new2,new3,new" in rec.calls[3] and len(rec.calls) == 4
    assert q.grad.shape == q.shape and k.grad.shape == k.shape and v.grad.shape == v.shape


@pytest.mark.parametrize("Hkv", [4, 2])
def test_the_encoder_stack_rotates_first_and_makes_one_attention_call_per_layer(rec, Hkv):
    import torch
    from flash_attention_minitorch_amd import modules_transformer as mt
    T, H, d, L = 300, 4, 64, 3
    g = torch.Generator().manual_seed(1)
    x = torch.randn((T, H * d), generator=g).to(torch.bfloat16)
    wq, wk = (torch.randn(s, generator=g).to(torch.bfloat16) / 16 for s in ((H * d, H * d), (H * d, Hkv * d)))
    layers = [(wq, wk, wk, wq)] * L
    rope = mt.Rotary(*(torch.zeros(T, d // 4) for _ in range(2)))
    cu = _cu(0, 100, 300)
    rec.reset(dict(cu=cu, cos=rope.cos, sin=rope.sin))
    xg = x.clone().requires_grad_()
    y = mt.encoder_stack_packed(xg, cu, layers, H, rope=rope)
    assert y.shape == x.shape
    names = [c.split("(")[0] for c in rec.calls if "bytes" not in c]
    assert names == ["fa_mi355x_rope_varlen", "fa_mi355x_rope_varlen", "fa_mi355x_fwd_bidir"] * L   # the rotation comes first
    y.sum().backward()
    calls = [c for c in rec.calls if "bytes" not in c]
    names = [c.split("(")[0] for c in calls]
    assert sorted(names[3 * L:]) == sorted(["fa_mi355x_rope_varlen", "fa_mi355x_rope_varlen", "fa_mi355x_bwd_bidir"] * L), names
    for c in calls:   # every call takes THE cu_seqlens tensor, for both sides, and its shapes
        if c.startswith("fa_mi355x_rope_varlen("):
            heads = re.fullmatch(rf"fa_mi355x_rope_varlen\(\w+,\w+,cos,sin,cu,2,{T},(\d+),{d},{d // 2},{T},0,([01]),1,null\)", c)
            assert heads and int(heads.group(1)) in (H, Hkv), c
        else:
            assert ",cu,cu,new" in c and c.endswith(f",2,{T},{T},{H},{Hkv},{d},0.0,1,null)"), c
    assert xg.grad is not None and xg.grad.shape == x.shape
    # without rope: the attention call alone
    rec.reset(dict(cu=cu))
    mt.multi_head_attention_packed_bidir(x, cu, wq, wk, wk, wq, H)
    assert [c.split("(")[0] for c in rec.calls if "bytes" not in c] == ["fa_mi355x_fwd_bidir"]


@pytest.mark.parametrize("Hkv", [4, 1])
def test_cross_attention_packed_reads_grouped_memory_weights_and_hands_over_both_arrays(rec, Hkv):
    import torch
    from flash_attention_minitorch_amd import modules_transformer as mt
    Tq, Tk, H, d, Em = 300, 200, 4, 64, 96
    g = torch.Generator().manual_seed(2)
    x, mem = (torch.randn(s, generator=g).to(torch.bfloat16).requires_grad_() for s in ((Tq, H * d), (Tk, Em)))
    wq, wk, wv = (torch.randn(s, generator=g).to(torch.bfloat16) / 16 for s in ((H * d, H * d), (Em, Hkv * d), (Em, Hkv * d)))
    cq, ck = _cu(0, 100, 300), _cu(0, 150, 200)
    rec.reset(dict(cq=cq, ck=ck))
    y = mt.cross_attention_packed(x, cq, mem, ck, wq, wk, wv, wq, H)
    assert y.shape == (Tq, H * d) and y.dtype == x.dtype
    calls = [c for c in rec.calls if "bytes" not in c]
    assert len(calls) == 1 and ",cq,ck,new" in calls[0] and calls[0].endswith(f",2,{Tq},{Tk},{H},{Hkv},{d},0.0,1,null)"), rec.calls
    y.sum().backward()
    assert [c.split("(")[0] for c in rec.calls if "bytes" not in c] == ["fa_mi355x_fwd_bidir", "fa_mi355x_bwd_bidir"]
    assert x.grad.shape == x.shape and mem.grad.shape == mem.shape
    with pytest.raises(ValueError, match="Hkv a divisor"):
        mt.cross_attention_packed(x, cq, mem, ck, wq, torch.zeros(Em, 3 * d).bfloat16(), torch.zeros(Em, 3 * d).bfloat16(), wq, H)
