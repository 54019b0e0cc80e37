"""Packed attention under a two-sided sliding window with separate cu_seqlens for q and k (include/flash_attn_mi355x_local.h,
libflash_attn_mi355x_local.so), the checks that need no GPU: the C ABI against _lib.LOCAL_ABI, every argument error of
tests/test_bidir_cpu.py's lists and the window's before any HIP call, the workspace formula (the bidirectional library's), the
library's kernels (no scratch, names of their own), the Python checks and the routing of the windows that are existing calls under
the recorder of tests/test_device_ops_cpu.py, and the fp64 band reference the GPU tests use, pinned three ways."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
from test_abi_cpu import ROOT, _device_kernels, built  # noqa: F401  (built: the module-scoped build fixture)
from test_bidir_cpu import _BAD, _BAD_BWD, _GOOD, QBLOCK, _align, _cu, _qkv, key_block
from test_varlen_cpu import seq_rows

HEADER = "flash_attn_mi355x_local.h"
SYMBOLS = ["fa_mi355x_fwd_local", "fa_mi355x_bwd_local", "fa_mi355x_fwd_local_workspace_bytes", "fa_mi355x_bwd_local_workspace_bytes",
           "fa_mi355x_local_last_error"]


# ---- the fp64 band reference (tests/test_gpu_local.py runs the kernels against it) ----

def local_admit(nq, nk, L, R):
    """(nq, nk) bool: row i, at key position p = i + nk - nq, admits key j iff (L < 0 or j >= p - L) and (R < 0 or j <= p + R)."""
    p, j = np.arange(nq)[:, None] + (nk - nq), np.arange(nk)[None, :]
    return ((j >= p - L) if L >= 0 else np.ones((nq, nk), bool)) & ((j <= p + R) if R >= 0 else np.ones((nq, nk), bool))


def _masked_attention(q, k, v, do, admit, tau):
    """Dense masked softmax attention and its gradient in fp64 for heads-first arrays q, do (H, nq, d), k, v (H, nk, d): out, lse
    (H, nq), dq, dk, dv.  A row that admits no key is zeros in out, lse and dq and adds nothing to dk, dv."""
    some = admit.any(1)[None, :, None]
    s = np.where(admit[None], tau * q @ k.swapaxes(-1, -2), -np.inf)
    mx = np.where(some, s.max(-1, keepdims=True), 0.0)
    e = np.exp(s - mx)
    l = np.where(some, e.sum(-1, keepdims=True), 1.0)
    p = e / l
    o = p @ v
    ds = p * (do @ v.swapaxes(-1, -2) - (do * o).sum(-1, keepdims=True))
    lse = np.where(some, mx + np.log(l), 0.0)[..., 0]
    return o, lse, tau * ds @ k, tau * ds.swapaxes(-1, -2) @ q, p.swapaxes(-1, -2) @ do


def local_reference(q, k, v, do, cu_q, Tq, cu_k, Tk, L, R, scale=None):
    """The fp64 reference per sequence and head: out (Tq, H, d), lse (H, Tq), dq, dk (Tk, Hkv, d), dv; zeros in the rows that admit
    no key, the keys no row admits and the rows no sequence owns.  ``scale``: the caller's softmax_scale (None: 1 / sqrt(d))."""
    H, Hkv, d = q.shape[1], k.shape[1], q.shape[2]
    G, tau = H // Hkv, 1.0 / math.sqrt(d) if scale is None else float(scale)
    out, dq, lse = np.zeros((Tq, H, d)), np.zeros((Tq, H, d)), np.zeros((H, Tq))
    dk, dv = np.zeros((Tk, Hkv, d)), np.zeros((Tk, Hkv, d))
    for (sq, nq), (sk, nk) in zip(seq_rows(cu_q, Tq), seq_rows(cu_k, Tk)):
        if nq == 0 or nk == 0:
            continue
        hq, hdo = (a[sq:sq + nq].transpose(1, 0, 2).astype(np.float64) for a in (q, do))
        hk, hv = (np.repeat(a[sk:sk + nk].transpose(1, 0, 2), G, 0).astype(np.float64) for a in (k, v))
        ro, rl, rdq, rdk, rdv = _masked_attention(hq, hk, hv, hdo, local_admit(nq, nk, L, R), tau)
        out[sq:sq + nq], dq[sq:sq + nq], lse[:, sq:sq + nq] = ro.transpose(1, 0, 2), rdq.transpose(1, 0, 2), rl
        dk[sk:sk + nk], dv[sk:sk + nk] = (a.reshape(Hkv, G, nk, d).sum(1).transpose(1, 0, 2) for a in (rdk, rdv))
    return out, lse, dq, dk, dv


def local_live(cu_q, Tq, cu_k, Tk, L, R):
    """(rows of the q buffers, rows of the k buffers) that carry a result: a query row that admits a key, a key some row admits."""
    lq, lk = np.zeros(Tq, bool), np.zeros(Tk, bool)
    for (sq, nq), (sk, nk) in zip(seq_rows(cu_q, Tq), seq_rows(cu_k, Tk)):
        if nq and nk:
            admit = local_admit(nq, nk, L, R)
            lq[sq:sq + nq], lk[sk:sk + nk] = admit.any(1), admit.any(0)
    return lq, lk


def _problem(rng, lens_q, lens_k, H, Hkv, d):
    cu_q, cu_k = (np.concatenate([[0], np.cumsum(n)]) for n in (lens_q, lens_k))
    Tq, Tk = int(cu_q[-1]), int(cu_k[-1])
    q, do = (rng.uniform(-1, 1, (Tq, H, d)) for _ in range(2))
    k, v = (rng.uniform(-1, 1, (Tk, Hkv, d)) for _ in range(2))
    return q, k, v, do, cu_q, Tq, cu_k, Tk


def test_the_admit_rule_and_its_special_cases():
    for nq, nk in ((5, 9), (9, 5), (7, 7), (1, 12), (12, 1)):
        D = nk - nq
        i, j = np.arange(nq)[:, None], np.arange(nk)[None, :]
        assert local_admit(nq, nk, -1, -1).all()
        assert np.array_equal(local_admit(nq, nk, -1, 0), j <= i + D)                       # the causal two-array mask
        assert np.array_equal(local_admit(nq, nk, 0, 0), j == i + D)                        # exactly key p
        assert np.array_equal(local_admit(nq, nk, 2, 0), (j <= i + D) & (j > i + D - 3))    # a causal window of W = 3 positions
        assert np.array_equal(local_admit(nq, nk, nk, -1), local_admit(nq, nk, -1, -1))     # a left bound >= n_k: unbounded
        assert np.array_equal(local_admit(nq, nk, -1, nk + nq), local_admit(nq, nk, -1, -1))
        empty_rows = ~local_admit(nq, nk, 3, 1).any(1)
        assert np.array_equal(empty_rows, np.arange(nq) + D + 1 < 0)                        # p + R < 0
        dead_keys = ~local_admit(nq, nk, 3, 1).any(0)
        assert np.array_equal(dead_keys, np.arange(nk) < D - 3)                             # j < D - L


def test_the_reference_is_the_oracle_where_the_window_is_an_existing_mask():
    rng = np.random.default_rng(0)
    q, k, v, do, cu_q, Tq, cu_k, Tk = _problem(rng, [17, 40, 3], [33, 8, 3], 4, 2, 16)
    got = local_reference(q, k, v, do, cu_q, Tq, cu_k, Tk, -1, -1)
    for b in range(3):
        qs, ks = slice(cu_q[b], cu_q[b + 1]), slice(cu_k[b], cu_k[b + 1])
        hq, hdo = (a[qs].transpose(1, 0, 2) for a in (q, do))
        hk, hv = (np.repeat(a[ks].transpose(1, 0, 2), 2, 0) for a in (k, v))
        ro, rl, _, _ = oracle.dense_attention_fw(hq, hk, hv, causal=False)
        rdq, rdk, rdv = oracle.dense_attention_bw(hq, hk, hv, hdo, causal=False)
        rdk, rdv = (a.reshape(2, 2, -1, 16).sum(1).transpose(1, 0, 2) for a in (rdk, rdv))
        want = (ro.transpose(1, 0, 2), rl.T, rdq.transpose(1, 0, 2), rdk, rdv)
        for g, w, rows in zip(got, want, (qs, qs, qs, ks, ks)):
            g = g.T[rows] if g.shape == (4, Tq) else g[rows]
            assert np.max(np.abs(g - w)) < 1e-9
    # (-1, 0) on one array: the oracle's causal mask
    q, k, v, do, cu, T, _, _ = _problem(rng, [29, 1, 50], [29, 1, 50], 4, 4, 8)
    got = local_reference(q, k, v, do, cu, T, cu, T, -1, 0)
    for b in range(3):
        rows = slice(cu[b], cu[b + 1])
        hq, hk, hv, hdo = (a[rows].transpose(1, 0, 2) for a in (q, k, v, do))
        ro, rl, _, _ = oracle.dense_attention_fw(hq, hk, hv, causal=True)
        rdq, rdk, rdv = oracle.dense_attention_bw(hq, hk, hv, hdo, causal=True)
        want = (ro.transpose(1, 0, 2), rl.T, rdq.transpose(1, 0, 2), rdk.transpose(1, 0, 2), rdv.transpose(1, 0, 2))
        for g, w in zip(got, want):
            g = g.T[rows] if g.shape == (4, T) else g[rows]
            assert np.max(np.abs(g - w)) < 1e-9


@pytest.mark.parametrize("L,R", [(2, 1), (0, 0), (-1, 3), (4, -1), (0, 5), (30, 30)])
def test_the_reference_is_a_per_row_loop_that_applies_the_admit_rule_literally(L, R):
    rng = np.random.default_rng((L + 1) * 100 + R + 1)
    H, Hkv, d = 2, 1, 8
    q, k, v, do, cu_q, Tq, cu_k, Tk = _problem(rng, [6, 11, 4, 0, 3], [13, 4, 4, 5, 0], H, Hkv, d)
    got = local_reference(q, k, v, do, cu_q, Tq, cu_k, Tk, L, R)
    out, dq, lse = np.zeros((Tq, H, d)), np.zeros((Tq, H, d)), np.zeros((H, Tq))
    dk, dv = np.zeros((Tk, Hkv, d)), np.zeros((Tk, Hkv, d))
    tau = 1.0 / math.sqrt(d)
    for b in range(len(cu_q) - 1):
        (sq, nq), (sk, nk) = (int(cu_q[b]), int(cu_q[b + 1] - cu_q[b])), (int(cu_k[b]), int(cu_k[b + 1] - cu_k[b]))
        for h in range(H):
            for i in range(nq):
                p = i + nk - nq
                keys = [j for j in range(nk) if 0 <= j < nk and (L < 0 or j >= p - L) and (R < 0 or j <= p + R)]
                if not keys:
                    continue
                s = np.array([tau * q[sq + i, h] @ k[sk + j, h // 2] for j in keys])
                m = s.max()
                l = np.exp(s - m).sum()
                pr = np.exp(s - m) / l
                o = sum(pj * v[sk + j, h // 2] for pj, j in zip(pr, keys))
                out[sq + i, h], lse[h, sq + i] = o, m + math.log(l)
                delta = do[sq + i, h] @ o
                for pj, j in zip(pr, keys):
                    ds = pj * (do[sq + i, h] @ v[sk + j, h // 2] - delta)
                    dq[sq + i, h] += tau * ds * k[sk + j, h // 2]
                    dk[sk + j, h // 2] += tau * ds * q[sq + i, h]
                    dv[sk + j, h // 2] += pj * do[sq + i, h]
    for g, w in zip(got, (out, lse, dq, dk, dv)):
        assert np.max(np.abs(g - w)) < 1e-9
    lq, lk = local_live(cu_q, Tq, cu_k, Tk, L, R)
    assert not got[0][~lq].any() and not got[1][:, ~lq].any() and not got[2][~lq].any() and not got[3][~lk].any() and not got[4][~lk].any()


def test_the_references_gradient_is_the_central_finite_difference_of_its_forward():
    rng = np.random.default_rng(7)
    H, d, L, R = 1, 4, 2, 1
    q, k, v, do, cu_q, Tq, cu_k, Tk = _problem(rng, [5], [9], H, H, d)
    _, _, dq, dk, dv = local_reference(q, k, v, do, cu_q, Tq, cu_k, Tk, L, R)
    loss = lambda q, k, v: float((local_reference(q, k, v, do, cu_q, Tq, cu_k, Tk, L, R)[0] * do).sum())
    eps = 1e-5
    for which, (x, g) in enumerate(((q, dq), (k, dk), (v, dv))):
        num = np.zeros_like(x)
        for idx in np.ndindex(*x.shape):
            hi, lo = x.copy(), x.copy()
            hi[idx] += eps
            lo[idx] -= eps
            args = [q, k, v]
            args[which] = hi
            up = loss(*args)
            args[which] = lo
            num[idx] = (up - loss(*args)) / (2 * eps)
        assert np.max(np.abs(num - g)) < 1e-6, which
    assert not dk[:9 - 5 - L].any() and dk[9 - 5 - L].any()   # the keys j < D - L are admitted by no row


# ---- the C ABI ----

def test_header_declares_what_the_abi_table_binds_and_the_library_exports(built):
    from test_lib_cpu import _ctypes_kind, _prototypes
    raw = open(os.path.join(ROOT, "include", HEADER)).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert sorted(set(re.findall(r"\b(fa_mi355x_\w+)\s*\(", text))) == sorted(SYMBOLS) == sorted(built.LOCAL_ABI)
    for other in os.listdir(os.path.join(ROOT, "include")):   # no other header gained a declaration
        if other != HEADER:
            assert not re.search(r"fa_mi355x_\w*local", open(os.path.join(ROOT, "include", other)).read()), other
    for said in ("(L < 0 or j >= p - L)", "(R < 0 or j <= p + R)", "bottom-right", "a row that admits no key", "a key that no row admits",
                 "rows no sequence owns", "bit\n * for bit", "Not built", "sinks or a logit cap beside the band", "MFMA-slot", "key mask",
                 "fp8", "rotary offsets", "host-pointer reference ABI", "longest-first", "KV-cache library"):
        assert said in raw, said
    protos = _prototypes(HEADER)
    lib = built.local()
    exported = subprocess.run(["nm", "-D", "--defined-only", built.lib_path(built.LOCAL_NAME)], capture_output=True, text=True, check=True).stdout
    assert sorted(re.findall(r" T (fa_mi355x_\w+)\n", exported)) == sorted(SYMBOLS)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        res, args = built.LOCAL_ABI[s]
        ret, kinds = protos[s]
        assert [_ctypes_kind(a) for a in args] == kinds and _ctypes_kind(res) == ret, s
        assert getattr(lib, s).argtypes == args and getattr(lib, s).restype is res, s
    for s in ("fa_mi355x_fwd_local", "fa_mi355x_bwd_local"):   # the bidirectional prototypes with the two ints behind softmax_scale
        twin = built.BIDIR_ABI[s.replace("local", "bidir")][1]
        assert built.LOCAL_ABI[s][1] == twin[:-2] + [ctypes.c_int, ctypes.c_int] + twin[-2:], s
    needed = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "-d", built.lib_path(built.LOCAL_NAME)], capture_output=True,
                            text=True, check=True).stdout
    assert "libflash_attn_mi355x" not in needed   # a library of its own: it loads without the other six


def _call(lib, bwd, **over):
    a = dict(dict(_GOOD, wl=5, wr=9), **over)
    p = lambda n: ctypes.c_void_p(a[n]) if a[n] else None
    tail = (p("cu_q"), p("cu_k"), p("ws"), a["nseq"], a["Tq"], a["Tk"], a["H"], a["Hkv"], a["d"], a["scale"], a["wl"], a["wr"],
            a["dtype"], None)
    if bwd:
        rc = lib.fa_mi355x_bwd_local(p("q"), p("k"), p("v"), p("out"), p("dout"), p("dq"), p("dk"), p("dv"), p("lse"), *tail)
    else:
        rc = lib.fa_mi355x_fwd_local(p("q"), p("k"), p("v"), p("out"), p("lse"), *tail)
    return rc, lib.fa_mi355x_local_last_error().decode()


_BAD_WINDOW = [(dict(wl=-2), "window_left must be -1 (unbounded) or >= 0"), (dict(wr=-2), "window_right must be -1 (unbounded) or >= 0"),
               (dict(wl=-(1 << 31)), "window_left"), (dict(wl=-1, wr=-7), "window_right")]


@pytest.mark.parametrize("bwd,over,msg", [(b, o, m) for b in (False, True) for o, m in _BAD + _BAD_WINDOW] + [(True, o, m) for o, m in _BAD_BWD],
                         ids=lambda x: "-".join(f"{k}={v}" for k, v in x.items()) if isinstance(x, dict) else None)
def test_each_bad_argument_is_rejected_before_any_hip_call(built, bwd, over, msg):
    """The local library alone, no GPU: FA_ERR_BAD_ARG = 1 and the bidirectional library's message (the window's own for a side below
    -1); the fake pointers would make any launch fail with FA_ERR_HIP = 3.  A call that passes the checks must not be made here."""
    rc, err = _call(built.local(), bwd, **over)
    assert rc == 1 and msg in err, (rc, err)


def test_workspace_bytes_are_the_headers_formula_and_the_bidirectional_librarys(built):
    fwd, bwd = built.local().fa_mi355x_fwd_local_workspace_bytes, built.local().fa_mi355x_bwd_local_workspace_bytes
    bfwd, bbwd = built.bidir().fa_mi355x_fwd_bidir_workspace_bytes, built.bidir().fa_mi355x_bwd_bidir_workspace_bytes
    pfwd, pbwd = built.prefix().fa_mi355x_fwd_prefix_workspace_bytes, built.prefix().fa_mi355x_bwd_prefix_workspace_bytes
    for nseq, Tq, Tk, H, Hkv, d in ((1, 1, 1, 1, 1, 32), (7, 612, 622, 4, 4, 64), (7, 612, 622, 4, 2, 64), (40, 552, 1080, 4, 1, 128),
                                    (1, 300, 700, 4, 2, 32), (8, 2048, 65536, 32, 8, 128), (256, 32768, 32768, 32, 32, 128)):
        mq, mk = (_align(32 * (T // QBLOCK + nseq)) for T in (Tq, Tk))
        assert fwd(nseq, Tq, Tk, H, Hkv, d) == mq == bfwd(nseq, Tq, Tk, H, Hkv, d) == pfwd(nseq, Tq, Tk, H, Hkv, d)
        vecs = 3 * H * Tq * 4
        assert bwd(nseq, Tq, Tk, H, Hkv, d) == (mq + mk + vecs if Hkv == H else mq + mk + _align(vecs) + 2 * H * Tk * d * 4)
        assert bwd(nseq, Tq, Tk, H, Hkv, d) == bbwd(nseq, Tq, Tk, H, Hkv, d) == pbwd(nseq, Tq, Tk, H, Hkv, d)
        for dt, dd in ((True, 32), (True, 64), (True, 128), (False, 64)):   # every build's key-block map fits the MAP(Tk) it is given
            assert 32 * (Tk // key_block(dt, dd) + nseq) <= mk
    for f in (fwd, bwd):
        assert (f(0, 100, 100, 4, 2, 64) == f(2, 0, 100, 4, 2, 64) == f(2, 100, 0, 4, 2, 64) == f(2, 100, 100, 0, 2, 64)
                == f(2, 100, 100, 4, 3, 64) == f(2, 100, 100, 4, 0, 64) == f(2, 100, 100, 4, 2, 0) == 0)
        assert f(-1, 100, 100, 4, 2, 64) == f(2, -5, 100, 4, 2, 64) == f(2, 100, -5, 4, 2, 64) == 0


# ---- the kernels ----

def test_every_kernel_of_the_local_library_has_no_scratch_and_a_name_of_its_own(built):
    kernels = _device_kernels(built.lib_path(built.LOCAL_NAME))
    names = [k[0] for k in kernels]
    for stem in ("local_fwd_kernel", "local_dq_kernel", "local_dkdv_kernel", "bwd_prep_kernel"):
        assert sum(stem in n for n in names) == 6, (stem, names)   # bf16 and fp32 at d = 32, 64, 128
    assert sum("bidir_schedule_kernel" in n for n in names) == 1 and sum("group_sum_kernel" in n for n in names) == 1
    # no kernel of another library: what is left is mfma_peak_kernel, which comes along with fa_aux.h and is not launched
    stems = ("local_fwd_kernel", "local_dq_kernel", "local_dkdv_kernel", "bidir_schedule_kernel", "bwd_prep_kernel", "group_sum_kernel")
    assert [n for n in names if not any(s in n for s in stems)] == [n for n in names if "mfma_peak_kernel" in n]
    assert not [n for n in names if "bidir_fwd" in n or "bidir_dq" in n or "bidir_dkdv" in n or "prefix_" in n or "win_" in n or "varlen_" in n]
    assert len(names) == 27, names
    for name, scratch, vgpr in kernels:
        assert scratch == 0, (name, scratch)
        assert vgpr <= 512, (name, vgpr)
    for other in (built.BIDIR_NAME, built.PREFIX_NAME):   # ... and no other library gained one of these
        assert not [k[0] for k in _device_kernels(built.lib_path(other)) if "local_" in k[0]], other


# ---- Python: the checks, and the calls under the recorder ----

@pytest.fixture
def rec(monkeypatch):
    from flash_attention_minitorch_amd import _lib
    from test_device_ops_cpu import install_recorder
    r = install_recorder(monkeypatch)
    for lib in ("local", "bidir", "prefix"):
        for sym in (f"fa_mi355x_fwd_{lib}_workspace_bytes", f"fa_mi355x_bwd_{lib}_workspace_bytes"):
            log = getattr(r, sym)
            r.__dict__[sym] = lambda *a, log=log: log(*a) or 4096   # (logged like the others, with a size)
        monkeypatch.setattr(_lib, lib, lambda: r)
    return r


def _names(rec):
    return [c.split("(")[0] for c in rec.calls if "bytes" not in c]


def test_python_checks_raise_before_any_launch(rec):
    import torch
    from flash_attention_minitorch_amd import device_ops as dev
    q, k, v = _qkv()
    cq, ck = _cu(0, 100, 300), _cu(0, 150, 200)
    o, lse = q.float(), q.float()[..., 0].transpose(0, 1).contiguous()
    for bad in ((5,), (5, 9, 1), 5, "59", (5.0, 9), (True, 9), (-2, 9), (5, -2), ("5", 9), (5, 2.5), torch.tensor([5, 9])):
        with pytest.raises(ValueError, match="window must be a pair"):
            dev.flash_attn_varlen_local_fwd(q, k, v, cq, ck, bad)
        with pytest.raises(ValueError, match="window must be a pair"):
            dev.flash_attn_varlen_local_bwd(q, k, v, o, q, lse, cq, ck, bad)
        with pytest.raises(ValueError, match="window must be a pair"):
            dev.flash_attn_varlen_local(q, k, v, cq, ck, bad)
        with pytest.raises(ValueError, match="window must be a pair"):
            dev.flash_attn_local(q[None], k[None], v[None], bad)
    with pytest.raises(ValueError, match="native head dim.*flash_attn_varlen_local pads"):
        dev.flash_attn_varlen_local_fwd(*_qkv(d=80), cq, ck, (5, 9))
    with pytest.raises(ValueError, match="multiple"):
        dev.flash_attn_varlen_local_fwd(*_qkv(H=4, Hkv=3), cq, ck, (5, 9))
    with pytest.raises(ValueError, match="3-d"):
        dev.flash_attn_varlen_local_fwd(q[None], k[None], v[None], cq, ck, (5, 9))
    with pytest.raises(ValueError, match="one dtype"):
        dev.flash_attn_varlen_local_fwd(q, k.float(), v.float(), cq, ck, (5, 9))
    with pytest.raises(ValueError, match="self-attention: k must have q's 300 rows"):
        dev.flash_attn_varlen_local_fwd(q, k, v, cq, None, (5, 9))
    with pytest.raises(ValueError, match="one length"):
        dev.flash_attn_varlen_local_fwd(q, k, v, cq, _cu(0, 50, 150, 200), (5, 9))
    for bad in (cq.long(), cq[:1], [0, 100, 300]):
        with pytest.raises(ValueError, match="cu_seqlens"):
            dev.flash_attn_varlen_local_fwd(q, k, v, bad, ck, (5, 9))
    with pytest.raises(ValueError, match="out_grad"):
        dev.flash_attn_varlen_local_bwd(q, k, v, o, k, lse, cq, ck, (5, 9))
    with pytest.raises(ValueError, match="lse"):
        dev.flash_attn_varlen_local_bwd(q, k, v, o, q, lse[:, :10], cq, ck, (5, 9))
    with pytest.raises(ValueError, match=r"workspace too small.*local_workspace\("):
        dev.flash_attn_varlen_local_bwd(q, k, v, o, q, lse, cq, ck, (5, 9), workspace=o.new_empty(16))
    with pytest.raises(ValueError, match="workspace too small"):
        dev.flash_attn_varlen_local_fwd(q, k, v, cq, ck, (5, 9), workspace=o.new_empty(16))
    with pytest.raises(ValueError, match="out must be"):
        dev.flash_attn_varlen_local_fwd(q, k, v, cq, ck, (5, 9), out=q)
    with pytest.raises(ValueError, match="grads"):
        dev.flash_attn_varlen_local_bwd(q, k, v, o, q, lse, cq, ck, (5, 9), grads=(o, o[:10], o))
    q4, k4 = torch.zeros(2, 5, 4, 64).bfloat16(), torch.zeros(2, 7, 2, 64).bfloat16()
    with pytest.raises(ValueError, match="flash_attn_local expects 4-d"):
        dev.flash_attn_local(q, k, v, (5, 9))
    with pytest.raises(ValueError, match="disagree on the batch"):
        dev.flash_attn_local(q4, k4[:1].contiguous(), k4[:1].contiguous(), (5, 9))
    assert not _names(rec), rec.calls


def test_a_window_calls_the_local_library_with_both_sides_behind_softmax_scale(rec):
    from flash_attention_minitorch_amd import device_ops as dev
    Tq, Tk, H, Hkv, d = 300, 200, 4, 2, 64
    q, k, v = (t.requires_grad_() for t in _qkv(Tq, Tk, H, Hkv, d))
    cq, ck = _cu(0, 100, 100, 300), _cu(0, 0, 150, 200)
    rec.reset(dict(q=q, k=k, v=v, cq=cq, ck=ck))
    o = dev.flash_attn_varlen_local(q, k, v, cq, ck, (5, 9))
    assert rec.calls == [f"fa_mi355x_fwd_local_workspace_bytes(3,{Tq},{Tk},{H},{Hkv},{d})",
                         f"fa_mi355x_fwd_local(q,k,v,new0,new1,cq,ck,new2,3,{Tq},{Tk},{H},{Hkv},{d},0.0,5,9,1,null)"], rec.calls
    assert o.shape == q.shape and o.element_size() == 4
    o.sum().backward()
    assert rec.calls[2] == f"fa_mi355x_bwd_local_workspace_bytes(3,{Tq},{Tk},{H},{Hkv},{d})"
    assert re.fullmatch(rf"fa_mi355x_bwd_local\(q,k,v,new0,new\d,new\d,new\d,new\d,new1,cq,ck,new\d,3,{Tq},{Tk},{H},{Hkv},{d},0.0,5,9,1,null\)",
                        rec.calls[3]), rec.calls
    assert len(rec.calls) == 4
    assert q.grad.shape == q.shape and q.grad.dtype == q.dtype and k.grad.shape == k.shape and v.grad.dtype == v.dtype
    # a softmax_scale reaches the library; one-sided forms, None for a side; fp32 is dtype 0; one array for both
    for window, sides in (((None, 17), "-1,17"), ((40, -1), "40,-1"), ([0, 0], "0,0"), ((np.int64(3), 1000000), "3,1000000")):
        rec.reset(dict(q=q, k=k, v=v, cq=cq, ck=ck))
        dev.flash_attn_varlen_local(q, k, v, cq, ck, window, 0.25)
        assert rec.calls[1] == f"fa_mi355x_fwd_local(q,k,v,new0,new1,cq,ck,new2,3,{Tq},{Tk},{H},{Hkv},{d},0.25,{sides},1,null)", rec.calls
    qf, kf, vf = _qkv(Tq, Tq, H, Hkv, d, dtype=q.float().dtype)
    rec.reset(dict(q=qf, k=kf, v=vf, cq=cq))
    dev.flash_attn_varlen_local_fwd(qf, kf, vf, cq, window=(63, 0))
    assert rec.calls[1] == f"fa_mi355x_fwd_local(q,k,v,new0,new1,cq,cq,new2,3,{Tq},{Tq},{H},{Hkv},{d},0.0,63,0,0,null)", rec.calls


@pytest.mark.parametrize("window,lib", [((-1, -1), "bidir"), (None, "bidir"), ((None, None), "bidir"), ((-1, 0), "prefix"), ((None, 0), "prefix")])
def test_the_windows_that_are_existing_calls_make_those_calls(rec, window, lib):
    from flash_attention_minitorch_amd import device_ops as dev
    Tq, Tk, H, Hkv, d = 300, 200, 4, 2, 64
    q, k, v = (t.requires_grad_() for t in _qkv(Tq, Tk, H, Hkv, d))
    cq, ck = _cu(0, 100, 300), _cu(0, 150, 200)
    kw = dict(window=window)
    rec.reset(dict(q=q, k=k, v=v, cq=cq, ck=ck))
    o = dev.flash_attn_varlen_local(q, k, v, cq, ck, **kw)
    o.sum().backward()
    existing = getattr(dev, f"flash_attn_varlen_{lib}")
    mine = list(rec.calls)
    q.grad = k.grad = v.grad = None
    rec.reset(dict(q=q, k=k, v=v, cq=cq, ck=ck))
    existing(q, k, v, cq, ck).sum().backward()
    assert mine == rec.calls and _names(rec) == [f"fa_mi355x_fwd_{lib}", f"fa_mi355x_bwd_{lib}"], (mine, rec.calls)
    # the two halves alone, with a workspace made by local_workspace
    ws = dev.local_workspace(q, k, cq, ck)
    assert rec.calls[-1] == f"fa_mi355x_bwd_local_workspace_bytes(2,{Tq},{Tk},{H},{Hkv},{d})"
    raw = ws.new_empty(ws.numel() + 64)   # (a host tensor is not 256-byte aligned by itself)
    ws = raw[(-raw.data_ptr() % 256) // 4:][:ws.numel()]
    rec.reset(dict(q=q, k=k, v=v, cq=cq, ck=ck, ws=ws))
    with __import__("torch").no_grad():
        o, lse = dev.flash_attn_varlen_local_fwd(q, k, v, cq, ck, workspace=ws, **kw)
        dev.flash_attn_varlen_local_bwd(q, k, v, o, q, lse, cq, ck, workspace=ws, **kw)
    assert _names(rec) == [f"fa_mi355x_fwd_{lib}", f"fa_mi355x_bwd_{lib}"] and all(",cq,ck,ws," in c for c in rec.calls if "bytes" not in c)
    assert all(c.endswith(f",2,{Tq},{Tk},{H},{Hkv},{d},0.0,1,null)") for c in rec.calls if "bytes" not in c), rec.calls


def test_a_head_dim_of_80_runs_through_zero_padded_columns(rec):
    from flash_attention_minitorch_amd import device_ops as dev
    Tq, Tk, H, Hkv, d = 300, 200, 4, 2, 80
    q, k, v = (t.requires_grad_() for t in _qkv(Tq, Tk, H, Hkv, d))
    cq, ck = _cu(0, 100, 300), _cu(0, 150, 200)
    rec.reset(dict(cq=cq, ck=ck))
    o = dev.flash_attn_varlen_local(q, k, v, cq, ck, (5, 9))
    assert o.shape == (Tq, H, d)
    assert rec.calls[1] == f"fa_mi355x_fwd_local(new0,new1,new2,new3,new4,cq,ck,new5,2,{Tq},{Tk},{H},{Hkv},128,{80 ** -0.5!r},5,9,1,null)", rec.calls
    o.sum().backward()
    assert _names(rec) == ["fa_mi355x_fwd_local", "fa_mi355x_bwd_local"]
    assert ",cq,ck,new" in rec.calls[-1] and rec.calls[-1].endswith(f",2,{Tq},{Tk},{H},{Hkv},128,{80 ** -0.5!r},5,9,1,null)")
    assert q.grad.shape == q.shape and k.grad.shape == k.shape and q.grad.dtype == q.dtype


def test_flash_attn_local_views_the_batch_as_packed_and_builds_both_arrays(rec):
    import torch
    from flash_attention_minitorch_amd import device_ops as dev
    B, Nq, Nk, H, Hkv, d = 3, 50, 70, 4, 2, 64
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn((B, n, h, d), generator=g).bfloat16().requires_grad_() for n, h in ((Nq, H), (Nk, Hkv), (Nk, Hkv)))
    rec.reset(dict(q=q, k=k, v=v))
    o = dev.flash_attn_local(q, k, v, (5, 9), 0.5)
    assert o.shape == (B, Nq, H, d) and o.dtype == torch.float32
    assert rec.calls == [f"fa_mi355x_fwd_local_workspace_bytes({B},{B * Nq},{B * Nk},{H},{Hkv},{d})",
                         f"fa_mi355x_fwd_local(q,k,v,new0,new1,new2,new3,new4,{B},{B * Nq},{B * Nk},{H},{Hkv},{d},0.5,5,9,1,null)"], rec.calls
    cu = [t for t in rec.alive if t.dtype == torch.int32]   # the two arrays whose addresses the call took
    assert [t.tolist() for t in cu[:2]] == [[0, 50, 100, 150], [0, 70, 140, 210]]
    o.sum().backward()
    assert rec.calls[3].startswith("fa_mi355x_bwd_local(q,k,v,new0,") and ",new1,new2,new3,new" in rec.calls[3] and len(rec.calls) == 4
    assert rec.calls[3].endswith(",0.5,5,9,1,null)")
    assert q.grad.shape == q.shape and k.grad.shape == k.shape and v.grad.shape == v.shape


# ---- the model functions ----

def _stack(Hkv=2, n_layers=4):
    import torch
    T, H, d = 300, 4, 64
    g = torch.Generator().manual_seed(1)
    x = torch.randn((T, H * d), generator=g).to(torch.bfloat16)
    wq, wk = (torch.randn(s, generator=g).to(torch.bfloat16) / 16 for s in ((H * d, H * d), (H * d, Hkv * d)))
    return x, [(wq, wk, wk, wq)] * n_layers, _cu(0, 100, 300), (T, H, Hkv, d)


def test_the_encoder_stack_makes_one_call_per_layer_with_that_layers_window(rec):
    from flash_attention_minitorch_amd import modules_transformer as mt
    x, layers, cu, (T, H, Hkv, d) = _stack()
    tail = rf"new\d+,new\d+,new\d+,new\d+,new\d+,cu,cu,new\d+,2,{T},{T},{H},{Hkv},{d},0.0,"
    rec.reset(dict(cu=cu))
    xg = x.clone().requires_grad_()
    y = mt.encoder_stack_packed(xg, cu, layers, H, window=[(64, 64), None, (None, 128), (-1, -1)])
    assert y.shape == x.shape and y.dtype == x.dtype
    calls = [c for c in rec.calls if "bytes" not in c]
    assert [c.split("(")[0] for c in calls] == ["fa_mi355x_fwd_local", "fa_mi355x_fwd_bidir", "fa_mi355x_fwd_local", "fa_mi355x_fwd_bidir"]
    for c, sides in zip(calls, ("64,64,", "", "-1,128,", "")):
        assert re.fullmatch(rf"fa_mi355x_fwd_\w+\({tail}{sides}1,null\)", c), c
    y.sum().backward()
    assert _names(rec)[4:] == ["fa_mi355x_bwd_bidir", "fa_mi355x_bwd_local", "fa_mi355x_bwd_bidir", "fa_mi355x_bwd_local"]
    assert rec.calls[-1].endswith(",0.0,64,64,1,null)") and xg.grad.shape == x.shape
    # one pair: every layer has it
    rec.reset(dict(cu=cu))
    mt.encoder_stack_packed(x, cu, layers, H, window=(5, 9))
    assert _names(rec) == ["fa_mi355x_fwd_local"] * 4 and all(c.endswith(",0.0,5,9,1,null)") for c in rec.calls if "bytes" not in c)
    rec.reset(dict(cu=cu))
    mt.multi_head_attention_packed_bidir(x, cu, *layers[0], H, None, (0, 3))
    assert _names(rec) == ["fa_mi355x_fwd_local"] and rec.calls[-1].endswith(",0.0,0,3,1,null)")
    with pytest.raises(ValueError, match="one entry per layer"):
        mt.encoder_stack_packed(x, cu, layers, H, window=[(5, 9), None, None])
    with pytest.raises(ValueError, match="window must be a pair"):
        mt.encoder_stack_packed(x, cu, layers, H, window=[(5, 9), (1, 2, 3), None, None])


def test_the_encoder_stack_without_a_window_makes_todays_calls(rec):
    from flash_attention_minitorch_amd import modules_transformer as mt
    x, layers, cu, (T, H, Hkv, d) = _stack()
    rec.reset(dict(cu=cu))
    mt.encoder_stack_packed(x, cu, layers, H)
    today = list(rec.calls)
    assert _names(rec) == ["fa_mi355x_fwd_bidir"] * 4
    for window in (None, [None] * 4):
        rec.reset(dict(cu=cu))
        mt.encoder_stack_packed(x, cu, layers, H, None, window)
        assert rec.calls == today
