"""Bidirectional packed attention with separate cu_seqlens for q and k (libflash_attn_mi355x_bidir.so) on the GPU: against the fp64
reference (oracle.dense_attention_fw / _bw, which take different row counts for q and k) run per sequence, against the same library
on each sequence alone (bit for bit: the law of include/flash_attn_mi355x_bidir.h), the two block maps against the NumPy model of
tests/test_bidir_cpu.py, clamping of bad arrays, autograd, flash_attn_cross, the packed model functions and graph capture.
Tolerances: the project's envelope, max-abs 1e-4 (fp32) and 1e-3 (bf16) on out, lse, dq, dk and dv (tests/test_gpu_decode.py: TOL)."""
import math

import numpy as np
import pytest

import oracle
from gpu_util import maxabs, rand_u, to_np
from test_bidir_cpu import QBLOCK, block_map_model, key_block
from test_gpu_decode import TOL
from test_varlen_cpu import pack, seq_rows

pytestmark = pytest.mark.gpu

NAMES = ("out", "lse", "dq", "dk", "dv")
QSIDE = (True, True, True, False, False)   # which buffer's rows an output has

# name -> (nq per sequence, nk per sequence, (q lead, q tail), (k lead, k tail)); nk None: self-attention, cu_seqlens_k=None
SETS = {
    "X": ([1, 129, 0, 128, 257, 33, 40], [77, 1, 50, 0, 300, 128, 63], (5, 19), (3, 0)),
    "Y": ([513, 31, 255, 256], None, (0, 0), (0, 0)),
    "Z": ([(1, 2, 3, 31, 32)[i % 5] for i in range(40)], [(32, 5, 64, 1, 33)[i % 5] for i in range(40)], (0, 0), (0, 0)),
    "U": ([300], [700], (0, 0), (0, 0)),
    # beside the issue's four: many queries on few keys, where a key's dK and dV collect the bf16 rounding of G * n_q probabilities
    # of order 1 / n_k (bidir_dkdv_kernel splits P and dS past G * n_q = n_k^2 / 32: both sides of that threshold for G = 1, 2, 4)
    "V": ([150, 600, 129, 70], [65, 70, 64, 100], (2, 5), (4, 3)),
}


def _torch():
    import torch
    return torch


def _tdt(dtype):
    torch = _torch()
    return torch.bfloat16 if dtype == "bf16" else torch.float32


def _cus(name):
    """(cu_q, Tq, cu_k, Tk) of a set."""
    nq, nk, (ql, qt), (kl, kt) = SETS[name]
    cu_q, Tq = pack(nq, ql, qt)
    cu_k, Tk = pack(nk, kl, kt) if nk is not None else (cu_q, Tq)
    return cu_q, Tq, cu_k, Tk


def _inputs(rng, dtype, Tq, Tk, H, Hkv, d):
    """q, k, v, do as packed (T, heads, d) float32 arrays, U(-1, 1), rounded to the dtype first."""
    rnd = (lambda s: oracle.bf16_round(rand_u(rng, s))) if dtype == "bf16" else (lambda s: rand_u(rng, s))
    return rnd((Tq, H, d)), rnd((Tk, Hkv, d)), rnd((Tk, Hkv, d)), rnd((Tq, H, d))


def _dev(a, dtype):
    return _torch().from_numpy(np.ascontiguousarray(a)).to("cuda", _tdt(dtype)).contiguous()


def _i32(a):
    torch = _torch()
    return torch.tensor([int(x) for x in a], dtype=torch.int32, device="cuda")


def _run(tq, tk, tv, tdo, tcq, tck, scale=None):
    """The forward and the backward through device_ops: (out, lse, dq, dk, dv) device tensors."""
    from flash_attention_minitorch_amd import device_ops
    o, lse = device_ops.flash_attn_varlen_bidir_fwd(tq, tk, tv, tcq, tck, scale)
    return (o, lse) + tuple(device_ops.flash_attn_varlen_bidir_bwd(tq, tk, tv, o, tdo, lse, tcq, tck, scale))


def _reference(q, k, v, do, cu_q, Tq, cu_k, Tk, scale=None):
    """The fp64 reference per sequence: out (Tq, H, d), lse (H, Tq), dq, dk, dv; zeros in the query rows of a keyless sequence, the
    key rows of a sequence without queries and the rows no sequence owns.  A caller's scale s is tau * f with f = s * sqrt(d): the
    oracle runs on f * q, and dq picks up the factor."""
    H, Hkv, d = q.shape[1], k.shape[1], q.shape[2]
    G, f = H // Hkv, 1.0 if scale is None else scale * math.sqrt(d)
    out, dq, lse = np.zeros((Tq, H, d)), np.zeros((Tq, H, d)), np.zeros((H, Tq))
    dk, dv = np.zeros((Tk, Hkv, d)), np.zeros((Tk, Hkv, d))
    for (sq, nq), (sk, nk) in zip(seq_rows(cu_q, Tq), seq_rows(cu_k, Tk)):
        if nq == 0 or nk == 0:
            continue
        hq, hdo = (a[sq:sq + nq].transpose(1, 0, 2).astype(np.float64) for a in (q, do))
        hk, hv = (np.repeat(a[sk:sk + nk].transpose(1, 0, 2), G, 0).astype(np.float64) for a in (k, v))
        ro, rl, _, _ = oracle.dense_attention_fw(hq * f, hk, hv)
        rdq, rdk, rdv = oracle.dense_attention_bw(hq * f, hk, hv, hdo)
        out[sq:sq + nq], dq[sq:sq + nq], lse[:, sq:sq + nq] = ro.transpose(1, 0, 2), f * rdq.transpose(1, 0, 2), rl
        dk[sk:sk + nk], dv[sk:sk + nk] = (a.reshape(Hkv, G, nk, d).sum(1).transpose(1, 0, 2) for a in (rdk, rdv))
    return out, lse, dq, dk, dv


def _live(cu_q, Tq, cu_k, Tk):
    """(rows of the q buffers, rows of the k buffers) that carry a result: owned by a sequence with a row on the other side too."""
    lq, lk = np.zeros(Tq, bool), np.zeros(Tk, bool)
    for (sq, nq), (sk, nk) in zip(seq_rows(cu_q, Tq), seq_rows(cu_k, Tk)):
        if nq and nk:
            lq[sq:sq + nq] = True
            lk[sk:sk + nk] = True
    return lq, lk


def _rows(name, a):
    """A (T, ..) or (H, T) array with the packed rows first."""
    return a if name != "lse" else a.T


def _bits_equal(a, b):
    torch = _torch()
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)))


# (set, H, Hkv, dtype, d): a covering selection, not the product
CASES = [
    ("X", 4, 2, "bf16", 32), ("X", 4, 1, "bf16", 64), ("X", 4, 2, "bf16", 128),
    ("X", 4, 1, "f32", 32), ("X", 4, 2, "f32", 64), ("X", 4, 2, "f32", 128),
    ("X", 4, 4, "bf16", 64), ("X", 4, 4, "f32", 64),
    ("Y", 4, 4, "bf16", 128), ("Y", 4, 2, "f32", 32), ("Y", 4, 1, "bf16", 64),
    ("Z", 4, 2, "bf16", 32), ("Z", 4, 1, "f32", 128), ("Z", 4, 4, "bf16", 64),
    ("U", 4, 2, "bf16", 64), ("U", 4, 4, "f32", 128), ("U", 4, 1, "bf16", 128),
    ("V", 4, 2, "bf16", 64), ("V", 4, 1, "bf16", 128), ("V", 4, 4, "bf16", 32), ("V", 4, 2, "f32", 64),
]


def test_the_cases_cover_every_set_every_dtype_d_pair_with_groups_and_every_pair_on_set_x():
    assert {c[0] for c in CASES} == set(SETS)
    assert {(c[1], c[2]) for c in CASES} == {(4, 4), (4, 2), (4, 1)}
    pairs = {(t, d) for t in ("bf16", "f32") for d in (32, 64, 128)}
    assert {(c[3], c[4]) for c in CASES if c[1] > c[2]} == pairs
    assert {(c[3], c[4]) for c in CASES if c[0] == "X"} == pairs
    assert [_cus(n)[1::2] for n in "XYZU"] == [(612, 622), (1055, 1055), (552, 1080), (300, 700)] and len(SETS["Z"][0]) == 40
    nq, nk = SETS["X"][:2]   # what set X is there for
    assert 1 in nq and 1 in nk and any(0 < n < 64 for n in nk) and any(n >= 64 for n in nk) and 128 in nk and 300 in nk
    assert any(k == 0 and q > 0 and 0 < i < len(nk) - 1 for i, (q, k) in enumerate(zip(nq, nk))) and any(q == 0 and k > 0 for q, k in zip(nq, nk))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "{}-h{}kv{}-{}-d{}".format(*c))
def test_forward_and_backward_match_the_fp64_reference_per_sequence(case):
    name, H, Hkv, dtype, d = case
    cu_q, Tq, cu_k, Tk = _cus(name)
    q, k, v, do = _inputs(np.random.default_rng(Tq * 1000 + Tk + d), dtype, Tq, Tk, H, Hkv, d)
    tck = None if SETS[name][1] is None else _i32(cu_k)
    got = [t.double().cpu().numpy() for t in _run(*(_dev(a, dtype) for a in (q, k, v, do)), _i32(cu_q), tck)]
    want = _reference(q, k, v, do, cu_q, Tq, cu_k, Tk)
    errs = {n: maxabs(g, w) for n, g, w in zip(NAMES, got, want)}
    print(case, {n: f"{e:.2e}" for n, e in errs.items()})
    assert all(np.all(np.isfinite(g)) for g in got), case
    assert all(e < TOL[dtype] for e in errs.values()), (case, errs, TOL[dtype])
    lq, lk = _live(cu_q, Tq, cu_k, Tk)
    for n, g, qside in zip(NAMES, got, QSIDE):   # keyless sequences, sequences without queries, unowned rows: exactly zero
        assert np.all(_rows(n, g)[~(lq if qside else lk)] == 0), (case, n)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_caller_scale_reaches_the_kernels(dtype):
    cu_q, Tq, cu_k, Tk = _cus("X")
    q, k, v, do = _inputs(np.random.default_rng(5), dtype, Tq, Tk, 4, 2, 64)
    got = [t.double().cpu().numpy() for t in _run(*(_dev(a, dtype) for a in (q, k, v, do)), _i32(cu_q), _i32(cu_k), 0.2)]
    for n, g, w in zip(NAMES, got, _reference(q, k, v, do, cu_q, Tq, cu_k, Tk, 0.2)):
        assert maxabs(g, w) < TOL[dtype], (n, maxabs(g, w))
    default = _reference(q, k, v, do, cu_q, Tq, cu_k, Tk)
    assert maxabs(got[0], default[0]) > 10 * TOL[dtype]   # (and 0.2 is not what d = 64 gives by itself)


# ---- the law that defines the calls ----

@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["X", "Y"])
def test_every_sequence_has_the_bits_of_the_same_call_on_that_sequence_alone(name, dtype, d):
    cu_q, Tq, cu_k, Tk = _cus(name)
    H, Hkv = 4, 2
    tq, tk, tv, tdo = (_dev(a, dtype) for a in _inputs(np.random.default_rng(Tq + d), dtype, Tq, Tk, H, Hkv, d))
    got = _run(tq, tk, tv, tdo, _i32(cu_q), None if SETS[name][1] is None else _i32(cu_k))
    seen = 0
    for (sq, nq), (sk, nk) in zip(seq_rows(cu_q, Tq), seq_rows(cu_k, Tk)):
        if nq == 0 or nk == 0:
            continue
        one = [t[s:s + n].contiguous() for t, s, n in ((tq, sq, nq), (tk, sk, nk), (tv, sk, nk), (tdo, sq, nq))]
        alone = _run(*one, _i32([0, nq]), _i32([0, nk]))
        for nm, g, a, qside in zip(NAMES, got, alone, QSIDE):
            s, n = (sq, nq) if qside else (sk, nk)
            mine = g[:, s:s + n] if nm == "lse" else g[s:s + n]
            assert _bits_equal(mine, a), (name, dtype, d, nm, (sq, nq, sk, nk), float((mine - a).abs().max()))
        seen += 1
    assert seen == sum(1 for a, b in zip(SETS[name][0], SETS[name][1] or SETS[name][0]) if a and b)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_two_calls_return_the_same_bits(dtype):
    cu_q, Tq, cu_k, Tk = _cus("X")
    ts = [_dev(a, dtype) for a in _inputs(np.random.default_rng(19), dtype, Tq, Tk, 4, 2, 64)]
    tcq, tck = _i32(cu_q), _i32(cu_k)
    first, second = _run(*ts, tcq, tck), _run(*ts, tcq, tck)
    assert all(_bits_equal(a, b) for a, b in zip(first, second))


# ---- the schedule launch against the model ----

@pytest.mark.parametrize("name,dtype,d", [("X", "bf16", 64), ("X", "f32", 64), ("Z", "bf16", 32), ("Z", "bf16", 128), ("U", "f32", 32)])
def test_the_two_block_maps_in_the_workspace_are_the_models(name, dtype, d):
    torch = _torch()
    from flash_attention_minitorch_amd import _lib, device_ops
    cu_q, Tq, cu_k, Tk = _cus(name)
    H, Hkv = 4, 2
    tq, tk, tv, tdo = (_dev(a, dtype) for a in _inputs(np.random.default_rng(3), dtype, Tq, Tk, H, Hkv, d))
    tcq, tck = _i32(cu_q), _i32(cu_k)
    ws = device_ops.bidir_workspace(tq, tk, tcq, tck)
    ws.fill_(float("nan"))
    o, lse = device_ops.flash_attn_varlen_bidir_fwd(tq, tk, tv, tcq, tck, workspace=ws)
    device_ops.flash_attn_varlen_bidir_bwd(tq, tk, tv, o, tdo, lse, tcq, tck, workspace=ws)
    torch.cuda.synchronize()
    words = ws.view(torch.int32).cpu().numpy()
    map_q_bytes = _lib.bidir().fa_mi355x_fwd_bidir_workspace_bytes(len(cu_q) - 1, Tq, Tk, H, Hkv, d)
    for off, bs, keys in ((0, QBLOCK, False), (map_q_bytes // 4, key_block(dtype == "bf16", d), True)):
        want = block_map_model(cu_q, Tq, cu_k, Tk, bs, keys)
        got = words[off:off + want.size].reshape(want.shape)
        assert np.array_equal(got, want), (name, bs, got[:12], want[:12])


# ---- clamping ----

# (cu_q, cu_k as given, the clamped arrays that own the same rows): Tq = 300, Tk = 200.  The last pair decreases in the middle, so
# that two sequences own the same rows (no array of the clamped form says that: good is None): the canaries alone are checked.
_CLAMP = [
    (([0, 200, 9999], [-7, 100, 200]), ([0, 200, 300], [0, 100, 200])),          # past Tq; negative in k
    (([-5, 100, 300], [0, 150, 5000]), ([0, 100, 300], [0, 150, 200])),          # negative in q; past Tk
    (([0, 200, 100], [0, 150, 200]), ([0, 200, 200], [0, 150, 200])),            # decreasing in q: a sequence without queries
    (([0, 100, 300], [0, 150, 20]), ([0, 100, 300], [0, 150, 150])),             # decreasing in k: a keyless sequence
    (([2 ** 31 - 1, -2 ** 31, 250], [0, -2 ** 31, 2 ** 31 - 1]), ([300, 0, 250], [0, 0, 200])),   # (q: (300, 0), (0, 250))
    (([0, 250, 100, 300], [0, 100, 100, 200]), None),
]


@pytest.mark.parametrize("bad,good", _CLAMP, ids=["past-q-neg-k", "neg-q-past-k", "decreasing-q", "decreasing-k", "extremes", "overlap"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_arrays_outside_the_buffers_are_clamped_and_nothing_outside_them_is_written(dtype, bad, good):
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    Tq, Tk, H, Hkv, d, C = 300, 200, 4, 2, 64, 8
    tq, tk, tv, tdo = (_dev(a, dtype) for a in _inputs(np.random.default_rng(7), dtype, Tq, Tk, H, Hkv, d))

    def call(cu_q, cu_k):
        """Every output sits between C canary rows (lse: one canary head on each side)."""
        full = [torch.full((T + 2 * C, h, d), 777.0, device="cuda") for T, h in ((Tq, H), (Tq, H), (Tk, Hkv), (Tk, Hkv))]
        lfull = torch.full((H + 2, Tq), 777.0, device="cuda")
        out, dq, dk, dv = (f[C:C + f.shape[0] - 2 * C] for f in full)
        lse = lfull[1:H + 1]
        tcq, tck = _i32(cu_q), _i32(cu_k)
        device_ops.flash_attn_varlen_bidir_fwd(tq, tk, tv, tcq, tck, out=out, lse=lse)
        device_ops.flash_attn_varlen_bidir_bwd(tq, tk, tv, out, tdo, lse, tcq, tck, grads=(dq, dk, dv))
        torch.cuda.synchronize()
        for f in full:
            assert bool((f[:C] == 777.0).all()) and bool((f[-C:] == 777.0).all())
        assert bool((lfull[0] == 777.0).all()) and bool((lfull[H + 1] == 777.0).all())
        return out, lse, dq, dk, dv
    res = call(*bad)
    assert all(bool(torch.isfinite(t).all()) for t in res)
    if good is not None:
        assert all(_bits_equal(a, b) for a, b in zip(res, call(*good)))


# ---- autograd ----

def _torch_reference(q, k, v, do, cu_q, Tq, cu_k, Tk):
    """out and the gradients by torch autograd in fp64 on the CPU, per sequence: plain softmax attention, groups by repetition."""
    torch = _torch()
    tq, tk, tv = (torch.from_numpy(a).double().requires_grad_() for a in (q, k, v))
    G, d = q.shape[1] // k.shape[1], q.shape[2]
    out = torch.zeros(q.shape, dtype=torch.float64)
    for (sq, nq), (sk, nk) in zip(seq_rows(cu_q, Tq), seq_rows(cu_k, Tk)):
        if nq and nk:
            kk, vv = (t[sk:sk + nk].repeat_interleave(G, dim=1) for t in (tk, tv))
            p = torch.softmax(torch.einsum("ihd,jhd->hij", tq[sq:sq + nq], kk) / math.sqrt(d), dim=-1)
            out = out.index_put((torch.arange(sq, sq + nq),), torch.einsum("hij,jhd->ihd", p, vv))
    out.backward(torch.from_numpy(do).double())
    return [t.detach().numpy() for t in (out, tq.grad, tk.grad, tv.grad)]


@pytest.mark.parametrize("d,dtype", [(64, "bf16"), (80, "bf16"), (80, "f32")])
def test_flash_attn_varlen_bidir_under_autograd(d, dtype):
    """flash_attn_varlen_bidir and .backward() against a torch fp64 reference; d = 80 through the zero padding.  The bound is that of
    tests/test_gpu_varlen.py::test_flash_attn_varlen_under_autograd: the gradients come back in the input dtype, and bf16 (8
    significant bits) adds one rounding, at most half an ulp = 2^-8 relative."""
    from flash_attention_minitorch_amd import device_ops
    cu_q, Tq, cu_k, Tk = _cus("X")
    H, Hkv = 4, 2
    q, k, v, do = _inputs(np.random.default_rng(d), dtype, Tq, Tk, H, Hkv, d)
    tq, tk, tv = (_dev(a, dtype).requires_grad_() for a in (q, k, v))
    o = device_ops.flash_attn_varlen_bidir(tq, tk, tv, _i32(cu_q), _i32(cu_k))
    assert o.shape == (Tq, H, d)
    o.backward(_dev(do, "f32"))
    for t in (tq, tk, tv):
        assert t.grad.dtype == t.dtype and t.grad.shape == t.shape
    want = _torch_reference(q, k, v, do, cu_q, Tq, cu_k, Tk)
    got = [t.detach().double().cpu().numpy() for t in (o, tq.grad, tk.grad, tv.grad)]
    tol = TOL[dtype]
    errs = [maxabs(g, w) for g, w in zip(got, want)]
    bound = [tol] + [tol + (2.0 ** -8 * float(np.max(np.abs(w))) if dtype == "bf16" else 0.0) for w in want[1:]]
    print(errs, bound)
    assert all(e < b for e, b in zip(errs, bound)), (errs, bound)
    lq, lk = _live(cu_q, Tq, cu_k, Tk)
    assert all(np.all(g[~(lq if qside else lk)] == 0) for g, qside in zip(got, (True, True, False, False)))   # a zero gradient


# ---- flash_attn_cross ----

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_flash_attn_cross_with_different_row_counts_matches_the_reference(dtype):
    from flash_attention_minitorch_amd import device_ops
    B, Nq, Nk, H, Hkv, d = 3, 70, 200, 4, 2, 64
    q, k, v, do = _inputs(np.random.default_rng(11), dtype, B * Nq, B * Nk, H, Hkv, d)
    tq, tk, tv = (_dev(a, dtype).view(B, n, h, d).requires_grad_() for a, n, h in ((q, Nq, H), (k, Nk, Hkv), (v, Nk, Hkv)))
    o = device_ops.flash_attn_cross(tq, tk, tv)
    assert o.shape == (B, Nq, H, d) and o.dtype == _torch().float32
    o.backward(_dev(do, "f32").view(B, Nq, H, d))
    cu_q, cu_k = np.arange(B + 1) * Nq, np.arange(B + 1) * Nk
    want = _reference(q, k, v, do, cu_q, B * Nq, cu_k, B * Nk)
    got = [t.detach().double().cpu().numpy().reshape(w.shape) for t, w in zip((o, tq.grad, tk.grad, tv.grad), (want[0],) + want[2:])]
    tol = TOL[dtype]
    for g, w, grad in zip(got, (want[0],) + want[2:], (False, True, True, True)):   # (the gradients are rounded to bf16: see the autograd test)
        assert maxabs(g, w) < tol + (2.0 ** -8 * float(np.max(np.abs(w))) if grad and dtype == "bf16" else 0.0), maxabs(g, w)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_flash_attn_cross_with_equal_row_counts_is_within_tol_of_flash_attn_gqa(dtype):
    """Other kernels (the batched non-causal call runs the MFMA-slot pipelines): a tolerance, not bits.  Both sides round their
    gradients to the input dtype: bf16 allows half an ulp, 2^-9 relative, for each."""
    from flash_attention_minitorch_amd import device_ops
    B, N, H, Hkv, d = 2, 256, 4, 2, 64
    q, k, v, do = _inputs(np.random.default_rng(12), dtype, B * N, B * N, H, Hkv, d)
    res = []
    for fn in (device_ops.flash_attn_cross, lambda a, b, c: device_ops.flash_attn_gqa(a, b, c, causal=False)):
        tq, tk, tv = (_dev(a, dtype).view(B, N, h, d).requires_grad_() for a, h in ((q, H), (k, Hkv), (v, Hkv)))
        o = fn(tq, tk, tv)
        o.backward(_dev(do, "f32").view(B, N, H, d))
        res.append([to_np(t.detach().float()).astype(np.float64) for t in (o, tq.grad, tk.grad, tv.grad)])
    for a, b, grad in zip(res[0], res[1], (False, True, True, True)):
        bound = TOL[dtype] + (2.0 ** -8 * float(np.max(np.abs(b))) if grad and dtype == "bf16" else 0.0)
        assert a.shape == b.shape and maxabs(a, b) < bound, (maxabs(a, b), bound)


# ---- the model functions ----

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_encoder_stack_packed_matches_attention_stack_on_each_sequence_alone(dtype):
    """Two layers, rotary positions that restart at every sequence, two kv heads, set Y's lengths with unowned rows around them.  The
    tolerance is the model tolerance of tests/test_gpu_varlen.py's model test (tests/test_gpu_extend.py: _model_tol): attention_stack
    runs the batched non-causal kernels, other kernels than the packed call's."""
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    from test_gpu_decode_append import _stack
    from test_gpu_extend import _model_tol
    E, H, Hkv, L = 256, 4, 2, 2
    cu, T = pack([130, 31, 255, 64], 5, 19)
    x3, layers = _stack(np.random.default_rng(21), dtype, 1, E, H, Hkv, L, T)
    x = x3[0].contiguous()
    rope = mt.Rotary.table(512, E // H, device="cuda")
    dy = torch.from_numpy(rand_u(np.random.default_rng(4), (T, E))).to("cuda", _tdt(dtype))
    xg = x.clone().requires_grad_()
    y = mt.encoder_stack_packed(xg, _i32(cu), layers, H, rope=rope)
    y.backward(dy)
    own = np.zeros(T, bool)
    for s, n in seq_rows(cu, T):
        own[s:s + n] = True
        xs = x[s:s + n][None].clone().requires_grad_()
        ys = mt.attention_stack(xs, layers, H, causal=False, rope=rope)
        ys.backward(dy[s:s + n][None])
        for got, want in ((y[s:s + n], ys[0]), (xg.grad[s:s + n], xs.grad[0])):
            tol = _model_tol(dtype, to_np(want))
            assert maxabs(to_np(got), to_np(want)) < tol, ((s, n), maxabs(to_np(got), to_np(want)), tol)
    own = torch.from_numpy(own).cuda()
    assert _bits_equal(y[~own], x[~own])   # an unowned row: the residual alone


@pytest.mark.parametrize("Hkv", [4, 1])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_cross_attention_packed_matches_a_torch_reference_per_sequence(dtype, Hkv):
    """Against torch fp64 on the CPU from the same (rounded) x, memory and weights, per sequence; one keyless sequence in the middle.
    The model tolerance (tests/test_gpu_extend.py: _model_tol): the projections run in the input dtype on the GPU."""
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    from test_gpu_extend import _model_tol
    E, Em, H = 256, 96, 4
    d = E // H
    cu_q, Tq = pack([70, 33, 129], 2, 3)
    cu_k, Tk = pack([200, 0, 45], 0, 4)
    rng = np.random.default_rng(31 + Hkv)
    rnd = (lambda s: oracle.bf16_round(rand_u(rng, s))) if dtype == "bf16" else (lambda s: rand_u(rng, s))
    x, mem, dy = rnd((Tq, E)), rnd((Tk, Em)), rnd((Tq, E))
    wq, wk, wv, wo = (rnd((a, b)) / np.float32(math.sqrt(a)) for a, b in ((E, E), (Em, Hkv * d), (Em, Hkv * d), (E, E)))
    wq, wk, wv, wo = (oracle.bf16_round(w) if dtype == "bf16" else w for w in (wq, wk, wv, wo))
    tx, tm = (_dev(a, dtype).requires_grad_() for a in (x, mem))
    y = mt.cross_attention_packed(tx, _i32(cu_q), tm, _i32(cu_k), *(_dev(w, dtype) for w in (wq, wk, wv, wo)), H)
    assert y.shape == (Tq, E) and y.dtype == _tdt(dtype)
    y.backward(_dev(dy, dtype))
    rx, rm = (torch.from_numpy(a).double().requires_grad_() for a in (x, mem))
    w64 = [torch.from_numpy(w).double() for w in (wq, wk, wv, wo)]
    q, k, v = (rx @ w64[0]).view(Tq, H, d), (rm @ w64[1]).view(Tk, Hkv, d), (rm @ w64[2]).view(Tk, Hkv, d)
    o = torch.zeros(Tq, H, d, dtype=torch.float64)
    for (sq, nq), (sk, nk) in zip(seq_rows(cu_q, Tq), seq_rows(cu_k, Tk)):
        if nq and nk:
            kk, vv = (t[sk:sk + nk].repeat_interleave(H // Hkv, dim=1) for t in (k, v))
            p = torch.softmax(torch.einsum("ihd,jhd->hij", q[sq:sq + nq], kk) / math.sqrt(d), dim=-1)
            o = o.index_put((torch.arange(sq, sq + nq),), torch.einsum("hij,jhd->ihd", p, vv))
    ry = o.reshape(Tq, E) @ w64[3]
    ry.backward(torch.from_numpy(dy).double())
    for got, want in ((y, ry), (tx.grad, rx.grad), (tm.grad, rm.grad)):
        want = want.detach().numpy()
        tol = _model_tol(dtype, want)
        assert maxabs(to_np(got.detach().float()), want) < tol, (maxabs(to_np(got.detach().float()), want), tol)
    assert not bool(y[int(cu_q[1]):int(cu_q[2])].any())   # the keyless sequence: zero attention output, zero rows


# ---- graph capture ----

def test_one_forward_and_backward_captured_in_a_graph_replays_on_new_data_and_new_lengths_in_both_arrays():
    """Neither array reaches the host: one capture, then q, k, v, dO and BOTH arrays change IN PLACE (other lengths, other unowned
    rows, a keyless sequence and one without queries) and the replay equals the eager calls on the new data."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    dtype, H, Hkv, d = "bf16", 4, 2, 64
    cu_q, Tq, cu_k, Tk = _cus("X")
    tq, tk, tv, tdo = (_dev(a, dtype) for a in _inputs(np.random.default_rng(8), dtype, Tq, Tk, H, Hkv, d))
    tcq, tck = _i32(cu_q), _i32(cu_k)
    ws = device_ops.bidir_workspace(tq, tk, tcq, tck)
    out, lse = torch.empty((Tq, H, d), device="cuda"), torch.empty((H, Tq), device="cuda")
    grads = tuple(torch.empty((T, h, d), device="cuda") for T, h in ((Tq, H), (Tk, Hkv), (Tk, Hkv)))

    def call(o, l, g, w):
        device_ops.flash_attn_varlen_bidir_fwd(tq, tk, tv, tcq, tck, out=o, workspace=w, lse=l)
        device_ops.flash_attn_varlen_bidir_bwd(tq, tk, tv, o, tdo, l, tcq, tck, workspace=w, grads=g)
    call(out, lse, grads, ws)   # (the library is loaded and has launched once before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):   # one stream: schedule, forward, schedule, row constants, dK/dV, group sum, dQ
        call(out, lse, grads, ws)
    for t in (out, lse) + grads:
        t.fill_(float("nan"))
    new_q, new_k = [0, 300, 301, 301, 430, 431, 560, 600], [10, 10, 200, 330, 331, 400, 401, 620]
    tcq.copy_(_i32(new_q)), tck.copy_(_i32(new_k))
    tq.mul_(-0.5), tk.mul_(0.75), tv.mul_(-1.0), tdo.mul_(0.5)
    g.replay()
    torch.cuda.synchronize()
    ro, rl = torch.empty_like(out), torch.empty_like(lse)
    rg = tuple(torch.empty_like(t) for t in grads)
    call(ro, rl, rg, device_ops.bidir_workspace(tq, tk, tcq, tck))
    torch.cuda.synchronize()
    for a, b in zip((out, lse) + grads, (ro, rl) + rg):
        assert _bits_equal(a, b) and not bool(torch.isnan(a).any())
    lq, lk = _live(np.array(new_q), Tq, np.array(new_k), Tk)
    tlq, tlk = torch.from_numpy(lq).cuda(), torch.from_numpy(lk).cuda()
    assert bool((out[~tlq] == 0).all()) and bool((out[tlq].abs().amax(dim=(1, 2)) > 0).all())
    assert bool((grads[1][~tlk] == 0).all()) and bool((grads[2][tlk].abs().amax(dim=(1, 2)) > 0).all())
