"""Causal packed attention with separate cu_seqlens for q and k (libflash_attn_mi355x_prefix.so) on the GPU: against the fp64
reference run per sequence, against the same library on each sequence alone (bit for bit: the law of
include/flash_attn_mi355x_prefix.h), the two block maps against the NumPy model of tests/test_bidir_cpu.py, clamping of bad arrays,
autograd, flash_attn_prefix (also against flash_attn_extend on a slab cache) and graph capture.

The reference is oracle.dense_attention_fw / _bw with causal=True (top-left aligned) on the SQUARE problem of n_k queries whose first
n_k - n_q query rows and out_grad rows are zeros: the last n_q rows of out, lse and dq are the bottom-right aligned answer, and dk
and dv are exact as they come (a row with dO = 0 has dP = delta = 0, hence dS = 0, and adds nothing to dV).  For n_q > n_k the first
n_q - n_k rows admit no key and give zeros; the rest is the square problem.
Tolerances: the project's envelope, max-abs 1e-4 (fp32) and 1e-3 (bf16) on out, lse, dq, dk and dv (tests/test_gpu_decode.py: TOL)."""
import math

import numpy as np
import pytest

import oracle
from gpu_util import maxabs
from test_bidir_cpu import QBLOCK, block_map_model, key_block
from test_gpu_bidir import _CLAMP, NAMES, QSIDE, _bits_equal, _dev, _i32, _inputs, _rows, _torch
from test_gpu_decode import TOL
from test_varlen_cpu import pack, seq_rows

pytestmark = pytest.mark.gpu

# name -> (nq per sequence, nk per sequence, (q lead, q tail), (k lead, k tail)); nk None: one array for both, cu_seqlens_k=None
SETS = {
    # decode; D = 0 across a block edge; no queries; no keys; D = 43; D = 95; few keys; n_q > n_k inside one block; n_q > n_k with the
    # whole first 128-row block empty and the second partly; D = 128
    "X": ([1, 129, 0, 128, 257, 33, 40, 5, 200, 64], [77, 129, 50, 0, 300, 128, 63, 2, 70, 192], (5, 19), (3, 0)),
    "Y": ([513, 31, 255, 256], None, (0, 0), (0, 0)),
    "Z": ([(1, 2, 3, 31, 32)[i % 5] for i in range(40)], [(32, 5, 64, 1, 33)[i % 5] for i in range(40)], (0, 0), (0, 0)),
    "U": ([300], [700], (0, 0), (0, 0)),   # the long prefix: block 0 must stop at key 527
    "V": ([150, 600, 129, 70], [165, 640, 129, 100], (0, 0), (0, 0)),   # short prefixes behind many queries
}


def _cus(name):
    """(cu_q, Tq, cu_k, Tk) of a set."""
    nq, nk, (ql, qt), (kl, kt) = SETS[name]
    cu_q, Tq = pack(nq, ql, qt)
    cu_k, Tk = pack(nk, kl, kt) if nk is not None else (cu_q, Tq)
    return cu_q, Tq, cu_k, Tk


def _run(tq, tk, tv, tdo, tcq, tck, scale=None):
    """The forward and the backward through device_ops: (out, lse, dq, dk, dv) device tensors."""
    from flash_attention_minitorch_amd import device_ops
    o, lse = device_ops.flash_attn_varlen_prefix_fwd(tq, tk, tv, tcq, tck, scale)
    return (o, lse) + tuple(device_ops.flash_attn_varlen_prefix_bwd(tq, tk, tv, o, tdo, lse, tcq, tck, scale))


def _reference(q, k, v, do, cu_q, Tq, cu_k, Tk, scale=None):
    """The fp64 reference per sequence (the module's docstring): out (Tq, H, d), lse (H, Tq), dq, dk, dv; zeros in the rows that
    admit no key, the key rows of a sequence without queries and the rows no sequence owns.  A caller's scale s is tau * f with
    f = s * sqrt(d): the oracle runs on f * q, and dq picks up the factor (tests/test_gpu_bidir.py: _reference)."""
    H, Hkv, d = q.shape[1], k.shape[1], q.shape[2]
    G, f = H // Hkv, 1.0 if scale is None else scale * math.sqrt(d)
    out, dq, lse = np.zeros((Tq, H, d)), np.zeros((Tq, H, d)), np.zeros((H, Tq))
    dk, dv = np.zeros((Tk, Hkv, d)), np.zeros((Tk, Hkv, d))
    for (sq, nq), (sk, nk) in zip(seq_rows(cu_q, Tq), seq_rows(cu_k, Tk)):
        if nq == 0 or nk == 0:
            continue
        drop, lead = max(nq - nk, 0), max(nk - nq, 0)   # query rows without a key; zero rows in front of the square problem
        sq, nq = sq + drop, nq - drop
        hq, hdo = (np.concatenate([np.zeros((H, lead, d)), a[sq:sq + nq].transpose(1, 0, 2).astype(np.float64)], 1) for a in (q, do))
        hk, hv = (np.repeat(a[sk:sk + nk].transpose(1, 0, 2), G, 0).astype(np.float64) for a in (k, v))
        ro, rl, _, _ = oracle.dense_attention_fw(hq * f, hk, hv, causal=True)
        rdq, rdk, rdv = oracle.dense_attention_bw(hq * f, hk, hv, hdo, causal=True)
        out[sq:sq + nq], dq[sq:sq + nq], lse[:, sq:sq + nq] = ro[:, lead:].transpose(1, 0, 2), f * rdq[:, lead:].transpose(1, 0, 2), rl[:, lead:]
        dk[sk:sk + nk], dv[sk:sk + nk] = (a.reshape(Hkv, G, nk, d).sum(1).transpose(1, 0, 2) for a in (rdk, rdv))
    return out, lse, dq, dk, dv


def _live(cu_q, Tq, cu_k, Tk):
    """(rows of the q buffers, rows of the k buffers) that carry a result: a query row that admits a key (i + n_k - n_q >= 0), a key
    row of a sequence with a query."""
    lq, lk = np.zeros(Tq, bool), np.zeros(Tk, bool)
    for (sq, nq), (sk, nk) in zip(seq_rows(cu_q, Tq), seq_rows(cu_k, Tk)):
        if nq and nk:
            lq[sq + max(nq - nk, 0):sq + nq] = True
            lk[sk:sk + nk] = True
    return lq, lk


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
    assert all({t for c in CASES if c[0] == n for t in (c[3],)} == {"bf16", "f32"} for n in SETS)
    assert [_cus(n)[1::2] for n in "XYZU"] == [(881, 1014), (1055, 1055), (552, 1080), (300, 700)] and len(SETS["Z"][0]) == 40
    deltas = [k - q for q, k in zip(*SETS["X"][:2]) if q and k]   # what set X is there for
    assert deltas == [76, 0, 43, 95, 23, -3, -130, 128] and (31, 1) in zip(*SETS["Z"][:2])


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
    for n, g, qside in zip(NAMES, got, QSIDE):   # empty rows, keyless sequences, sequences without queries, unowned rows: exactly zero
        assert np.all(_rows(n, g)[~(lq if qside else lk)] == 0), (case, n)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_caller_scale_reaches_the_kernels(dtype):
    cu_q, Tq, cu_k, Tk = _cus("X")
    q, k, v, do = _inputs(np.random.default_rng(5), dtype, Tq, Tk, 4, 2, 64)
    got = [t.double().cpu().numpy() for t in _run(*(_dev(a, dtype) for a in (q, k, v, do)), _i32(cu_q), _i32(cu_k), 0.2)]
    for n, g, w in zip(NAMES, got, _reference(q, k, v, do, cu_q, Tq, cu_k, Tk, 0.2)):
        assert maxabs(g, w) < TOL[dtype], (n, maxabs(g, w))


# ---- the law that defines the calls ----

@pytest.mark.parametrize("dtype,d", [("bf16", 64), ("f32", 128)])
@pytest.mark.parametrize("name", ["X", "Z"])
def test_every_sequence_has_the_bits_of_the_same_call_on_that_sequence_alone(name, dtype, d):
    cu_q, Tq, cu_k, Tk = _cus(name)
    H, Hkv = 4, 2
    tq, tk, tv, tdo = (_dev(a, dtype) for a in _inputs(np.random.default_rng(Tq + d), dtype, Tq, Tk, H, Hkv, d))
    got = _run(tq, tk, tv, tdo, _i32(cu_q), _i32(cu_k))
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
    assert seen == sum(1 for a, b in zip(*SETS[name][:2]) if a and b)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_two_calls_return_the_same_bits(dtype):
    cu_q, Tq, cu_k, Tk = _cus("X")
    ts = [_dev(a, dtype) for a in _inputs(np.random.default_rng(19), dtype, Tq, Tk, 4, 2, 64)]
    tcq, tck = _i32(cu_q), _i32(cu_k)
    first, second = _run(*ts, tcq, tck), _run(*ts, tcq, tck)
    assert all(_bits_equal(a, b) for a, b in zip(first, second))


# ---- the schedule launch against the model ----

@pytest.mark.parametrize("name,dtype,d", [("X", "bf16", 64), ("X", "f32", 64), ("Z", "bf16", 128), ("U", "f32", 32)])
def test_the_two_block_maps_in_the_workspace_are_the_models(name, dtype, d):
    torch = _torch()
    from flash_attention_minitorch_amd import _lib, device_ops
    cu_q, Tq, cu_k, Tk = _cus(name)
    H, Hkv = 4, 2
    tq, tk, tv, tdo = (_dev(a, dtype) for a in _inputs(np.random.default_rng(3), dtype, Tq, Tk, H, Hkv, d))
    tcq, tck = _i32(cu_q), _i32(cu_k)
    ws = device_ops.prefix_workspace(tq, tk, tcq, tck)
    ws.fill_(float("nan"))
    o, lse = device_ops.flash_attn_varlen_prefix_fwd(tq, tk, tv, tcq, tck, workspace=ws)
    device_ops.flash_attn_varlen_prefix_bwd(tq, tk, tv, o, tdo, lse, tcq, tck, workspace=ws)
    torch.cuda.synchronize()
    words = ws.view(torch.int32).cpu().numpy()
    map_q_bytes = _lib.prefix().fa_mi355x_fwd_prefix_workspace_bytes(len(cu_q) - 1, Tq, Tk, H, Hkv, d)
    for off, bs, keys in ((0, QBLOCK, False), (map_q_bytes // 4, key_block(dtype == "bf16", d), True)):
        want = block_map_model(cu_q, Tq, cu_k, Tk, bs, keys)
        got = words[off:off + want.size].reshape(want.shape)
        assert np.array_equal(got, want), (name, bs, got[:12], want[:12])


# ---- clamping ----

@pytest.mark.parametrize("bad,good", _CLAMP, ids=["past-q-neg-k", "neg-q-past-k", "decreasing-q", "decreasing-k", "extremes", "overlap"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_arrays_outside_the_buffers_are_clamped_and_nothing_outside_them_is_written(dtype, bad, good):
    """tests/test_gpu_bidir.py's bad arrays (Tq = 300, Tk = 200): decreasing, negative, past T.  No fault, every output finite,
    canary rows around every output untouched, the bits of the call on the clamped arrays, zeros outside the clamped ranges."""
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
        device_ops.flash_attn_varlen_prefix_fwd(tq, tk, tv, tcq, tck, out=out, lse=lse)
        device_ops.flash_attn_varlen_prefix_bwd(tq, tk, tv, out, tdo, lse, tcq, tck, grads=(dq, dk, dv))
        torch.cuda.synchronize()
        for f in full:
            assert bool((f[:C] == 777.0).all()) and bool((f[-C:] == 777.0).all())
        assert bool((lfull[0] == 777.0).all()) and bool((lfull[H + 1] == 777.0).all())
        return out, lse, dq, dk, dv
    res = call(*bad)
    assert all(bool(torch.isfinite(t).all()) for t in res)
    if good is not None:
        assert all(_bits_equal(a, b) for a, b in zip(res, call(*good)))
        lq, lk = _live(np.array(good[0]), Tq, np.array(good[1]), Tk)
        for n, t, qside in zip(NAMES, res, QSIDE):
            assert np.all(_rows(n, t.cpu().numpy())[~(lq if qside else lk)] == 0), n


# ---- autograd ----

def _grad_bound(dtype, want):
    """The gradients come back in the input dtype: bf16 (8 significant bits) adds one rounding, at most half an ulp = 2^-8 relative
    (tests/test_gpu_bidir.py::test_flash_attn_varlen_bidir_under_autograd)."""
    return TOL[dtype] + (2.0 ** -8 * float(np.max(np.abs(want))) if dtype == "bf16" else 0.0)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_flash_attn_varlen_prefix_under_autograd_with_a_padded_head_dim_and_a_callers_scale(dtype):
    from flash_attention_minitorch_amd import device_ops
    cu_q, Tq, cu_k, Tk = _cus("X")
    H, Hkv, d, scale = 4, 2, 80, 0.15
    q, k, v, do = _inputs(np.random.default_rng(d), dtype, Tq, Tk, H, Hkv, d)
    tq, tk, tv = (_dev(a, dtype).requires_grad_() for a in (q, k, v))
    o = device_ops.flash_attn_varlen_prefix(tq, tk, tv, _i32(cu_q), _i32(cu_k), scale)
    assert o.shape == (Tq, H, d)
    o.backward(_dev(do, "f32"))
    for t in (tq, tk, tv):
        assert t.grad.dtype == t.dtype and t.grad.shape == t.shape
    want = _reference(q, k, v, do, cu_q, Tq, cu_k, Tk, scale)
    want = (want[0],) + want[2:]
    got = [t.detach().double().cpu().numpy() for t in (o, tq.grad, tk.grad, tv.grad)]
    errs = [maxabs(g, w) for g, w in zip(got, want)]
    bound = [TOL[dtype]] + [_grad_bound(dtype, w) for w in want[1:]]
    print(errs, bound)
    assert all(e < b for e, b in zip(errs, bound)), (errs, bound)
    lq, lk = _live(cu_q, Tq, cu_k, Tk)
    assert all(np.all(g[~(lq if qside else lk)] == 0) for g, qside in zip(got, (True, True, False, False)))   # a zero gradient


# ---- flash_attn_prefix ----

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_flash_attn_prefix_matches_the_reference_and_flash_attn_extend_on_a_slab_cache(dtype):
    from flash_attention_minitorch_amd import device_ops
    B, Nq, Nk, H, Hkv, d = 2, 40, 170, 4, 2, 64
    q, k, v, do = _inputs(np.random.default_rng(11), dtype, B * Nq, B * Nk, H, Hkv, d)
    tq, tk, tv = (_dev(a, dtype).view(B, n, h, d).requires_grad_() for a, n, h in ((q, Nq, H), (k, Nk, Hkv), (v, Nk, Hkv)))
    o = device_ops.flash_attn_prefix(tq, tk, tv)
    assert o.shape == (B, Nq, H, d) and o.dtype == _torch().float32
    o.backward(_dev(do, "f32").view(B, Nq, H, d))
    cu_q, cu_k = np.arange(B + 1) * Nq, np.arange(B + 1) * Nk
    want = _reference(q, k, v, do, cu_q, B * Nq, cu_k, B * Nk)
    want = (want[0],) + want[2:]
    got = [t.detach().double().cpu().numpy().reshape(w.shape) for t, w in zip((o, tq.grad, tk.grad, tv.grad), want)]
    for g, w, grad in zip(got, want, (False, True, True, True)):
        assert maxabs(g, w) < (_grad_bound(dtype, w) if grad else TOL[dtype]), maxabs(g, w)
    # the forward against flash_attn_extend on a slab cache that holds the same keys: other kernels, each within TOL of fp64
    eo, _ = device_ops.flash_attn_extend(tq.detach(), tk.detach(), tv.detach(), None, causal=True)
    assert eo.shape == o.shape and maxabs(eo.double().cpu().numpy(), o.detach().double().cpu().numpy()) < 2 * TOL[dtype]


# ---- graph capture ----

def test_one_forward_and_backward_captured_in_a_graph_replays_on_new_data_and_new_lengths_in_both_arrays():
    """Neither array reaches the host: one capture, then q, k, v, dO and BOTH arrays change IN PLACE (other lengths, other unowned
    rows, other offsets between queries and keys, n_q > n_k, a keyless sequence and one without queries) and the replay equals the
    eager calls on the new data."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    dtype, H, Hkv, d = "bf16", 4, 2, 64
    cu_q, Tq, cu_k, Tk = _cus("X")
    tq, tk, tv, tdo = (_dev(a, dtype) for a in _inputs(np.random.default_rng(8), dtype, Tq, Tk, H, Hkv, d))
    tcq, tck = _i32(cu_q), _i32(cu_k)
    ws = device_ops.prefix_workspace(tq, tk, tcq, tck)
    out, lse = torch.empty((Tq, H, d), device="cuda"), torch.empty((H, Tq), device="cuda")
    grads = tuple(torch.empty((T, h, d), device="cuda") for T, h in ((Tq, H), (Tk, Hkv), (Tk, Hkv)))

    def call(o, l, g, w):
        device_ops.flash_attn_varlen_prefix_fwd(tq, tk, tv, tcq, tck, out=o, workspace=w, lse=l)
        device_ops.flash_attn_varlen_prefix_bwd(tq, tk, tv, o, tdo, l, tcq, tck, workspace=w, grads=g)
    call(out, lse, grads, ws)   # (the library is loaded and has launched once before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):   # one stream: schedule, forward, schedule, row constants, dK/dV, group sum, dQ
        call(out, lse, grads, ws)
    for t in (out, lse) + grads:
        t.fill_(float("nan"))
    new_q = [0, 300, 301, 301, 430, 431, 560, 600, 700, 800, 870]
    new_k = [10, 10, 200, 330, 331, 400, 401, 620, 650, 900, 1014]
    assert len(new_q) == len(cu_q) and new_q[-1] <= Tq and new_k[-1] <= Tk
    tcq.copy_(_i32(new_q)), tck.copy_(_i32(new_k))
    tq.mul_(-0.5), tk.mul_(0.75), tv.mul_(-1.0), tdo.mul_(0.5)
    g.replay()
    torch.cuda.synchronize()
    ro, rl = torch.empty_like(out), torch.empty_like(lse)
    rg = tuple(torch.empty_like(t) for t in grads)
    call(ro, rl, rg, device_ops.prefix_workspace(tq, tk, tcq, tck))
    torch.cuda.synchronize()
    for a, b in zip((out, lse) + grads, (ro, rl) + rg):
        assert _bits_equal(a, b) and not bool(torch.isnan(a).any())
    lq, lk = _live(np.array(new_q), Tq, np.array(new_k), Tk)
    tlq, tlk = torch.from_numpy(lq).cuda(), torch.from_numpy(lk).cuda()
    assert bool((out[~tlq] == 0).all()) and bool((out[tlq].abs().amax(dim=(1, 2)) > 0).all())
    assert bool((grads[1][~tlk] == 0).all()) and bool((grads[2][tlk].abs().amax(dim=(1, 2)) > 0).all())
