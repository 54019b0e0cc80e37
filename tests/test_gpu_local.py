"""Packed attention under a two-sided sliding window with separate cu_seqlens for q and k (libflash_attn_mi355x_local.so) on the
GPU: against the fp64 band reference of tests/test_local_cpu.py per sequence, against the existing calls where the window is an
existing mask (the new library called through its C symbols, past the Python routing), against the same library on each sequence
alone (bit for bit: the law of include/flash_attn_mi355x_local.h), the two block maps against the NumPy model of
tests/test_bidir_cpu.py, clamping of bad arrays, autograd, flash_attn_local, the encoder stack with a local and a global layer, graph
capture, and scores beyond U(-1, 1).

Tolerances: the project's envelope, max-abs 1e-4 (fp32) and 1e-3 (bf16) on out, lse, dq, dk and dv (tests/test_gpu_decode.py: TOL);
two calls that are each within TOL of one fp64 answer agree within 2 x TOL.  The large-score cases: the envelope of
tests/test_gpu_score_range.py."""
import ctypes
import functools

import numpy as np
import pytest

import score_range as sr
import test_gpu_prefix as tp
import test_gpu_varlen as tv
from gpu_util import maxabs, rand_u
from test_bidir_cpu import QBLOCK, block_map_model, key_block
from test_gpu_bidir import _CLAMP, NAMES, QSIDE, _bits_equal, _dev, _i32, _inputs, _rows, _tdt, _torch
from test_gpu_bidir import _run as bidir_run
from test_gpu_decode import TOL
from test_local_cpu import local_admit, local_live, local_reference
from test_varlen_cpu import pack, seq_rows

pytestmark = pytest.mark.gpu

# name -> (nq per sequence, nk per sequence, (q lead, q tail), (k lead, k tail)); nk None: one array for both, cu_seqlens_k=None
SETS = {
    "X": tp.SETS["X"],   # two arrays, leads and tails, n_k - n_q of 76, 0, 43, 95, 23, -3, -130, 128, no queries, no keys
    "Y": ([513, 31, 255, 256], None, (0, 0), (0, 0)),
    "U": ([300], [700], (0, 0), (0, 0)),
    "S": ([700], None, (0, 0), (0, 0)),
}
# narrower than a 32-wide sub-tile; the 64-key split threshold from both sides; across the 32 / 64-key forward tiles, the 128 / 256-key
# dK/dV blocks and the 32 / 64 / 128-query slices; each one-sided form; wider than every sequence
WINDOWS = [(0, 0), (1, 0), (0, 1), (5, 9), (31, 32), (63, 64), (64, 63), (127, 128), (200, 100), (-1, 17), (40, -1), (300, 0), (0, 300),
           (1000, 1000)]
_ROTA = [("X", 2, 32), ("Y", 1, 64), ("X", 1, 64), ("U", 2, 128), ("X", 2, 128), ("S", 4, 64), ("X", 4, 32)]   # (set, Hkv, d)
# (set, H, Hkv, dtype, d, window): a covering selection, not the product; every window once per dtype
CASES = [(s, 4, hkv, dt, d, w) for i, w in enumerate(WINDOWS) for dt, (s, hkv, d) in (("bf16", _ROTA[i % 7]), ("f32", _ROTA[(i + 3) % 7]))]


def _cus(name):
    """(cu_q, Tq, cu_k, Tk) of a set."""
    nq, nk, (ql, qt), (kl, kt) = SETS[name]
    cu_q, Tq = pack(nq, ql, qt)
    cu_k, Tk = pack(nk, kl, kt) if nk is not None else (cu_q, Tq)
    return cu_q, Tq, cu_k, Tk


def _tck(name, cu_k):
    return None if SETS[name][1] is None else _i32(cu_k)


def _run(tq, tk, tv_, tdo, tcq, tck, window, scale=None):
    """The forward and the backward through device_ops: (out, lse, dq, dk, dv) device tensors."""
    from flash_attention_minitorch_amd import device_ops
    o, lse = device_ops.flash_attn_varlen_local_fwd(tq, tk, tv_, tcq, tck, window, scale)
    return (o, lse) + tuple(device_ops.flash_attn_varlen_local_bwd(tq, tk, tv_, o, tdo, lse, tcq, tck, window, scale))


def _direct(tq, tk, tv_, tdo, tcq, tck, window, scale=None):
    """The same through the library's C symbols, whatever the window: no Python routing."""
    torch = _torch()
    from flash_attention_minitorch_amd import _lib, device_ops
    lib = _lib.local()
    tck = tcq if tck is None else tck
    (Tq, H, d), (Tk, Hkv, _) = tq.shape, tk.shape
    geom = (tcq.numel() - 1, Tq, Tk, H, Hkv, d)
    ws = torch.empty(lib.fa_mi355x_bwd_local_workspace_bytes(*geom) // 4 + 1, device="cuda")
    out, lse = torch.empty((Tq, H, d), device="cuda"), torch.empty((H, Tq), device="cuda")
    dq, dk, dv = (torch.empty(t.shape, device="cuda") for t in (tq, tk, tk))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    tail = (p(tcq), p(tck), p(ws), *geom, float(scale or 0.0), window[0], window[1], int(tq.dtype == torch.bfloat16), device_ops._stream_ptr())
    _lib.local_check(lib.fa_mi355x_fwd_local(p(tq), p(tk), p(tv_), p(out), p(lse), *tail))
    _lib.local_check(lib.fa_mi355x_bwd_local(p(tq), p(tk), p(tv_), p(out), p(tdo), p(dq), p(dk), p(dv), p(lse), *tail))
    return out, lse, dq, dk, dv


def _host(ts):
    return [t.double().cpu().numpy() for t in ts]


def _zeros_where_nothing_is_admitted(got, cu_q, Tq, cu_k, Tk, window, what):
    lq, lk = local_live(cu_q, Tq, cu_k, Tk, *window)
    for n, g, qside in zip(NAMES, got, QSIDE):   # rows that admit no key, keys no row admits, keyless and queryless sequences, unowned rows
        assert np.all(_rows(n, g)[~(lq if qside else lk)] == 0), (what, n)


def test_the_cases_cover_every_set_every_window_in_both_dtypes_and_every_dtype_d_pair_with_groups_on_set_x():
    assert len(WINDOWS) == 14 and len(CASES) == 28
    assert {c[0] for c in CASES} == set(SETS)
    assert {(c[1], c[2]) for c in CASES} == {(4, 4), (4, 2), (4, 1)}
    pairs = {(t, d) for t in ("bf16", "f32") for d in (32, 64, 128)}
    assert {(c[3], c[4]) for c in CASES if c[0] == "X" and c[1] > c[2]} == pairs
    for w in WINDOWS:
        assert {c[3] for c in CASES if c[5] == w} == {"bf16", "f32"}, w
    assert [_cus(n)[1::2] for n in "XYUS"] == [(881, 1014), (1055, 1055), (300, 700), (700, 700)]
    deltas = [k - q for q, k in zip(*SETS["X"][:2]) if q and k]
    assert deltas == [76, 0, 43, 95, 23, -3, -130, 128] and 0 in SETS["X"][0] and 0 in SETS["X"][1]
    assert max(max(s[0]) for s in SETS.values()) <= 700 and max(max(s[1] or [0]) for s in SETS.values()) <= 700
    # what the windows are there for: rows without a key and keys without a row exist on set X under (5, 9)
    admit = local_admit(200, 70, 5, 9)
    assert (~admit.any(1)).sum() == 121 and not local_admit(40, 63, 5, 9)[:, :18].any() and local_admit(40, 63, 5, 9)[:, 18].any()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "{}-h{}kv{}-{}-d{}-w{}_{}".format(*c[:5], *c[5]))
def test_forward_and_backward_match_the_fp64_reference_per_sequence(case):
    name, H, Hkv, dtype, d, window = case
    cu_q, Tq, cu_k, Tk = _cus(name)
    q, k, v, do = _inputs(np.random.default_rng(Tq * 1000 + Tk + d), dtype, Tq, Tk, H, Hkv, d)
    got = _host(_run(*(_dev(a, dtype) for a in (q, k, v, do)), _i32(cu_q), _tck(name, cu_k), window))
    want = local_reference(q, k, v, do, cu_q, Tq, cu_k, Tk, *window)
    errs = {n: maxabs(g, w) for n, g, w in zip(NAMES, got, want)}
    print(case, {n: f"{e:.2e}" for n, e in errs.items()})
    assert all(np.all(np.isfinite(g)) for g in got), case
    assert all(e < TOL[dtype] for e in errs.values()), (case, errs, TOL[dtype])
    _zeros_where_nothing_is_admitted(got, cu_q, Tq, cu_k, Tk, window, case)


# ---- the windows that are existing masks: the new kernels against the existing calls ----

def _agree(mine, theirs, want, dtype, what):
    for n, a, b, w in zip(NAMES, _host(mine), _host(theirs), want):
        errs = (maxabs(a, b), maxabs(a, w), maxabs(b, w))
        print(what, n, " ".join(f"{e:.2e}" for e in errs))
        assert np.all(np.isfinite(a)) and errs[0] < 2 * TOL[dtype] and errs[1] < TOL[dtype] and errs[2] < TOL[dtype], (what, n, errs)


@pytest.mark.parametrize("dtype,d,Hkv", [("bf16", 64, 2), ("f32", 128, 1), ("bf16", 32, 4)])
def test_unbounded_on_both_sides_agrees_with_the_bidirectional_call(dtype, d, Hkv):
    cu_q, Tq, cu_k, Tk = _cus("X")
    q, k, v, do = _inputs(np.random.default_rng(d + Hkv), dtype, Tq, Tk, 4, Hkv, d)
    ts = [_dev(a, dtype) for a in (q, k, v, do)]
    tcq, tck = _i32(cu_q), _i32(cu_k)
    _agree(_direct(*ts, tcq, tck, (-1, -1)), bidir_run(*ts, tcq, tck), local_reference(q, k, v, do, cu_q, Tq, cu_k, Tk, -1, -1), dtype,
           ("bidir", dtype, d))


@pytest.mark.parametrize("name,dtype,d,Hkv", [("X", "bf16", 64, 2), ("X", "f32", 32, 1), ("U", "bf16", 128, 2), ("U", "f32", 64, 4)])
def test_unbounded_on_the_left_and_closed_on_the_right_agrees_with_the_causal_two_array_call(name, dtype, d, Hkv):
    cu_q, Tq, cu_k, Tk = _cus(name)
    q, k, v, do = _inputs(np.random.default_rng(d + Hkv), dtype, Tq, Tk, 4, Hkv, d)
    ts = [_dev(a, dtype) for a in (q, k, v, do)]
    tcq, tck = _i32(cu_q), _i32(cu_k)
    _agree(_direct(*ts, tcq, tck, (-1, 0)), tp._run(*ts, tcq, tck), local_reference(q, k, v, do, cu_q, Tq, cu_k, Tk, -1, 0), dtype,
           ("prefix", name, dtype, d))


@pytest.mark.parametrize("W", [1, 64, 200])
@pytest.mark.parametrize("dtype,d,Hkv", [("bf16", 64, 2), ("f32", 64, 1)])
def test_a_causal_window_on_one_array_agrees_with_the_packed_causal_call(dtype, d, Hkv, W):
    cu, T, _, _ = _cus("Y")
    q, k, v, do = _inputs(np.random.default_rng(W + d), dtype, T, T, 4, Hkv, d)
    ts = [_dev(a, dtype) for a in (q, k, v, do)]
    tcu = _i32(cu)
    _agree(_direct(*ts, tcu, None, (W - 1, 0)), tv._run(*ts, tcu, W, 0), local_reference(q, k, v, do, cu, T, cu, T, W - 1, 0), dtype,
           ("varlen", W, dtype))


@pytest.mark.parametrize("dtype,d", [("bf16", 64), ("f32", 32)])
def test_a_band_wider_than_the_sequence_is_the_unwindowed_problem(dtype, d):
    cu, T, _, _ = _cus("S")
    q, k, v, do = _inputs(np.random.default_rng(d), dtype, T, T, 4, 2, d)
    got = _host(_run(*(_dev(a, dtype) for a in (q, k, v, do)), _i32(cu), None, (1000, 1000)))
    for n, g, w in zip(NAMES, got, local_reference(q, k, v, do, cu, T, cu, T, -1, -1)):
        assert maxabs(g, w) < TOL[dtype], (n, maxabs(g, w))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_caller_scale_reaches_the_kernels(dtype):
    cu_q, Tq, cu_k, Tk = _cus("X")
    q, k, v, do = _inputs(np.random.default_rng(5), dtype, Tq, Tk, 4, 2, 64)
    got = _host(_run(*(_dev(a, dtype) for a in (q, k, v, do)), _i32(cu_q), _i32(cu_k), (31, 32), 0.2))
    for n, g, w in zip(NAMES, got, local_reference(q, k, v, do, cu_q, Tq, cu_k, Tk, 31, 32, 0.2)):
        assert maxabs(g, w) < TOL[dtype], (n, maxabs(g, w))
    default = local_reference(q, k, v, do, cu_q, Tq, cu_k, Tk, 31, 32)
    assert maxabs(got[0], default[0]) > 10 * TOL[dtype]   # (the scale is not the default's)


# ---- the law that defines the calls ----

@pytest.mark.parametrize("window", [(5, 9), (63, 64)], ids=lambda w: "w{}_{}".format(*w))
@pytest.mark.parametrize("dtype,d", [("bf16", 64), ("f32", 128)])
@pytest.mark.parametrize("name", ["X", "Y"])
def test_every_sequence_has_the_bits_of_the_same_call_on_that_sequence_alone(name, dtype, d, window):
    cu_q, Tq, cu_k, Tk = _cus(name)
    H, Hkv = 4, 2
    tq, tk, tv_, tdo = (_dev(a, dtype) for a in _inputs(np.random.default_rng(Tq + d), dtype, Tq, Tk, H, Hkv, d))
    got = _run(tq, tk, tv_, tdo, _i32(cu_q), _tck(name, cu_k), window)
    seen = 0
    for (sq, nq), (sk, nk) in zip(seq_rows(cu_q, Tq), seq_rows(cu_k, Tk)):
        if nq == 0 or nk == 0:
            continue
        one = [t[s:s + n].contiguous() for t, s, n in ((tq, sq, nq), (tk, sk, nk), (tv_, sk, nk), (tdo, sq, nq))]
        alone = _run(*one, _i32([0, nq]), _i32([0, nk]), window)
        for nm, g, a, qside in zip(NAMES, got, alone, QSIDE):
            s, n = (sq, nq) if qside else (sk, nk)
            mine = g[:, s:s + n] if nm == "lse" else g[s:s + n]
            assert _bits_equal(mine, a), (name, dtype, d, window, nm, (sq, nq, sk, nk), float((mine - a).abs().max()))
        seen += 1
    assert seen == sum(1 for a, b in zip(SETS[name][0], SETS[name][1] or SETS[name][0]) if a and b)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_two_calls_return_the_same_bits(dtype):
    cu_q, Tq, cu_k, Tk = _cus("X")
    ts = [_dev(a, dtype) for a in _inputs(np.random.default_rng(19), dtype, Tq, Tk, 4, 2, 64)]
    tcq, tck = _i32(cu_q), _i32(cu_k)
    first, second = _run(*ts, tcq, tck, (63, 64)), _run(*ts, tcq, tck, (63, 64))
    assert all(_bits_equal(a, b) for a, b in zip(first, second))


@pytest.mark.parametrize("name,dtype,d", [("X", "bf16", 64), ("X", "f32", 64), ("U", "f32", 32)])
def test_the_two_block_maps_in_the_workspace_are_the_models_whatever_the_window(name, dtype, d):
    torch = _torch()
    from flash_attention_minitorch_amd import _lib, device_ops
    cu_q, Tq, cu_k, Tk = _cus(name)
    H, Hkv = 4, 2
    tq, tk, tv_, tdo = (_dev(a, dtype) for a in _inputs(np.random.default_rng(3), dtype, Tq, Tk, H, Hkv, d))
    tcq, tck = _i32(cu_q), _i32(cu_k)
    map_q_bytes = _lib.local().fa_mi355x_fwd_local_workspace_bytes(len(cu_q) - 1, Tq, Tk, H, Hkv, d)
    seen = []
    for window in ((5, 9), (200, 100)):
        ws = device_ops.local_workspace(tq, tk, tcq, tck)
        ws.fill_(float("nan"))
        o, lse = device_ops.flash_attn_varlen_local_fwd(tq, tk, tv_, tcq, tck, window, workspace=ws)
        device_ops.flash_attn_varlen_local_bwd(tq, tk, tv_, o, tdo, lse, tcq, tck, window, workspace=ws)
        torch.cuda.synchronize()
        words = ws.view(torch.int32).cpu().numpy()
        for off, bs, keys in ((0, QBLOCK, False), (map_q_bytes // 4, key_block(dtype == "bf16", d), True)):
            want = block_map_model(cu_q, Tq, cu_k, Tk, bs, keys)
            got = words[off:off + want.size].reshape(want.shape)
            assert np.array_equal(got, want), (name, window, bs, got[:12], want[:12])
            seen.append(got.copy())
    assert np.array_equal(seen[0], seen[2]) and np.array_equal(seen[1], seen[3])   # the same maps under both windows


# ---- clamping ----

@pytest.mark.parametrize("bad,good", _CLAMP, ids=["past-q-neg-k", "neg-q-past-k", "decreasing-q", "decreasing-k", "extremes", "overlap"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_arrays_outside_the_buffers_are_clamped_and_nothing_outside_them_is_written(dtype, bad, good):
    """tests/test_gpu_bidir.py's bad arrays (Tq = 300, Tk = 200) under window (5, 9): no fault, every output finite, canary rows
    around every output untouched, the bits of the call on the clamped arrays, zeros wherever nothing is admitted."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    Tq, Tk, H, Hkv, d, C, window = 300, 200, 4, 2, 64, 8, (5, 9)
    tq, tk, tv_, tdo = (_dev(a, dtype) for a in _inputs(np.random.default_rng(7), dtype, Tq, Tk, H, Hkv, d))

    def call(cu_q, cu_k):
        """Every output sits between C canary rows (lse: one canary head on each side)."""
        full = [torch.full((T + 2 * C, h, d), 777.0, device="cuda") for T, h in ((Tq, H), (Tq, H), (Tk, Hkv), (Tk, Hkv))]
        lfull = torch.full((H + 2, Tq), 777.0, device="cuda")
        out, dq, dk, dv = (f[C:C + f.shape[0] - 2 * C] for f in full)
        lse = lfull[1:H + 1]
        tcq, tck = _i32(cu_q), _i32(cu_k)
        device_ops.flash_attn_varlen_local_fwd(tq, tk, tv_, tcq, tck, window, out=out, lse=lse)
        device_ops.flash_attn_varlen_local_bwd(tq, tk, tv_, out, tdo, lse, tcq, tck, window, grads=(dq, dk, dv))
        torch.cuda.synchronize()
        for f in full:
            assert bool((f[:C] == 777.0).all()) and bool((f[-C:] == 777.0).all())
        assert bool((lfull[0] == 777.0).all()) and bool((lfull[H + 1] == 777.0).all())
        return out, lse, dq, dk, dv
    res = call(*bad)
    assert all(bool(torch.isfinite(t).all()) for t in res)
    if good is not None:
        assert all(_bits_equal(a, b) for a, b in zip(res, call(*good)))
        _zeros_where_nothing_is_admitted([t.cpu().numpy() for t in res], np.array(good[0]), Tq, np.array(good[1]), Tk, window, "clamped")


# ---- autograd and the wrappers ----

def _grad_bound(dtype, want):
    """The gradients come back in the input dtype: bf16 (8 significant bits) adds one rounding, at most half an ulp = 2^-8 relative
    (tests/test_gpu_bidir.py::test_flash_attn_varlen_bidir_under_autograd)."""
    return TOL[dtype] + (2.0 ** -8 * float(np.max(np.abs(want))) if dtype == "bf16" else 0.0)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_flash_attn_varlen_local_under_autograd_with_a_padded_head_dim_and_a_callers_scale(dtype):
    from flash_attention_minitorch_amd import device_ops
    cu_q, Tq, cu_k, Tk = _cus("X")
    H, Hkv, d, scale, window = 4, 2, 80, 0.15, (31, 32)
    q, k, v, do = _inputs(np.random.default_rng(d), dtype, Tq, Tk, H, Hkv, d)
    tq, tk, tv_ = (_dev(a, dtype).requires_grad_() for a in (q, k, v))
    o = device_ops.flash_attn_varlen_local(tq, tk, tv_, _i32(cu_q), _i32(cu_k), window, scale)
    assert o.shape == (Tq, H, d)
    o.backward(_dev(do, "f32"))
    for t in (tq, tk, tv_):
        assert t.grad.dtype == t.dtype and t.grad.shape == t.shape
    want = local_reference(q, k, v, do, cu_q, Tq, cu_k, Tk, *window, scale)
    want = (want[0],) + want[2:]
    got = [t.detach().double().cpu().numpy() for t in (o, tq.grad, tk.grad, tv_.grad)]
    errs = [maxabs(g, w) for g, w in zip(got, want)]
    bound = [TOL[dtype]] + [_grad_bound(dtype, w) for w in want[1:]]
    print(errs, bound)
    assert all(e < b for e, b in zip(errs, bound)), (errs, bound)
    lq, lk = local_live(cu_q, Tq, cu_k, Tk, *window)
    assert all(np.all(g[~(lq if qside else lk)] == 0) for g, qside in zip(got, (True, True, False, False)))   # a zero gradient


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_flash_attn_local_matches_the_reference(dtype):
    from flash_attention_minitorch_amd import device_ops
    B, Nq, Nk, H, Hkv, d, window = 2, 40, 170, 4, 2, 64, (40, 3)
    q, k, v, do = _inputs(np.random.default_rng(11), dtype, B * Nq, B * Nk, H, Hkv, d)
    tq, tk, tv_ = (_dev(a, dtype).view(B, n, h, d).requires_grad_() for a, n, h in ((q, Nq, H), (k, Nk, Hkv), (v, Nk, Hkv)))
    o = device_ops.flash_attn_local(tq, tk, tv_, window)
    assert o.shape == (B, Nq, H, d) and o.dtype == _torch().float32
    o.backward(_dev(do, "f32").view(B, Nq, H, d))
    cu_q, cu_k = np.arange(B + 1) * Nq, np.arange(B + 1) * Nk
    want = local_reference(q, k, v, do, cu_q, B * Nq, cu_k, B * Nk, *window)
    want = (want[0],) + want[2:]
    got = [t.detach().double().cpu().numpy().reshape(w.shape) for t, w in zip((o, tq.grad, tk.grad, tv_.grad), want)]
    for g, w, grad in zip(got, want, (False, True, True, True)):
        assert maxabs(g, w) < (_grad_bound(dtype, w) if grad else TOL[dtype]), maxabs(g, w)
    assert not got[2].reshape(B, Nk, Hkv, d)[:, :Nk - Nq - 40].any()   # the keys j < D - L take no gradient


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_the_encoder_stack_with_a_local_and_a_global_layer_matches_the_same_stack_on_each_sequence_alone(dtype):
    """Two layers, window (64, 64) then none, rotary positions that restart at every sequence, two kv heads, unowned rows around the
    sequences.  The attention calls repeat bit for bit per sequence; the projections run on other row counts, so the comparison takes
    the model tolerance of tests/test_gpu_bidir.py's stack test (tests/test_gpu_extend.py: _model_tol)."""
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    from gpu_util import to_np
    from test_gpu_decode_append import _stack
    from test_gpu_extend import _model_tol
    E, H, Hkv, L, windows = 256, 4, 2, 2, [(64, 64), None]
    cu, T = pack([130, 31, 255, 64], 5, 19)
    x3, layers = _stack(np.random.default_rng(21), dtype, 1, E, H, Hkv, L, T)
    x = x3[0].contiguous()
    rope = mt.Rotary.table(512, E // H, device="cuda")
    dy = torch.from_numpy(rand_u(np.random.default_rng(4), (T, E))).to("cuda", _tdt(dtype))
    xg = x.clone().requires_grad_()
    y = mt.encoder_stack_packed(xg, _i32(cu), layers, H, rope=rope, window=windows)
    y.backward(dy)
    glob = mt.encoder_stack_packed(x, _i32(cu), layers, H, rope=rope)
    assert maxabs(to_np(y.detach()), to_np(glob)) > 1e-2   # (the window does something: 255 and 130 tokens do not fit a band of 129)
    own = np.zeros(T, bool)
    for s, n in seq_rows(cu, T):
        own[s:s + n] = True
        xs = x[s:s + n].clone().requires_grad_()
        ys = mt.encoder_stack_packed(xs, _i32([0, n]), layers, H, rope=rope, window=windows)
        ys.backward(dy[s:s + n])
        for got, want in ((y[s:s + n], ys), (xg.grad[s:s + n], xs.grad)):
            tol = _model_tol(dtype, to_np(want.detach()))
            assert maxabs(to_np(got.detach()), to_np(want.detach())) < tol, ((s, n), maxabs(to_np(got.detach()), to_np(want.detach())), tol)
    own = torch.from_numpy(own).cuda()
    assert _bits_equal(y[~own], x[~own])   # an unowned row: the residual alone


# ---- graph capture ----

def test_one_forward_and_backward_captured_in_a_graph_replays_on_new_data_and_new_lengths_in_both_arrays():
    """Neither array reaches the host and no grid knows the window's effect on a sequence: one capture under window (31, 32), then
    q, k, v, dO and BOTH arrays change IN PLACE and the replay equals the eager calls on the new data."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    dtype, H, Hkv, d, window = "bf16", 4, 2, 64, (31, 32)
    cu_q, Tq, cu_k, Tk = _cus("X")
    tq, tk, tv_, tdo = (_dev(a, dtype) for a in _inputs(np.random.default_rng(8), dtype, Tq, Tk, H, Hkv, d))
    tcq, tck = _i32(cu_q), _i32(cu_k)
    ws = device_ops.local_workspace(tq, tk, tcq, tck)
    out, lse = torch.empty((Tq, H, d), device="cuda"), torch.empty((H, Tq), device="cuda")
    grads = tuple(torch.empty((T, h, d), device="cuda") for T, h in ((Tq, H), (Tk, Hkv), (Tk, Hkv)))

    def call(o, l, g, w):
        device_ops.flash_attn_varlen_local_fwd(tq, tk, tv_, tcq, tck, window, out=o, workspace=w, lse=l)
        device_ops.flash_attn_varlen_local_bwd(tq, tk, tv_, o, tdo, l, tcq, tck, window, workspace=w, grads=g)
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
    tq.mul_(-0.5), tk.mul_(0.75), tv_.mul_(-1.0), tdo.mul_(0.5)
    g.replay()
    torch.cuda.synchronize()
    ro, rl = torch.empty_like(out), torch.empty_like(lse)
    rg = tuple(torch.empty_like(t) for t in grads)
    call(ro, rl, rg, device_ops.local_workspace(tq, tk, tcq, tck))
    torch.cuda.synchronize()
    for a, b in zip((out, lse) + grads, (ro, rl) + rg):
        assert _bits_equal(a, b) and not bool(torch.isnan(a).any())
    lq, lk = local_live(np.array(new_q), Tq, np.array(new_k), Tk, *window)
    tlq, tlk = torch.from_numpy(lq).cuda(), torch.from_numpy(lk).cuda()
    assert bool((out[~tlq] == 0).all()) and bool((out[tlq].abs().amax(dim=(1, 2)) > 0).all())
    assert bool((grads[1][~tlk] == 0).all()) and bool((grads[2][tlk].abs().amax(dim=(1, 2)) > 0).all())


# ---- scores beyond U(-1, 1) ----

SCORE_WINDOW = (63, 64)


@functools.lru_cache(maxsize=None)
def _large(family, dtype):
    """Set Y at d = 64, four query heads on two key heads, window (63, 64): tests/score_range.py's family, and for `spikes` further
    spiked keys on the two edges of the band of row i0 = n - 100 of every sequence above 200 rows (key i0 - 63: the last row that admits
    it is i0; key i0 + 64: the first is i0) beside the family's own on the edge between key tiles 0 and 1, on a diagonal and on the last
    key.  Returns the inputs and the fp64 reference, computed once."""
    cu, T, _, _ = _cus("Y")
    segments = [(s, n, s, n) for s, n in seq_rows(cu, T)]
    rng = np.random.default_rng(len(family) + (dtype == "bf16"))
    q, k, v, do = sr.family(family, rng, dtype, (T, sr.H, 64), (T, sr.HKV, 64), segments, 0, 0)
    if family == "spikes":
        for s, n, _, _ in segments:
            if n > 200:
                u = np.sign(k[s + n - 1])   # the family's sign vector per key head: its last key is a spike
                i0 = n - 100
                for j in (i0 - SCORE_WINDOW[0], i0 + SCORE_WINDOW[1]):
                    assert 0 <= j < n
                    k[s + j] = np.float32(6.0) * u
    want = local_reference(q, k, v, do, cu, T, cu, T, *SCORE_WINDOW)
    for w in want:
        w.setflags(write=False)
    return (q, k, v, do), want, cu, T


def _large_bounds(dtype, inputs, want, cu, T):
    """tests/test_gpu_score_range.py's: 5e-3 x max(1, max |reference tensor|) for bf16; for fp32 TOL["f32"], or where it is larger
    the fp32 rounding of the scores themselves, ln 2 x sqrt(d) x 2^-24 x max |S'| over the admitted pairs (S' in log2 units), times
    the same scale."""
    if dtype == "bf16":
        rel = 5e-3
    else:
        q, k = inputs[0].astype(np.float64), inputs[1].astype(np.float64)
        smax = 0.0
        for s, n in seq_rows(cu, T):
            admit = local_admit(n, n, *SCORE_WINDOW)
            for h in range(q.shape[1]):
                smax = max(smax, float(np.max(np.abs(np.where(admit, q[s:s + n, h] @ k[s:s + n, h // 2].T, 0.0)))))
        smax *= 1.4426950408889634 / 8.0
        rel = max(TOL["f32"], float(np.log(2.0) * 8.0 * 2.0 ** -24 * smax))
    return {n: rel * max(1.0, float(np.max(np.abs(w)))) for n, w in zip(NAMES, want)}


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("family", ["x6", "spikes"])
def test_large_scores_stay_inside_the_training_side_envelope(family, dtype):
    inputs, want, cu, T = _large(family, dtype)
    got = _host(_run(*(_dev(a, dtype) for a in inputs), _i32(cu), None, SCORE_WINDOW))
    bnd = _large_bounds(dtype, inputs, want, cu, T)
    errs = {n: maxabs(g, w) for n, g, w in zip(NAMES, got, want)}
    print(f"local_accuracy {family}-{dtype}-d64-setY-w63_64: " + " ".join(f"{n} {errs[n]:.3e} (bound {bnd[n]:.2e})" for n in NAMES))
    assert all(np.all(np.isfinite(g)) for g in got)
    assert all(errs[n] < bnd[n] for n in NAMES), (errs, bnd)
    _zeros_where_nothing_is_admitted(got, cu, T, cu, T, SCORE_WINDOW, (family, dtype))
