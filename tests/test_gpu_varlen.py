"""Packed variable-length forward and backward (libflash_attn_mi355x_varlen.so) on the GPU: against the fp64 reference of
tests/test_window_train_cpu.py run per sequence, against the window library on each sequence alone (bit for bit: the law of
include/flash_attn_mi355x_varlen.h), the block maps against the NumPy model of tests/test_varlen_cpu.py, clamping of a bad
cu_seqlens, the rotary embedding, autograd and the packed model functions.  Tolerances: the project's envelope, max-abs 1e-4 (fp32)
and 1e-3 (bf16) on out, lse, dq, dk and dv (tests/test_gpu_decode.py: TOL)."""
import numpy as np
import pytest

import oracle
from gpu_util import maxabs, rand_u, to_np
from test_gpu_decode import TOL
from test_varlen_cpu import QBLOCK, block_map_model, key_block, pack, seq_rows
from test_window_train_cpu import window_train_reference

pytestmark = pytest.mark.gpu

NAMES = ("out", "lse", "dq", "dk", "dv")
NO_WINDOW = 2 ** 31 - 1   # what the window library takes for "every j <= i"

# name -> (lengths, unowned rows in front, behind)
SETS = {
    "A": ([1, 129, 0, 128, 257, 33], 5, 19),
    "B": ([513, 31, 255, 256], 0, 0),
    "C": ([300], 0, 0),
    "D": ([(1, 2, 3, 31, 32)[i % 5] for i in range(40)], 0, 0),
}
MASKS = [(0, 0), (33, 0), (100, 5), (129, 33), (4096, 0)]   # (W, S); W = 0: no window; 4096: wider than every sequence


def _torch():
    import torch
    return torch


def _tdt(dtype):
    torch = _torch()
    return torch.bfloat16 if dtype == "bf16" else torch.float32


def _cu(name):
    lengths, lead, tail = SETS[name]
    return pack(lengths, lead, tail)


def _inputs(rng, dtype, T, H, Hkv, d):
    """q, k, v, do as packed (T, heads, d) float32 arrays, U(-1, 1), rounded to the dtype first."""
    rnd = (lambda s: oracle.bf16_round(rand_u(rng, s))) if dtype == "bf16" else (lambda s: rand_u(rng, s))
    return rnd((T, H, d)), rnd((T, Hkv, d)), rnd((T, Hkv, d)), rnd((T, H, d))


def _dev(a, dtype):
    return _torch().from_numpy(np.ascontiguousarray(a)).to("cuda", _tdt(dtype)).contiguous()


def _i32(a):
    torch = _torch()
    return torch.tensor([int(x) for x in a], dtype=torch.int32, device="cuda")


def _run(tq, tk, tv, tdo, tcu, W, S, scale=None):
    """The forward and the backward through device_ops: (out, lse, dq, dk, dv) device tensors."""
    from flash_attention_minitorch_amd import device_ops
    o, lse = device_ops.flash_attn_varlen_fwd(tq, tk, tv, tcu, W, S, scale)
    return (o, lse) + tuple(device_ops.flash_attn_varlen_bwd(tq, tk, tv, o, tdo, lse, tcu, W, S, scale))


def _reference(q, k, v, do, cu, T, W, S, scale=None):
    """The fp64 reference per sequence, concatenated: out (T, H, d), lse (H, T), dq, dk, dv; zeros in the rows no sequence owns."""
    H, Hkv, d = q.shape[1], k.shape[1], q.shape[2]
    out, dq = np.zeros((T, H, d)), np.zeros((T, H, d))
    lse, dk, dv = np.zeros((H, T)), np.zeros((T, Hkv, d)), np.zeros((T, Hkv, d))
    for s, n in seq_rows(cu, T):
        if n == 0:
            continue
        bhnd = lambda a: a[s:s + n].transpose(1, 0, 2)[None]
        ro, rl, rdq, rdk, rdv = window_train_reference(bhnd(q), bhnd(k), bhnd(v), bhnd(do), W or n, S, scale)
        out[s:s + n], dq[s:s + n] = ro[0].transpose(1, 0, 2), rdq[0].transpose(1, 0, 2)
        dk[s:s + n], dv[s:s + n] = rdk[0].transpose(1, 0, 2), rdv[0].transpose(1, 0, 2)
        lse[:, s:s + n] = rl[0]
    return out, lse, dq, dk, dv


def _owned(cu, T):
    own = np.zeros(T, bool)
    for s, n in seq_rows(cu, T):
        own[s:s + n] = True
    return own


def _rows(name, a, T):
    """A (T, ..) or (H, T) array with the packed rows first."""
    return a if name != "lse" else a.T


def _bits_equal(a, b):
    torch = _torch()
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)))


# (set, W, S, H, Hkv, dtype, d): a covering selection, not the product
CASES = [
    ("A", 100, 5, 4, 2, "bf16", 32), ("A", 100, 5, 4, 2, "bf16", 64), ("A", 129, 33, 4, 1, "bf16", 128),
    ("A", 100, 5, 4, 1, "f32", 32), ("A", 129, 33, 4, 2, "f32", 64), ("A", 100, 5, 4, 2, "f32", 128),
    ("A", 0, 0, 4, 4, "bf16", 64), ("A", 33, 0, 4, 4, "f32", 64),
    ("B", 0, 0, 4, 2, "bf16", 128), ("B", 33, 0, 4, 4, "bf16", 32), ("B", 4096, 0, 4, 1, "f32", 32), ("B", 100, 5, 4, 2, "f32", 64),
    ("C", 129, 33, 4, 4, "bf16", 64), ("C", 0, 0, 4, 2, "f32", 128),
    ("D", 100, 5, 4, 2, "bf16", 64), ("D", 0, 0, 4, 4, "f32", 32), ("D", 4096, 0, 4, 1, "bf16", 128),
]


def test_the_cases_cover_every_axis_value_and_every_dtype_d_pair_with_a_sink_with_groups_and_with_set_a():
    assert {c[0] for c in CASES} == set(SETS) and {(c[1], c[2]) for c in CASES} == set(MASKS)
    assert {(c[3], c[4]) for c in CASES} == {(4, 4), (4, 2), (4, 1)}
    pairs = {(t, d) for t in ("bf16", "f32") for d in (32, 64, 128)}
    assert {(c[5], c[6]) for c in CASES if c[2] > 0} == pairs
    assert {(c[5], c[6]) for c in CASES if c[3] > c[4]} == pairs
    assert {(c[5], c[6]) for c in CASES if c[0] == "A"} == pairs
    assert [sum(SETS[n][0]) + SETS[n][1] + SETS[n][2] for n in "ABCD"] == [572, 1055, 300, 552] and len(SETS["D"][0]) == 40


@pytest.mark.parametrize("case", CASES, ids=lambda c: "{}-W{}-S{}-h{}kv{}-{}-d{}".format(*c))
def test_forward_and_backward_match_the_fp64_reference_per_sequence(case):
    name, W, S, H, Hkv, dtype, d = case
    cu, T = _cu(name)
    q, k, v, do = _inputs(np.random.default_rng(T * 1000 + W + S + d), dtype, T, H, Hkv, d)
    got = [t.double().cpu().numpy() for t in _run(*(_dev(a, dtype) for a in (q, k, v, do)), _i32(cu), W, S)]
    want = _reference(q, k, v, do, cu, T, W, S)
    errs = {n: maxabs(g, w) for n, g, w in zip(NAMES, got, want)}
    print(case, {n: f"{e:.2e}" for n, e in errs.items()})
    assert all(np.all(np.isfinite(g)) for g in got), case
    assert all(e < TOL[dtype] for e in errs.values()), (case, errs, TOL[dtype])
    own = _owned(cu, T)
    for n, g in zip(NAMES, got):   # rows no sequence owns: exactly zero
        assert np.all(_rows(n, g, T)[~own] == 0), (case, n)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_caller_scale_reaches_the_kernels(dtype):
    cu, T = _cu("A")
    q, k, v, do = _inputs(np.random.default_rng(5), dtype, T, 4, 2, 64)
    got = [t.double().cpu().numpy() for t in _run(*(_dev(a, dtype) for a in (q, k, v, do)), _i32(cu), 100, 5, 0.2)]
    for n, g, w in zip(NAMES, got, _reference(q, k, v, do, cu, T, 100, 5, 0.2)):
        assert maxabs(g, w) < TOL[dtype], (n, maxabs(g, w))


# ---- the law that defines the calls ----

@pytest.mark.parametrize("W,S,d", [(0, 0, 128), (100, 5, 64), (33, 0, 32)], ids=["none-d128", "W100-S5-d64", "W33-d32"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_every_sequence_has_the_bits_of_the_window_library_on_that_sequence_alone(name, dtype, W, S, d):
    from flash_attention_minitorch_amd import device_ops
    cu, T = _cu(name)
    H, Hkv = 4, 2
    tq, tk, tv, tdo = (_dev(a, dtype) for a in _inputs(np.random.default_rng(T + W + d), dtype, T, H, Hkv, d))
    got = _run(tq, tk, tv, tdo, _i32(cu), W, S)
    seen = 0
    for s, n in seq_rows(cu, T):
        if n == 0:
            continue
        one = [t[s:s + n][None].contiguous() for t in (tq, tk, tv, tdo)]
        o, lse = device_ops.flash_attn_fwd_window(one[0], one[1], one[2], W or NO_WINDOW, S)
        dq, dk, dv = device_ops.flash_attn_bwd_window(one[0], one[1], one[2], o, one[3], lse, W or NO_WINDOW, S)
        alone = (o[0], lse[0], dq[0], dk[0], dv[0])
        for nm, g, a in zip(NAMES, got, alone):
            mine = g[:, s:s + n] if nm == "lse" else g[s:s + n]
            assert _bits_equal(mine, a), (name, dtype, W, S, d, nm, (s, n), float((mine - a).abs().max()))
        seen += 1
    assert seen == sum(1 for x in SETS[name][0] if x)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_two_calls_return_the_same_bits(dtype):
    cu, T = _cu("A")
    ts = [_dev(a, dtype) for a in _inputs(np.random.default_rng(19), dtype, T, 4, 2, 64)]
    tcu = _i32(cu)
    first, second = _run(*ts, tcu, 100, 5), _run(*ts, tcu, 100, 5)
    assert all(_bits_equal(a, b) for a, b in zip(first, second))


# ---- the schedule launch against the model ----

@pytest.mark.parametrize("name,dtype,d", [("A", "bf16", 64), ("A", "f32", 64), ("D", "bf16", 32), ("D", "bf16", 128)])
def test_the_block_maps_in_the_workspace_are_the_models(name, dtype, d):
    torch = _torch()
    from flash_attention_minitorch_amd import _lib, device_ops
    cu, T = _cu(name)
    H, Hkv = 4, 2
    tq, tk, tv, tdo = (_dev(a, dtype) for a in _inputs(np.random.default_rng(3), dtype, T, H, Hkv, d))
    tcu = _i32(cu)
    ws = device_ops.varlen_workspace(tq, tk, tcu)
    ws.fill_(float("nan"))
    o, lse = device_ops.flash_attn_varlen_fwd(tq, tk, tv, tcu, 100, 5, workspace=ws)
    device_ops.flash_attn_varlen_bwd(tq, tk, tv, o, tdo, lse, tcu, 100, 5, workspace=ws)
    torch.cuda.synchronize()
    words = ws.view(torch.int32).cpu().numpy()
    nseq = len(cu) - 1
    map_bytes = _lib.varlen().fa_mi355x_fwd_varlen_workspace_bytes(nseq, T, H, Hkv, d)
    for off, bs in ((0, QBLOCK), (map_bytes // 4, key_block(dtype == "bf16", d))):
        want = block_map_model(cu, T, bs)
        got = words[off:off + want.size].reshape(want.shape)
        assert np.array_equal(got, want), (name, bs, got[:12], want[:12])


# ---- clamping ----

@pytest.mark.parametrize("bad,good", [([0, 200, 9999], [0, 200, 300]), ([-7, 100, 300], [0, 100, 300])])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_cu_seqlens_outside_the_buffers_is_clamped_and_nothing_outside_them_is_written(dtype, bad, good):
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    T, H, Hkv, d, C = 300, 4, 2, 64, 8
    tq, tk, tv, tdo = (_dev(a, dtype) for a in _inputs(np.random.default_rng(7), dtype, T, H, Hkv, d))

    def call(cu):
        """Every output sits between C canary rows (lse: one canary head on each side)."""
        full = [torch.full((T + 2 * C, h, d), 777.0, device="cuda") for h in (H, H, Hkv, Hkv)]
        lfull = torch.full((H + 2, T), 777.0, device="cuda")
        out, dq, dk, dv = (f[C:C + T] for f in full)
        lse = lfull[1:H + 1]
        tcu = _i32(cu)
        device_ops.flash_attn_varlen_fwd(tq, tk, tv, tcu, 100, 5, out=out, lse=lse)
        device_ops.flash_attn_varlen_bwd(tq, tk, tv, out, tdo, lse, tcu, 100, 5, grads=(dq, dk, dv))
        torch.cuda.synchronize()
        for f in full:
            assert bool((f[:C] == 777.0).all()) and bool((f[C + T:] == 777.0).all())
        assert bool((lfull[0] == 777.0).all()) and bool((lfull[H + 1] == 777.0).all())
        return out, lse, dq, dk, dv
    assert all(_bits_equal(a, b) for a, b in zip(call(bad), call(good)))


# ---- rotary ----

@pytest.mark.parametrize("rot,interleaved", [(64, False), (32, False), (64, True), (16, True), (6, False)])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_apply_rotary_varlen_is_apply_rotary_on_each_sequence_alone(dtype, rot, interleaved):
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    cu, T = _cu("A")
    H, d = 3, 64
    x = _dev(_inputs(np.random.default_rng(rot), dtype, T, H, H, d)[0], dtype)
    cos, sin = device_ops.rotary_table(200, rot, device="cuda")   # (shorter than the longest sequence: positions are clamped)
    tcu = _i32(cu)
    y = device_ops.apply_rotary_varlen(x, cos, sin, tcu, interleaved)
    own = _owned(cu, T)
    assert _bits_equal(y[torch.from_numpy(~own).cuda()], x[torch.from_numpy(~own).cuda()])   # unowned rows: copied
    for s, n in seq_rows(cu, T):
        if n:
            alone = device_ops.apply_rotary(x[s:s + n][None].contiguous(), cos, sin, None, interleaved)
            assert _bits_equal(y[s:s + n], alone[0]), (s, n)
    # in place, and the inverse
    z = x.clone()
    assert device_ops.apply_rotary_varlen(z, cos, sin, tcu, interleaved, out=z) is z and _bits_equal(z, y)
    back = device_ops.apply_rotary_varlen(y, cos, sin, tcu, interleaved, inverse=True)
    assert maxabs(to_np(back), to_np(x)) < (2e-2 if dtype == "bf16" else 1e-6)
    # autograd: the backward is the inverse rotation of the cotangent
    xg = x.clone().requires_grad_()
    g = _dev(_inputs(np.random.default_rng(1), dtype, T, H, H, d)[0], dtype)
    device_ops.apply_rotary_varlen(xg, cos, sin, tcu, interleaved).backward(g)
    assert _bits_equal(xg.grad, device_ops.apply_rotary_varlen(g, cos, sin, tcu, interleaved, inverse=True))


# ---- autograd ----

@pytest.mark.parametrize("d,dtype", [(64, "bf16"), (80, "bf16"), (80, "f32")])
def test_flash_attn_varlen_under_autograd(d, dtype):
    """flash_attn_varlen and .backward() against the reference's gradients; d = 80 through the zero padding.  The bound is that of
    tests/test_gpu_window_train.py::test_flash_attn_gqa_window_under_autograd: the gradients come back in the input dtype, and bf16
    (8 significant bits) adds one rounding, at most half an ulp = 2^-8 relative."""
    from flash_attention_minitorch_amd import device_ops
    cu, T = _cu("A")
    H, Hkv, W, S = 4, 2, 50, 4
    q, k, v, do = _inputs(np.random.default_rng(d), dtype, T, H, Hkv, d)
    tq, tk, tv = (_dev(a, dtype).requires_grad_() for a in (q, k, v))
    o = device_ops.flash_attn_varlen(tq, tk, tv, _i32(cu), window=W, sink=S)
    assert o.shape == (T, H, d)
    o.backward(_dev(do, "f32"))
    assert tq.grad.dtype == tq.dtype and tk.grad.shape == tk.shape
    want = _reference(q, k, v, do, cu, T, W, S)
    got = [t.detach().double().cpu().numpy() for t in (o, tq.grad, tk.grad, tv.grad)]
    tol = TOL[dtype]
    errs = [maxabs(g, w) for g, w in zip(got, (want[0], want[2], want[3], want[4]))]
    bound = [tol] + [tol + (2.0 ** -8 * float(np.max(np.abs(w))) if dtype == "bf16" else 0.0) for w in want[2:]]
    print(errs, bound)
    assert all(e < b for e, b in zip(errs, bound)), (errs, bound)
    own = _owned(cu, T)
    assert all(np.all(g[~own] == 0) for g in got)   # an unused row takes a zero gradient


# ---- the model functions ----

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_attention_stack_packed_matches_attention_stack_on_each_sequence_alone(dtype):
    """Two layers, rotary positions that restart at every sequence, W = 100, S = 5, two kv heads, set A without its empty sequence.
    The tolerance is the model tolerance tests/test_gpu_window_train_model.py applies to its two paths (tests/test_gpu_extend.py:
    _model_tol): a sequence shorter than the window runs attention_stack's unwindowed kernels, other kernels than the packed call's."""
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    from test_gpu_decode_append import _stack
    from test_gpu_extend import _model_tol
    E, H, Hkv, L, W, S = 256, 4, 2, 2, 100, 5
    lengths, lead, tail = SETS["A"]
    cu, T = pack([n for n in lengths if n], lead, tail)
    x3, layers = _stack(np.random.default_rng(W + S), dtype, 1, E, H, Hkv, L, T)
    x = x3[0].contiguous()
    rope = mt.Rotary.table(512, E // H, device="cuda")
    dy = torch.from_numpy(rand_u(np.random.default_rng(4), (T, E))).to("cuda", _tdt(dtype))
    xg = x.clone().requires_grad_()
    y = mt.attention_stack_packed(xg, _i32(cu), layers, H, rope=rope, window=W, sink=S)
    y.backward(dy)
    for s, n in seq_rows(cu, T):
        xs = x[s:s + n][None].clone().requires_grad_()
        ys = mt.attention_stack(xs, layers, H, rope=rope, window=W, sink=S)
        ys.backward(dy[s:s + n][None])
        for got, want in ((y[s:s + n], ys[0]), (xg.grad[s:s + n], xs.grad[0])):
            tol = _model_tol(dtype, to_np(want))
            assert maxabs(to_np(got), to_np(want)) < tol, ((s, n), maxabs(to_np(got), to_np(want)), tol)
    own = torch.from_numpy(_owned(cu, T)).cuda()
    assert _bits_equal(y[~own], x[~own])   # an unowned row: the residual alone


def test_one_forward_and_backward_captured_in_a_graph_replays_on_new_data_and_new_lengths():
    """cu_seqlens never reaches the host: one capture, then q, k, v, dO and cu_seqlens change IN PLACE (other lengths, another
    number of unowned rows) and the replay equals the eager calls on the new data."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    dtype, H, Hkv, d, W, S = "bf16", 4, 2, 64, 100, 5
    cu, T = _cu("A")
    tq, tk, tv, tdo = (_dev(a, dtype) for a in _inputs(np.random.default_rng(8), dtype, T, H, Hkv, d))
    tcu = _i32(cu)
    ws = device_ops.varlen_workspace(tq, tk, tcu)
    out, lse = torch.empty((T, H, d), device="cuda"), torch.empty((H, T), device="cuda")
    grads = tuple(torch.empty((T, h, d), device="cuda") for h in (H, Hkv, Hkv))

    def call(o, l, g, w):
        device_ops.flash_attn_varlen_fwd(tq, tk, tv, tcu, W, S, out=o, workspace=w, lse=l)
        device_ops.flash_attn_varlen_bwd(tq, tk, tv, o, tdo, l, tcu, W, S, workspace=w, grads=g)
    call(out, lse, grads, ws)   # (the library is loaded and has launched once before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):   # one stream: schedule, forward, schedule, row constants, dK/dV, group sum, dQ
        call(out, lse, grads, ws)
    for t in (out, lse) + grads:
        t.fill_(float("nan"))
    tcu.copy_(_i32([0, 300, 301, 301, 430, 431, 560]))
    tq.mul_(-0.5), tk.mul_(0.75), tv.mul_(-1.0), tdo.mul_(0.5)
    g.replay()
    torch.cuda.synchronize()
    ro, rl = torch.empty_like(out), torch.empty_like(lse)
    rg = tuple(torch.empty_like(t) for t in grads)
    call(ro, rl, rg, device_ops.varlen_workspace(tq, tk, tcu))
    torch.cuda.synchronize()
    for a, b in zip((out, lse) + grads, (ro, rl) + rg):
        assert _bits_equal(a, b) and not bool(torch.isnan(a).any())
    assert bool((out[560:] == 0).all()) and bool((out[:560].abs().amax(dim=(1, 2)) > 0).all())
