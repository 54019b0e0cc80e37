"""Learned sink logits on the GPU (fa_mi355x_fwd_decode_lsink / _extend_lsink / _ragged_lsink,
include/flash_attn_mi355x_decode_lsink.h) against the fp64 references of tests/test_lsink_cpu.py, a softmax over the admitted scores
plus one column, on the same (bf16-rounded) inputs at the family's own tolerances (fp32 1e-4, bf16 1e-3 max-abs on out and lse: the
sink column only shrinks P).  The cases and their inputs are tests/test_lsink_cpu.py's (kv_case), which shows on the CPU that every
one of them is at least 10 tolerances away from the call without the logits.  The caches are the front of larger NaN-filled buffers,
every row at or past a length holds NaN, out and lse are pre-filled with NaN.  Then the range (a = +-80, scores of tens), and the laws
that hold bit for bit: paged against slab, ragged against extend, fused against append-then-attend, null logits through the new C
entry points against the _window call, roped against apply_rotary, a graphed step against the eager one after the logits changed in
place; and a model on caches with logits against the dense stack."""
import ctypes
import math

import numpy as np
import pytest

from gpu_util import maxabs, to_np
from test_gpu_decode import _from_dev, _inputs, _tdt, _to_dev, _torch
from test_gpu_decode_append import _bits, _dev, _stack
from test_gpu_extend import _grouped_inputs, _model_tol
from test_gpu_paged import _dev_table, _pool, _table
from test_gpu_ragged import _cu, _i32, _nan_out, _packed, _rnd
from test_gpu_window import _caches, _nan_like, _new_tokens, _ops
from test_lsink_cpu import (COUNTS, GROUPS, HKV, KV_CASES, LENS, NCAP, RLENS, TAIL, TOL, WINDOWS, kv_case, kv_reference, lsink_reference,
                            ragged_lsink_reference)

pytestmark = pytest.mark.gpu

H = 4                                # (the bit-for-bit and range tests: a group of two)
MODES = [(True, 0), (True, 100), (False, 0)]   # (causal, window): a window needs the causal mask, the logits do not


def _f32(x):
    return _torch().from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def _splits(family, B, Hq, Nq, Ncap, d, W):
    from flash_attention_minitorch_amd import _lib
    return getattr(_lib.decode(), f"fa_mi355x_{family}_window_splits")(B, Hq, HKV, Nq, Ncap, d, 1, W)


def _kw(W, logits):
    return dict(sink_logits=logits, **(dict(window=W) if W else {}))


def _same(a, b):
    return bool(_torch().equal(_bits(a), _bits(b)))


# ---- parity with the fp64 reference ----

def _run_uniform(family, c, lens, W, layout, dtype, causal=True):
    torch = _torch()
    B, Hq, Nq, d = c["q"].shape
    tq = _to_dev(c["q"], layout, d, dtype)
    tk, tv = _caches(c["k"], c["v"], layout, d, dtype)
    out, lse = _nan_like(tq, B, Hq, Nq)
    got = _ops(family)(tq, tk, tv, _i32(lens), causal=causal, layout=layout, out=out, lse=lse, **_kw(W, _f32(c["logits"])))
    torch.cuda.synchronize()
    assert got[0] is out and got[1] is lse
    return _from_dev(out, layout), to_np(lse)


def _check_uniform(c, lens, W, dtype, out, lse, what):
    """out (B, H, Nq, d), lse (B, H, Nq) against the reference: all finite (with the logits no row is empty), inside the tolerance;
    a sequence of length 0: out = 0 and lse = its head's logit, exactly."""
    ro, rl = kv_reference(what[0], c, lens, W)
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(lse)), what
    eo, el = maxabs(out, ro), maxabs(lse, rl)
    assert eo < TOL[dtype] and el < TOL[dtype], (what, eo, el)
    for b, n in enumerate(lens):
        if n == 0:
            assert not out[b].any() and np.array_equal(lse[b], np.broadcast_to(c["logits"][:, None], lse[b].shape)), what


@pytest.mark.parametrize("G", GROUPS)
@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_decode_lsink_matches_fp64_reference(dtype, layout, d, G):
    """Nq = 1 and 5 at the lengths 1, 127, 128, 129, 300 and 0 of a 384-row cache, with and without a window of 64, and at a length
    of 2000 beside one of 3.  The unwindowed calls run as several splits (the logit enters in the combine kernel), the windowed ones
    on the short cache as one (the split kernel's own store): both occur, by the library's size query."""
    seen = set()
    for family, Nq, lens, Ncap in KV_CASES:
        if family != "decode":
            continue
        for W in WINDOWS:
            seen.add(_splits("decode", len(lens), G * HKV, Nq, Ncap, d, W) > 1)
            c = kv_case("decode", dtype, d, G, W, Nq, lens, Ncap)
            out, lse = _run_uniform("decode", c, lens, W, layout, dtype)
            _check_uniform(c, lens, W, dtype, out, lse, ("decode", Nq, Ncap, W))
    assert seen == {True, False}


@pytest.mark.parametrize("G", GROUPS)
@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_extend_lsink_matches_fp64_reference(dtype, layout, d, G):
    """Nq = 130: two 128-row blocks for G = 1 (a last one of two rows), five for G = 4; rows at negative positions (a length below
    130) admit no key: out = 0 and lse = the logit, which the tolerance holds."""
    for family, Nq, lens, Ncap in KV_CASES:
        if family != "extend":
            continue
        for W in WINDOWS:
            c = kv_case("extend", dtype, d, G, W, Nq, lens, Ncap)
            out, lse = _run_uniform("extend", c, lens, W, layout, dtype)
            _check_uniform(c, lens, W, dtype, out, lse, ("extend", Nq, Ncap, W))
            empty = np.arange(Nq)[None, :] < (Nq - np.minimum(np.asarray(lens), Ncap))[:, None]   # (B, Nq): positions below 0
            assert empty.any() and not out.transpose(0, 2, 1, 3)[empty].any()
            assert np.array_equal(lse.transpose(0, 2, 1)[empty], np.broadcast_to(c["logits"], (int(empty.sum()), G * HKV)))


@pytest.mark.parametrize("G", GROUPS)
@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_ragged_lsink_matches_fp64_reference(dtype, layout, d, G):
    """Counts 0, 1, 37, 130 with three unused tail rows: the rows no sequence owns are neither read nor written (they keep their
    NaN), the others are finite and inside the tolerance."""
    torch = _torch()
    for family, _, lens, Ncap in KV_CASES:
        if family != "ragged":
            continue
        for W in WINDOWS:
            c = kv_case("ragged", dtype, d, G, W, None, lens, Ncap)
            T, Hq = c["q"].shape[:2]
            tk, tv = _caches(c["k"], c["v"], layout, d, dtype)
            out, lse = _nan_out(T, Hq, d)
            _ops("ragged")(_packed(c["q"], dtype), tk, tv, _i32(c["cu"]), _i32(lens), causal=True, layout=layout, out=out, lse=lse,
                           **_kw(W, _f32(c["logits"])))
            torch.cuda.synchronize()
            out, lse = to_np(out), to_np(lse)
            ro, rl = kv_reference("ragged", c, lens, W)
            owned = ~np.isnan(rl[0])
            assert owned.sum() == sum(COUNTS) and (~owned).sum() == TAIL
            assert np.all(np.isnan(out[~owned])) and np.all(np.isnan(lse[:, ~owned]))
            assert np.all(np.isfinite(out[owned])) and np.all(np.isfinite(lse[:, owned]))
            eo, el = maxabs(out[owned], ro[owned]), maxabs(lse[:, owned], rl[:, owned])
            assert eo < TOL[dtype] and el < TOL[dtype], (W, eo, el)


# ---- the range ----

@pytest.mark.parametrize("a,amp", [(80.0, 1.0), (-80.0, 1.0), (0.0, 16.0)], ids=["a=+80", "a=-80", "qx16,a=0"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_lsink_stays_finite_at_the_ends_of_the_range(dtype, a, amp):
    """a = +80 (the sink takes nearly all of every row: out of the order of e^-75), a = -80 (the sink takes nothing: the call
    without logits, which is asserted at the plain tolerances) and q x 16 (exact in bf16) with a = 0 (scores of tens, the sink in
    the middle).  out and lse are finite and inside the project's large-magnitude envelope, 5e-3 x the tensor's scale."""
    torch = _torch()
    rng = np.random.default_rng([int(a) + 80, int(amp), dtype == "bf16"])
    d = 64
    logits = np.full(H, a, np.float32)
    for family, Nq in (("decode", 1), ("decode", 5), ("extend", 130)):
        for causal, W in MODES:
            q, k, v = _grouped_inputs(rng, dtype, len(LENS), H, HKV, Nq, NCAP, d, LENS)
            q = q * np.float32(amp)
            c = dict(q=q, k=k, v=v, logits=logits)
            out, lse = _run_uniform(family, c, LENS, W, "bnhd", dtype, causal)
            G = H // HKV
            B = len(LENS)
            ks, vs = (np.repeat(t, G, axis=1).reshape(B * H, NCAP, d) for t in (k, v))
            ro, rl = lsink_reference(q.reshape(B * H, Nq, d), ks, vs, np.repeat(LENS, H), W, 1.0 / math.sqrt(d), np.tile(logits, B), causal)
            ro, rl = ro.reshape(out.shape), rl.reshape(lse.shape)
            assert np.all(np.isfinite(out)) and np.all(np.isfinite(lse)), (family, Nq, causal, W)
            so, sl = max(1.0, float(np.max(np.abs(ro)))), max(1.0, float(np.max(np.abs(rl))))
            eo, el = maxabs(out, ro), maxabs(lse, rl)
            print(f"lsink_range {dtype} a={a:g} amp={amp:g} {family} Nq={Nq} causal={int(causal)} W={W}: out {eo:.3e} (scale {so:.2f}) "
                  f"lse {el:.3e} (scale {sl:.2f})")
            assert eo < 5e-3 * so and el < 5e-3 * sl, (family, Nq, causal, W, eo, el)
            if a == -80.0:   # the call without logits, at the plain tolerances, wherever that call has a key
                tq = _to_dev(q, "bnhd", d, dtype)
                tk, tv = _caches(k, v, "bnhd", d, dtype)
                o0, l0 = _ops(family)(tq, tk, tv, _i32(LENS), causal=causal, **(dict(window=W) if W else {}))
                torch.cuda.synchronize()
                o0, l0 = _from_dev(o0, "bnhd"), to_np(l0)
                fin = np.isfinite(l0)
                assert maxabs(out, o0) < TOL[dtype] and maxabs(lse[fin], l0[fin]) < TOL[dtype]
                assert np.all(lse[~fin] == -80.0)


# ---- bit for bit ----

def _ragged_case(rng, dtype, counts, lens, Ncap, d, tail=0):
    q = _rnd(rng, dtype, (sum(counts) + tail, H, d))
    _, k, v = _inputs(rng, dtype, len(counts), HKV, 1, Ncap, d, lens)
    return q, k, v, _cu(counts)


def _family_case(rng, dtype, family, layout, lens, Ncap, d, counts=None, Nq=None):
    """(device q, the arguments between the caches and the keywords, numpy k and v, the counts)."""
    if family == "ragged":
        q, k, v, cu = _ragged_case(rng, dtype, counts, lens, Ncap, d)
        return _packed(q, dtype), (_i32(cu), _i32(lens)), k, v, counts
    q, k, v = _grouped_inputs(rng, dtype, len(lens), H, HKV, Nq, Ncap, d, lens)
    return _to_dev(q, layout, d, dtype), (_i32(lens),), k, v, [Nq] * len(lens)


def _some_logits(rng):
    return _f32(rng.uniform(-1.0, 3.0, H))


@pytest.mark.parametrize("permuted", [False, True], ids=["identity", "permuted"])
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_paged_lsink_returns_the_slab_bits(dtype, layout, permuted):
    torch = _torch()
    rng = np.random.default_rng(128 + permuted + len(layout))
    d, ps = 64, 128
    mp = NCAP // ps
    a = _some_logits(rng)
    for family, Nq in (("decode", 1), ("decode", 5), ("extend", 130), ("ragged", None)):
        lens = RLENS if family == "ragged" else LENS
        tq, head, k, v, _ = _family_case(rng, dtype, family, layout, lens, NCAP, d, COUNTS, Nq)
        tk, tv = (_to_dev(t, layout, d, dtype) for t in (k, v))
        table, num_pages = _table(rng, len(lens), NCAP, ps, lens)
        if not permuted:
            table = np.arange(len(lens) * mp, dtype=np.int32).reshape(len(lens), mp)
        (kp, _), (vp, _) = (_pool(t, layout, ps, table, num_pages, None if not permuted else lens) for t in (tk, tv))
        for causal, W in MODES:
            want = _ops(family)(tq, tk, tv, *head, causal=causal, layout=layout, **_kw(W, a))
            got = _ops(family)(tq, kp, vp, *head, causal=causal, layout=layout, block_table=_dev_table(table), **_kw(W, a))
            plain = _ops(family)(tq, kp, vp, *head, causal=causal, layout=layout, block_table=_dev_table(table), **_kw(W, None))
            torch.cuda.synchronize()
            assert _same(got[0], want[0]) and _same(got[1], want[1]), (family, Nq, causal, W)
            assert not bool(torch.isnan(got[0]).any()) and not _same(got[1], plain[1])


@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_ragged_lsink_is_the_extend_lsink_call_on_each_sequence_alone(dtype, layout):
    """A cache of 256 rows is one split under both policies: the same bits per sequence."""
    rng = np.random.default_rng(43)
    d, Ncap, counts, lens = 64, 256, [0, 1, 37, 130, 5, 1], [100, 1, 256, 129, 9999, 0]
    T = sum(counts)
    a = _some_logits(rng)
    for causal, W in MODES:
        assert _splits("ragged", len(counts), H, T, Ncap, d, W) == 1
        q, k, v, cu = _ragged_case(rng, dtype, counts, lens, Ncap, d)
        tq, (tk, tv), tl = _packed(q, dtype), _caches(k, v, layout, d, dtype), _i32(lens)
        out, lse = _nan_out(T, H, d)
        _ops("ragged")(tq, tk, tv, _i32(cu), tl, causal=causal, layout=layout, out=out, lse=lse, **_kw(W, a))
        for b, nq in enumerate(counts):
            if nq == 0:
                continue
            s = int(cu[b])
            qb = tq[s:s + nq][None]
            if layout == "bhnd":
                qb = qb.transpose(1, 2).contiguous()
            assert _splits("extend", 1, H, nq, Ncap, d, W) == 1
            o, l = _ops("extend")(qb, tk[b:b + 1], tv[b:b + 1], tl[b:b + 1], causal=causal, layout=layout, **_kw(W, a))
            o = (o[0] if layout == "bnhd" else o[0].transpose(0, 1)).contiguous()
            assert _same(out[s:s + nq], o) and _same(lse[:, s:s + nq].contiguous(), l[0].contiguous()), (b, causal, W)
        ro, rl = ragged_lsink_reference(q, k, v, cu, lens, W, 1.0 / math.sqrt(d), to_np(a).astype(np.float64), causal)
        assert maxabs(to_np(out), ro) < TOL[dtype] and maxabs(to_np(lse), rl) < TOL[dtype]


@pytest.mark.parametrize("paged", [False, True], ids=["slab", "paged"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_fused_lsink_call_is_the_append_then_the_lsink_call(dtype, paged):
    """The rows the append writes hold NaN before it: the fused call returns the bits of append-then-attend, out and lse, and leaves
    the whole caches as the plain append leaves them."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    rng = np.random.default_rng(19 + paged)
    d, ps = 64, 128
    a = _some_logits(rng)
    appends = {"decode": device_ops.decode_append, "extend": device_ops.extend_append, "ragged": device_ops.ragged_append}
    for family, Nq in (("decode", 5), ("extend", 130), ("ragged", None)):
        lens = RLENS if family == "ragged" else LENS
        tq, head, k, v, counts = _family_case(rng, dtype, family, "bnhd", lens, NCAP, d, COUNTS, Nq)
        if family == "ragged":
            kn, vn = (_packed(_new_tokens(rng, dtype, (sum(counts), HKV, d)), dtype) for _ in range(2))
        else:
            kn, vn = (_dev(_new_tokens(rng, dtype, (len(lens), Nq, HKV, d)), "bnhd", dtype) for _ in range(2))
        for b, (n, nq) in enumerate(zip(lens, counts)):   # the new tokens' rows are not there yet
            n = min(max(n, 0), NCAP)
            k[b, :, max(n - nq, 0):n] = np.nan
            v[b, :, max(n - nq, 0):n] = np.nan
        tk, tv = (_to_dev(t, "bnhd", d, dtype) for t in (k, v))
        kw = {}
        if paged:
            table, num_pages = _table(rng, len(lens), NCAP, ps, lens)
            (tk, _), (tv, _) = (_pool(t, "bnhd", ps, table, num_pages, lens) for t in (tk, tv))
            kw = dict(block_table=_dev_table(table))
        for causal, W in MODES:
            k1, v1, k2, v2 = tk.clone(), tv.clone(), tk.clone(), tv.clone()
            appends[family](kn, vn, k1, v1, *head, **kw)
            o1, l1 = _ops(family)(tq, k1, v1, *head, causal=causal, **_kw(W, a), **kw)
            o2, l2 = _ops(family)(tq, k2, v2, *head, causal=causal, k_new=kn, v_new=vn, **_kw(W, a), **kw)
            torch.cuda.synchronize()
            for x, y in ((o1, o2), (l1, l2), (k1, k2), (v1, v2)):
                assert _same(x, y), (family, causal, W)
            assert not _same(k2, tk) and not bool(torch.isnan(o2).any())


def _c_call(family, tq, tk, tv, head, Nq, Ncap, d, causal, W, logits, dtype, ws):
    """The lsink C entry point itself, attend only on slab caches ("bnhd"), into fresh NaN-filled out and lse."""
    torch = _torch()
    from flash_attention_minitorch_amd import _lib
    B = tk.shape[0]
    out = torch.full(tq.shape, float("nan"), dtype=torch.float32, device="cuda")
    lse = torch.full((H, Nq) if family == "ragged" else (B, H, Nq), float("nan"), dtype=torch.float32, device="cuda")
    p = lambda t: ctypes.c_void_p(None if t is None else t.data_ptr())
    args = [p(tq), None, None, p(tk), p(tv), p(out), p(lse)] + [p(t) for t in head] + [None, p(ws), B, H, HKV, Nq, Ncap, 0, 0, 0, d, d,
                                                                                       _lib.FA_LAYOUT_BNHD, 0.0, int(causal), W, p(logits),
                                                                                       _lib.FA_DTYPE_BF16 if dtype == "bf16" else _lib.FA_DTYPE_F32,
                                                                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)]
    _lib.decode_check(getattr(_lib.decode(), f"fa_mi355x_fwd_{family}_lsink")(*args))
    torch.cuda.synchronize()
    return out, lse


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_null_logits_through_the_new_entry_points_are_the_window_call(dtype):
    """A null sink_logits is the _window call exactly (the same launches, splits, workspace and bits); and the entry point with
    logits is what device_ops calls."""
    from flash_attention_minitorch_amd import device_ops
    rng = np.random.default_rng(77)
    d = 64
    a = _some_logits(rng)
    sizes = {"decode": device_ops.decode_workspace, "extend": device_ops.extend_workspace, "ragged": device_ops.ragged_workspace}
    for family, Nq in (("decode", 5), ("extend", 130), ("ragged", None)):
        lens = RLENS if family == "ragged" else LENS
        tq, head, k, v, counts = _family_case(rng, dtype, family, "bnhd", lens, NCAP, d, COUNTS, Nq)
        n = tq.shape[0] if family == "ragged" else Nq
        tk, tv = (_to_dev(t, "bnhd", d, dtype) for t in (k, v))
        for W in (0, 100):
            ws = sizes[family](tq, tk, *head[:-1], window=W)
            want = _ops(family)(tq, tk, tv, *head, causal=True, window=W)   # (window = 0 included: the _window symbol)
            got = _c_call(family, tq, tk, tv, head, n, NCAP, d, True, W, None, dtype, ws)
            assert _same(got[0], want[0]) and _same(got[1], want[1]), (family, W)   # (every packed row is a sequence's: no tail here)
            with_a = _ops(family)(tq, tk, tv, *head, causal=True, **_kw(W, a))
            got = _c_call(family, tq, tk, tv, head, n, NCAP, d, True, W, a, dtype, ws)
            assert _same(got[0], with_a[0]) and _same(got[1], with_a[1]) and not _same(with_a[1], want[1]), (family, W)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_roped_lsink_call_is_the_lsink_call_on_rotated_q_and_k_new(dtype):
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    rng = np.random.default_rng(5)
    d, lens = 64, [3, 127, 128, 129, 300, 9999]
    a = _some_logits(rng)
    cos, sin = device_ops.rotary_table(NCAP, 32, device="cuda")
    for family, Nq in (("decode", 5), ("extend", 130)):
        lens_f = [max(n, Nq) for n in lens]
        tq, head, k, v, _ = _family_case(rng, dtype, family, "bnhd", lens_f, NCAP, d, None, Nq)
        kn, vn = (_dev(_new_tokens(rng, dtype, (len(lens), Nq, HKV, d)), "bnhd", dtype) for _ in range(2))
        tk, tv = (_to_dev(np.nan_to_num(t), "bnhd", d, dtype) for t in (k, v))
        offs = head[0].clamp(0, NCAP) - Nq
        qa, ka = (device_ops.apply_rotary(t, cos, sin, offs) for t in (tq, kn))
        for W in (0, 100):
            k1, v1, k2, v2 = tk.clone(), tv.clone(), tk.clone(), tv.clone()
            o1, l1 = _ops(family)(qa, k1, v1, *head, causal=True, k_new=ka, v_new=vn, **_kw(W, a))
            o2, l2 = _ops(family)(tq, k2, v2, *head, causal=True, k_new=kn, v_new=vn, rotary_cos=cos, rotary_sin=sin, **_kw(W, a))
            torch.cuda.synchronize()
            for x, y in ((o1, o2), (l1, l2), (k1, k2), (v1, v2)):
                assert _same(x, y), (family, W)
            assert not _same(qa, tq) and not bool(torch.isnan(o2).any())


# ---- the model ----

def _dense_lsink_stack(x, layers, n_head, W, logits):
    """The stack with its attention recomputed densely in torch fp32: the scores of all N x N pairs under the causal (and window)
    mask, one more column that holds the layer's logit of the head, the softmax over all of it, and P without that column on V."""
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    B, N, E = x.shape
    i = torch.arange(N, device=x.device)
    ok = i[None, :] <= i[:, None]
    if W:
        ok &= i[None, :] > i[:, None] - W
    for li, (wq, wk, wv, wo) in enumerate(layers):
        q, k, v = mt._project(x, wq, wk, wv, n_head)
        G = n_head // k.shape[2]
        qf, kf, vf = (t.float().permute(0, 2, 1, 3) for t in (q, k.repeat_interleave(G, 2), v.repeat_interleave(G, 2)))
        s = ((qf @ kf.transpose(2, 3)) * q.shape[3] ** -0.5).masked_fill(~ok, float("-inf"))
        if logits is not None:
            s = torch.cat([s, logits[li].float().view(1, n_head, 1, 1).expand(B, n_head, N, 1)], dim=-1)
        p = torch.softmax(s, dim=-1)[..., :N]
        o = (p @ vf).permute(0, 2, 1, 3)
        x = x + (o.reshape(B * N, E).to(x.dtype) @ wo).view(B, N, E)
    return x


@pytest.mark.parametrize("paged", [False, True], ids=["slab", "paged-window"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_model_on_a_cache_with_logits_matches_the_dense_stack(dtype, paged):
    """260 tokens through a 2-layer stack on KVCache(sink_logits=) and on PagedKVCache(window=, sink_logits=), every layer with its
    own logits: a prompt of 150 (the extend path: the square forward has no logit), 100 more at once, a ragged step, then single
    steps.  In fp32 the stack without the logits is many tolerances away (asserted)."""
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    E, L, B, N, W = 128, 2, 2, 260, 160 if paged else 0
    x, layers = _stack(np.random.default_rng(E + paged), dtype, B, E, H, HKV, L, N)
    logits = _f32(np.random.default_rng(9).uniform(-1.0, 3.0, (L, H)))
    want = to_np(_dense_lsink_stack(x, layers, H, W, logits))
    tol = _model_tol(dtype, want)
    if dtype == "f32":
        assert maxabs(want, to_np(_dense_lsink_stack(x, layers, H, W, None))) > 5 * tol   # (the logits matter at this tolerance)
    if paged:
        cache = mt.PagedKVCache(L, B, 384, H, E // H, _tdt(dtype), "cuda", n_kv_head=HKV, page_size=128, window=W, sink_logits=logits)
    else:
        cache = mt.KVCache(L, B, 384, H, E // H, _tdt(dtype), "cuda", n_kv_head=HKV, sink_logits=logits)
    got = [mt.attention_stack_prefill(x[:, :150].contiguous(), layers, H, cache),
           mt.attention_stack_extend(x[:, 150:250].contiguous(), layers, H, cache)]
    packed = torch.cat([x[0, 250:253], x[1, 250:253]]).contiguous()
    r = mt.attention_stack_ragged(packed, [3, 3], layers, H, cache)
    got.append(torch.stack([r[:3], r[3:6]]))
    for n in range(253, N):
        got.append(mt.attention_stack_step_fused(x[:, n:n + 1].contiguous(), layers, H, cache))
    assert cache.lengths.tolist() == [N] * B
    got = to_np(torch.cat(got, dim=1))
    assert maxabs(got, want) < tol, (maxabs(got, want), tol)


def test_graphed_step_replays_the_eager_fused_step_after_the_logits_changed_in_place():
    """The kernels read the logits on the device: a captured step replays with the values the tensor holds THEN.  Three steps, the
    logits raised by 1.5 in place, three more: the graph's output stays the eager step's bit for bit, and leaves the output of a
    cache that kept the first values."""
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    dtype, E, L, B, P, S = "bf16", 128, 2, 2, 250, 6
    x, layers = _stack(np.random.default_rng(31), dtype, B, E, H, HKV, L, P + S)
    assert _splits("decode", B, H, 1, 1024, E // H, 0) == 4   # (the steps run as four splits: the lsink combine build is in the graph)
    first = np.random.default_rng(4).uniform(-1.0, 3.0, (L, H))
    params = [_f32(first) for _ in range(3)]
    caches = [mt.KVCache(L, B, 1024, H, E // H, _tdt(dtype), "cuda", n_kv_head=HKV, sink_logits=p) for p in params]
    for c in caches:
        mt.attention_stack_prefill(x[:, :P].contiguous(), layers, H, c)
    graphed = mt.GraphedStep(layers, H, caches[0], T=1)
    for n in range(P, P + S):
        if n == P + 3:
            params[0].add_(1.5)
            params[1].add_(1.5)
        a = graphed.step(x[:, n:n + 1].contiguous()).clone()
        b = mt.attention_stack_step_fused(x[:, n:n + 1].contiguous(), layers, H, caches[1])
        c = mt.attention_stack_step_fused(x[:, n:n + 1].contiguous(), layers, H, caches[2])
        torch.cuda.synchronize()
        assert _same(a, b), n
        assert _same(b, c) == (n < P + 3), n
    assert caches[0].lengths.tolist() == caches[1].lengths.tolist() == [P + S] * B
