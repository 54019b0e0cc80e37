"""Attention-sink tokens on the GPU (fa_mi355x_fwd_decode_sink / _extend_sink / _ragged_sink, include/flash_attn_mi355x_decode_sink.h)
against the fp64 references of tests/test_sink_cpu.py on the same (bf16-rounded) inputs, at the project's tolerances (TOL of
tests/test_gpu_decode.py: fp32 1e-4, bf16 1e-3 max-abs on out and lse, the -inf pattern of lse exact).  The NaN discipline of
tests/test_gpu_window.py: the caches are the front of larger NaN-filled buffers, every row at or past a length holds NaN, out and lse
are pre-filled with NaN -- and every cache row from S up to a sequence's lowest window edge holds NaN too, so one read between the
sinks and the window shows.  Then: the bits of the windowed call at sink = 0 and of the unwindowed call where the window or the
sinks cover the cache; the bits of the slab call through a block table, with the slots between the sink slots and the window invalid
and their pages NaN; ragged against extend per sequence; the fused forms; a paged model with sinks that gives its pages back and
keeps its sink page; graph capture."""
import math

import numpy as np
import pytest

from gpu_util import maxabs, to_np
from test_gpu_decode import TOL, _from_dev, _inputs, _tdt, _to_dev, _torch
from test_gpu_decode_append import _bits, _dev, _stack
from test_gpu_extend import _grouped_inputs, _model_tol, _nan_buffer
from test_gpu_paged import _dev_table, _pool, _table
from test_gpu_ragged import COUNTS, LENS, _cu, _i32, _nan_out, _packed, _rnd
from test_gpu_window import _new_tokens, _nan_like, _picked
from test_sink_cpu import (DECODE_NQ, EXTEND_NQ, GPU_SPLITS, NCAP, RAGGED_T, grid_heads, grid_lens, grid_pairs, ragged_sink_reference,
                           sink_reference)

pytestmark = pytest.mark.gpu


def _ops(family):
    from flash_attention_minitorch_amd import device_ops
    return {"decode": device_ops.flash_attn_decode, "extend": device_ops.flash_attn_extend, "ragged": device_ops.flash_attn_ragged}[family]


def _splits(family, B, H, Hkv, Nq, Ncap, d, W, S):
    from flash_attention_minitorch_amd import _lib
    return getattr(_lib.decode(), f"fa_mi355x_{family}_sink_splits")(B, H, Hkv, Nq, Ncap, d, 1, W, S)


def _edge(n, nq, W, Ncap):
    """The lowest key the window of any query of a sequence of (clamped) length n with nq new tokens admits."""
    return max(min(max(n, 0), Ncap) - nq - W + 1, 0) if W > 0 else 0


def _nan_between(k, v, lens, counts, W, S):
    """NaN in every cache row S <= j < each sequence's lowest window edge (k, v (B, Hkv, Ncap, d), in place)."""
    for b, (n, nq) in enumerate(zip(lens, counts)):
        if nq > 0 and W > 0:
            e = _edge(n, nq, W, k.shape[2])
            k[b, :, S:e] = np.nan
            v[b, :, S:e] = np.nan


def _caches(k, v, layout, dp, dtype):
    return tuple(_to_dev(t, layout, dp, dtype, _nan_buffer(t, dp, dtype)) for t in (k, v))


def _uniform(family, q, k, v, lens, W, S, layout, dtype, dp, **kw):
    """flash_attn_decode / flash_attn_extend with window=W, sink=S on numpy q (B, H, Nq, d), k / v (B, Hkv, Ncap, d) into NaN-filled
    out and lse.  Returns numpy (out (B, H, Nq, d), lse (B, H, Nq))."""
    torch = _torch()
    B, H, Nq, d = q.shape
    tq = _to_dev(q, layout, d, dtype)
    tk, tv = _caches(k, v, layout, dp, dtype)
    out, lse = _nan_like(tq, B, H, Nq)
    got = _ops(family)(tq, tk, tv, _i32(lens), causal=True, layout=layout, out=out, lse=lse, window=W, sink=S, **kw)
    torch.cuda.synchronize()
    assert got[0] is out and got[1] is lse
    return _from_dev(out, layout), to_np(lse)


def _check_uniform(q, k, v, lens, W, S, dtype, out, lse, heads=None):
    """out (B, H, Nq, d), lse (B, H, Nq) against sink_reference: every value finite (no NaN came in from between the sinks and the
    window, from past a length or from an unwritten row), the -inf pattern of lse exact, the values within the tolerance."""
    B, H, Nq, d = q.shape
    G = H // k.shape[1]
    assert np.all(np.isfinite(out)) and not np.any(np.isnan(lse)), (W, S)
    for b in range(B):
        for h in (range(H) if heads is None else heads):
            ro, rl = sink_reference(q[b, h][None], k[b, h // G][None], v[b, h // G][None], [lens[b]], W, S, 1.0 / math.sqrt(d))
            assert np.array_equal(np.isneginf(lse[b, h]), np.isneginf(rl[0])), (b, h, W, S)
            fin = np.isfinite(rl[0])
            assert maxabs(out[b, h], ro[0]) < TOL[dtype], (b, h, W, S, maxabs(out[b, h], ro[0]))
            if fin.any():
                assert maxabs(lse[b, h][fin], rl[0][fin]) < TOL[dtype], (b, h, W, S)


def _uniform_case(rng, dtype, H, Hkv, Nq, d, lens, W, S, Ncap=NCAP):
    q, k, v = _grouped_inputs(rng, dtype, len(lens), H, Hkv, Nq, Ncap, d, lens)
    _nan_between(k, v, lens, [Nq] * len(lens), W, S)
    return q, k, v


def _grid(family, dtype, layout, d, ni, Nq):
    """The (S, W) pairs of this case (grid_pairs: a rotating half of the cross product) at every length of grid_lens, G cycling through
    1, 4, 8 (the split count of every call is held against the policy in tests/test_sink_cpu.py).  Returns the set of (several
    splits?) seen."""
    rng = np.random.default_rng(d + (7 if dtype == "bf16" else 0) + len(family) + Nq)
    dp = {80: 128}.get(d, d)
    seen = set()
    for pi, S, W in grid_pairs(d, ni):
        H, Hkv = grid_heads(pi, d)
        lens = grid_lens(S, W)
        ns = _splits(family, len(lens), H, Hkv, Nq, NCAP, dp, W, S)
        seen.add(ns > 1)
        assert all(p[1] == ns for p in GPU_SPLITS if p[0] == (family, len(lens), H, Hkv, Nq, NCAP, dp, W, S))
        q, k, v = _uniform_case(rng, dtype, H, Hkv, Nq, d, lens, W, S)
        out, lse = _uniform(family, q, k, v, lens, W, S, layout, dtype, dp)
        _check_uniform(q, k, v, lens, W, S, dtype, out, lse, heads=_picked(H, Hkv))
    return seen


@pytest.mark.parametrize("d", [32, 64, 128, 80])
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_decode_sink_matches_fp64_reference_at_the_edges(dtype, layout, d):
    """Sinks inside one 32-key sub-tile, on a tile boundary, across tiles; the jump from the sink tiles to the window's range inside a
    chunk and on a chunk boundary; adjacent and overlapping ranges; lengths below S; rows at negative positions; one split and
    several (the combine launch)."""
    seen = set()
    for ni, Nq in enumerate(DECODE_NQ):
        seen |= _grid("decode", dtype, layout, d, ni, Nq)
    assert seen == {True, False}


@pytest.mark.parametrize("ni,Nq", list(enumerate(EXTEND_NQ)))
@pytest.mark.parametrize("d", [32, 64, 128, 80])
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_extend_sink_matches_fp64_reference_at_the_edges(dtype, layout, d, ni, Nq):
    """... and row blocks whose window ranges start at different tiles behind the same sink tiles, waves of one block with different
    window edges."""
    assert _grid("extend", dtype, layout, d, ni, Nq) <= {True, False}


def _ragged_case(rng, dtype, H, Hkv, counts, lens, Ncap, d, W, S, tail=0):
    q = _rnd(rng, dtype, (sum(counts) + tail, H, d))
    _, k, v = _inputs(rng, dtype, len(counts), Hkv, 1, Ncap, d, lens)
    _nan_between(k, v, lens, counts, W, S)
    return q, k, v, _cu(counts)


def _check_ragged(q, k, v, cu, lens, W, S, dtype, out, lse):
    out, lse = to_np(out), to_np(lse)
    ro, rl = ragged_sink_reference(q, k, v, cu, lens, W, S, 1.0 / math.sqrt(q.shape[2]))
    owned = ~np.isnan(rl[0])
    assert owned.sum() == int(cu[-1]) - int(cu[0])
    assert np.all(np.isnan(out[~owned])) and np.all(np.isnan(lse[:, ~owned]))   # (the unused tail keeps its NaN)
    assert np.all(np.isfinite(out[owned])) and not np.any(np.isnan(lse[:, owned])), (W, S)
    assert np.array_equal(np.isneginf(lse[:, owned]), np.isneginf(rl[:, owned]))
    fin = np.isfinite(rl)
    assert maxabs(out[owned], ro[owned]) < TOL[dtype], (W, S, maxabs(out[owned], ro[owned]))
    assert maxabs(lse[fin], rl[fin]) < TOL[dtype], (W, S, maxabs(lse[fin], rl[fin]))


@pytest.mark.parametrize("d", [32, 64, 128, 80])
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_ragged_sink_matches_fp64_reference_at_the_edges(dtype, layout, d):
    """The COUNTS and LENS of tests/test_gpu_ragged.py (no tokens, one token into an empty cache, fewer keys than tokens, a full and
    an out-of-range length) with seven unused tail rows, at every (S, W) pair of the grid."""
    torch = _torch()
    rng = np.random.default_rng(d + (11 if dtype == "bf16" else 0))
    dp = {80: 128}.get(d, d)
    for pi, S, W in grid_pairs(d, 0) + grid_pairs(d, 1):
        H, Hkv = grid_heads(pi, d)
        q, k, v, cu = _ragged_case(rng, dtype, H, Hkv, COUNTS, LENS, NCAP, d, W, S, tail=7)
        T = q.shape[0]
        assert T == RAGGED_T
        ns = _splits("ragged", len(COUNTS), H, Hkv, T, NCAP, dp, W, S)
        assert all(p[1] == ns for p in GPU_SPLITS if p[0] == ("ragged", len(COUNTS), H, Hkv, T, NCAP, dp, W, S))
        tk, tv = _caches(k, v, layout, dp, dtype)
        out, lse = _nan_out(T, H, d)
        _ops("ragged")(_packed(q, dtype), tk, tv, _i32(cu), _i32(LENS), causal=True, layout=layout, out=out, lse=lse, window=W, sink=S)
        torch.cuda.synchronize()
        _check_ragged(q, k, v, cu, LENS, W, S, dtype, out, lse)


# ---- no sinks: the windowed call's bits; a window or sinks over the whole cache: the unwindowed call's bits ----

@pytest.mark.parametrize("paged", [False, True], ids=["slab", "paged"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_no_sinks_return_the_windowed_bits_and_sinks_over_the_whole_cache_the_unwindowed_bits(dtype, paged):
    torch = _torch()
    rng = np.random.default_rng(5 + paged)
    H, Hkv, d, Ncap, ps, W = 4, 2, 64, 640 if paged else NCAP, 128, 160
    lens = [0, 1, 129, 300, NCAP, 9999]
    for family, Nq in (("decode", 1), ("decode", 33), ("extend", 200), ("ragged", None)):
        if family == "ragged":
            counts = [0, 1, 33, 129, 200, 5]
            q, k, v, cu = _ragged_case(rng, dtype, H, Hkv, counts, lens, Ncap, d, 0, 0)
            tq, head = _packed(q, dtype), (_i32(cu), _i32(lens))
        else:
            q, k, v = _uniform_case(rng, dtype, H, Hkv, Nq, d, lens, 0, 0, Ncap)
            tq, head = _to_dev(q, "bnhd", d, dtype), (_i32(lens),)
        tk, tv = (_to_dev(t, "bnhd", d, dtype) for t in (k, v))
        kw = {}
        if paged:
            table, num_pages = _table(rng, len(lens), Ncap, ps, lens)
            (tk, _), (tv, _) = (_pool(t, "bnhd", ps, table, num_pages, lens) for t in (tk, tv))
            kw = dict(block_table=_dev_table(table))
        same = lambda a, b: torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))
        windowed = _ops(family)(tq, tk, tv, *head, causal=True, window=W, **kw)
        assert same(_ops(family)(tq, tk, tv, *head, causal=True, window=W, sink=0, **kw), windowed), (family, Nq)
        want = _ops(family)(tq, tk, tv, *head, causal=True, **kw)
        assert not same(windowed, want)
        for Wx, S in [(Wx, 4) for Wx in (0, Ncap, 2 ** 31 - 1)] + [(W, S) for S in (Ncap, Ncap + 1, 2 ** 31 - 1)] + [(1, Ncap), (0, 0)]:
            got = _ops(family)(tq, tk, tv, *head, causal=True, window=Wx, sink=S, **kw)
            torch.cuda.synchronize()
            assert same(got, want), (family, Nq, Wx, S)
        # (and sinks that do change the result: the entry point is not the windowed one in disguise)
        assert not same(_ops(family)(tq, tk, tv, *head, causal=True, window=W, sink=4, **kw), windowed), (family, Nq)


# ---- paged ----

def _between(table, lens, counts, W, S, ps, Ncap, num_pages):
    """(the table with every slot wholly below its sequence's lowest window edge, except the sink slots, made invalid; the pages
    those slots named)."""
    bad, pages = table.copy(), []
    for b, (n, nq) in enumerate(zip(lens, counts)):
        if nq == 0:
            continue
        for s in range(-(-S // ps), _edge(n, nq, W, Ncap) // ps):
            pages.append(int(table[b, s]))
            bad[b, s] = -1 if (b + s) % 2 else num_pages + 5
    return bad, pages


@pytest.mark.parametrize("ps,permuted", [(128, False), (128, True), (256, True)])
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_paged_sink_returns_the_slab_bits_and_never_reads_a_slot_between_the_sinks_and_the_window(dtype, layout, ps, permuted):
    """Five pages of 128 rows (three of 256): the paged call returns the slab sink call's bits on the gathered cache; then the table
    entries of the slots wholly below each sequence's window, except the sink slot, become -1 or num_pages + 5 and their pages NaN,
    and the bits stay: what PagedKVCache.release_behind_window relies on.  The sink slots keep valid ids.  (By hand from _edge, with
    W = 160, S = 4 and the counts of the window test: 3 + 3 + 1 + 2 = 9 slots at ps = 128 with the lengths [0, 130, 289, 300, 520,
    9999]; those lengths give only 3 at ps = 256, Ncap = 768, so that case runs [0, 130, 289, 700, 768, 9999]: 3 + 2 + 0 + 1 = 6.)"""
    torch = _torch()
    rng = np.random.default_rng(ps + permuted + len(layout))
    H, Hkv, d, W, S = 4, 2, 64, 160, 4
    Ncap = 640 if ps == 128 else 768
    lens = [0, 130, 289, 300, NCAP, 9999] if ps == 128 else [0, 130, 289, 700, 768, 9999]
    B, mp = len(lens), Ncap // ps
    released = 0
    for family, Nq in (("decode", 1), ("decode", 33), ("extend", 200), ("ragged", None)):
        if family == "ragged":
            counts = [0, 1, 33, 129, 200, 5]
            q, k, v, cu = _ragged_case(rng, dtype, H, Hkv, counts, lens, Ncap, d, W, S)
            tq, head = _packed(q, dtype), (_i32(cu), _i32(lens))
        else:
            counts = [Nq] * B
            q, k, v = _uniform_case(rng, dtype, H, Hkv, Nq, d, lens, W, S, Ncap)
            tq, head = _to_dev(q, layout, d, dtype), (_i32(lens),)
        tk, tv = (_to_dev(t, layout, d, dtype) for t in (k, v))
        table, num_pages = _table(rng, B, Ncap, ps, lens)
        if not permuted:
            table = np.arange(B * mp, dtype=np.int32).reshape(B, mp)
        (kp, _), (vp, _) = (_pool(t, layout, ps, table, num_pages, None if not permuted else lens) for t in (tk, tv))
        want = _ops(family)(tq, tk, tv, *head, causal=True, layout=layout, window=W, sink=S)
        got = _ops(family)(tq, kp, vp, *head, causal=True, layout=layout, window=W, sink=S, block_table=_dev_table(table))
        assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(_bits(got[1]), _bits(want[1])), (family, Nq)
        bad, pages = _between(table, lens, counts, W, S, ps, Ncap, num_pages)
        released += len(pages)
        for b, nq in enumerate(counts):   # the sink slots still hold valid ids
            if nq > 0 and min(lens[b], Ncap) > 0:
                assert 0 <= bad[b, 0] < num_pages and bad[b, 0] == table[b, 0]
        for p in pages:
            kp[p] = float("nan")
            vp[p] = float("nan")
        got = _ops(family)(tq, kp, vp, *head, causal=True, layout=layout, window=W, sink=S, block_table=_dev_table(bad))
        torch.cuda.synchronize()
        assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(_bits(got[1]), _bits(want[1])), (family, Nq, "released")
        if layout == "bnhd":   # an independent opinion
            if family == "ragged":
                _check_ragged(q, k, v, cu, lens, W, S, dtype, got[0], got[1])
            else:
                _check_uniform(q, k, v, lens, W, S, dtype, _from_dev(got[0], layout), to_np(got[1]))
    assert released >= 6 and released == (9 if ps == 128 else 6)   # (slots did fall between the sinks and the windows)


# ---- ragged against extend ----

@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_ragged_sink_is_the_extend_sink_call_on_each_sequence_alone(dtype, layout):
    """Ncap = 256 with W = 100, S = 4 is one split under both policies (pinned; no jump exists there: the ranges are adjacent): the
    same bits per sequence.  Ncap = 520 with W = 200, S = 129 is three splits of the ragged call: the same values at the tolerance."""
    torch = _torch()
    rng = np.random.default_rng(43)
    H, Hkv, d = 4, 2, 64
    for Ncap, W, S, counts, lens, one in ((256, 100, 4, [0, 1, 33, 129, 200, 5], [100, 1, 256, 129, 230, 9999], True),
                                          (NCAP, 200, 129, [0, 1, 33, 129, 200, 5], [100, 1, 400, 129, NCAP, 9999], False)):
        T = sum(counts)
        ns = _splits("ragged", len(counts), H, Hkv, T, Ncap, d, W, S)
        assert (ns == 1) == one
        if one:
            assert (("ragged", 6, H, Hkv, T, Ncap, d, W, S), 1) in GPU_SPLITS
        q, k, v, cu = _ragged_case(rng, dtype, H, Hkv, counts, lens, Ncap, d, W, S)
        tq, (tk, tv), tl = _packed(q, dtype), _caches(k, v, layout, d, dtype), _i32(lens)
        out, lse = _nan_out(T, H, d)
        _ops("ragged")(tq, tk, tv, _i32(cu), tl, causal=True, layout=layout, out=out, lse=lse, window=W, sink=S)
        for b, nq in enumerate(counts):
            if nq == 0:
                continue
            s = int(cu[b])
            qb = tq[s:s + nq][None]
            if layout == "bhnd":
                qb = qb.transpose(1, 2).contiguous()
            o, l = _ops("extend")(qb, tk[b:b + 1], tv[b:b + 1], tl[b:b + 1], causal=True, layout=layout, window=W, sink=S)
            o = (o[0] if layout == "bnhd" else o[0].transpose(0, 1)).contiguous()
            if one:
                assert _splits("extend", 1, H, Hkv, nq, Ncap, d, W, S) == 1
                assert torch.equal(_bits(out[s:s + nq]), _bits(o)) and torch.equal(_bits(lse[:, s:s + nq]), _bits(l[0])), b
            else:
                a, bb = to_np(lse[:, s:s + nq]), to_np(l[0])
                assert np.array_equal(np.isneginf(a), np.isneginf(bb))
                fin = np.isfinite(bb)
                assert maxabs(to_np(out[s:s + nq]), to_np(o)) < TOL[dtype] and maxabs(a[fin], bb[fin]) < TOL[dtype], b
        _check_ragged(q, k, v, cu, lens, W, S, dtype, out, lse)


# ---- fused append ----

@pytest.mark.parametrize("paged", [False, True], ids=["slab", "paged"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_fused_sink_call_is_the_append_then_the_sink_call(dtype, paged):
    """The rows the append writes hold NaN before it (and so do the rows between the sinks and every window): the fused call returns
    the bits of append-then-attend, out and lse, and leaves the caches the plain append leaves, bit for bit."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    rng = np.random.default_rng(19 + paged)
    H, Hkv, d, W, S, ps = 4, 2, 64, 160, 4, 128
    Ncap = 640 if paged else NCAP
    lens = [0, 2, 161, 300, NCAP, 9999]
    B = len(lens)
    appends = {"decode": device_ops.decode_append, "extend": device_ops.extend_append, "ragged": device_ops.ragged_append}
    for family, Nq in (("decode", 3), ("extend", 200), ("ragged", None)):
        counts = [0, 1, 33, 129, 200, 5] if family == "ragged" else [Nq] * B
        if family == "ragged":
            q, k, v, cu = _ragged_case(rng, dtype, H, Hkv, counts, lens, Ncap, d, W, S)
            tq, head = _packed(q, dtype), (_i32(cu), _i32(lens))
            kn, vn = (_packed(_new_tokens(rng, dtype, (sum(counts), Hkv, d)), dtype) for _ in range(2))
        else:
            q, k, v = _uniform_case(rng, dtype, H, Hkv, Nq, d, lens, W, S, Ncap)
            tq, head = _to_dev(q, "bnhd", d, dtype), (_i32(lens),)
            kn, vn = (_dev(_new_tokens(rng, dtype, (B, Nq, Hkv, d)), "bnhd", dtype) for _ in range(2))
        for b, (n, nq) in enumerate(zip(lens, counts)):   # the new tokens' rows are not there yet
            n = min(max(n, 0), Ncap)
            k[b, :, max(n - nq, 0):n] = np.nan
            v[b, :, max(n - nq, 0):n] = np.nan
        tk, tv = (_to_dev(t, "bnhd", d, dtype) for t in (k, v))
        kw = {}
        if paged:
            table, num_pages = _table(rng, B, Ncap, ps, lens)
            (tk, _), (tv, _) = (_pool(t, "bnhd", ps, table, num_pages, lens) for t in (tk, tv))
            kw = dict(block_table=_dev_table(table))
        k1, v1, k2, v2 = tk.clone(), tv.clone(), tk.clone(), tv.clone()
        appends[family](kn, vn, k1, v1, *head, **kw)
        o1, l1 = _ops(family)(tq, k1, v1, *head, causal=True, window=W, sink=S, **kw)
        o2, l2 = _ops(family)(tq, k2, v2, *head, causal=True, window=W, sink=S, k_new=kn, v_new=vn, **kw)
        torch.cuda.synchronize()
        for a, b in ((o1, o2), (l1, l2), (k1, k2), (v1, v2)):
            assert torch.equal(_bits(a), _bits(b)), family
        assert not torch.equal(_bits(k2), _bits(tk)) and not bool(torch.isnan(o2).any())


# ---- the model ----

def _dense_sink_stack(x, layers, n_head, W, S):
    """The stack with its attention recomputed densely in torch fp32 under the sink + window mask: projections and the residual as
    modules_transformer makes them, the scores of all N x N pairs."""
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    B, N, E = x.shape
    i = torch.arange(N, device=x.device)
    ok = (i[None, :] <= i[:, None]) & ((i[None, :] > i[:, None] - W) | (i[None, :] < S))
    for wq, wk, wv, wo in layers:
        q, k, v = mt._project(x, wq, wk, wv, n_head)
        G = n_head // k.shape[2]
        qf, kf, vf = (t.float().permute(0, 2, 1, 3) for t in (q, k.repeat_interleave(G, 2), v.repeat_interleave(G, 2)))
        s = (qf @ kf.transpose(2, 3)) * q.shape[3] ** -0.5
        p = torch.softmax(s.masked_fill(~ok, float("-inf")), dim=-1)
        o = (p @ vf).permute(0, 2, 1, 3)
        x = x + (o.reshape(B * N, E).to(x.dtype) @ wo).view(B, N, E)
    return x


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_paged_model_with_sinks_releases_its_pages_keeps_the_sink_page_and_matches_dense_attention(dtype):
    """440 tokens through a 2-layer stack on a PagedKVCache(window=160, sink=4) of 128-row pages: a prompt of 100 (the extend path),
    140 and 150 more at once, then 50 fused steps, release_behind_window every 16 tokens.  The outputs are those of the dense stack
    under the sink + window mask; the pool gets slot 1's pages back at 416 tokens and keeps slot 0's."""
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    E, H, Hkv, L, B, W, S, ps, N = 128, 4, 2, 2, 2, 160, 4, 128, 440
    x, layers = _stack(np.random.default_rng(E + W + S), dtype, B, E, H, Hkv, L, N)
    want = to_np(_dense_sink_stack(x, layers, H, W, S))
    assert maxabs(want, to_np(_dense_sink_stack(x, layers, H, W, 0))) > 1e-2   # (the sinks matter to this stack)
    tol = _model_tol(dtype, want)
    cache = mt.PagedKVCache(L, B, 512, H, E // H, _tdt(dtype), "cuda", n_kv_head=Hkv, page_size=ps, window=W, sink=S)
    assert cache.n_pages == 8 and cache.sink_pages == 1
    got = [mt.attention_stack_prefill(x[:, :100].contiguous(), layers, H, cache),
           mt.attention_stack_extend(x[:, 100:240].contiguous(), layers, H, cache),
           mt.attention_stack_extend(x[:, 240:390].contiguous(), layers, H, cache)]
    assert len(cache.free) == 0 and cache.release_behind_window([390] * B) == 0
    first = [own[0] for own in cache.pages]
    second = [own[1] for own in cache.pages]
    free = []
    for n in range(390, N):
        got.append(mt.attention_stack_step_fused(x[:, n:n + 1].contiguous(), layers, H, cache))
        if (n + 1) % 16 == 0:
            cache.release_behind_window([n + 1] * B)
            free.append((n + 1, len(cache.free)))
    # slot 1 (rows 128 .. 255) is behind the window from 415 tokens on: the release at 416; slot 0 holds the sinks and stays
    assert free == [(400, 0), (416, 2), (432, 2)] and cache.released == [1, 1] and [len(p) for p in cache.pages] == [3, 3]
    assert sorted(cache.free) == sorted(second) and [own[0] for own in cache.pages] == first
    assert cache.block_table[:, 0].tolist() == first
    assert cache.lengths.tolist() == [N] * B
    got = to_np(torch.cat(got, dim=1))
    assert maxabs(got, want) < tol, (maxabs(got, want), tol)
    # the released pages may hold anything: NaN in them changes no later step
    clean = [(cache.k[li].clone(), cache.v[li].clone()) for li in range(L)]
    lengths = cache.lengths.clone()
    a = mt.attention_stack_step_fused(x[:, :1].contiguous(), layers, H, cache).clone()
    cache.lengths.copy_(lengths)
    cache.length_bound = N
    for li in range(L):
        cache.k[li].copy_(clean[li][0])
        cache.v[li].copy_(clean[li][1])
        cache.k[li][cache.free] = float("nan")
        cache.v[li][cache.free] = float("nan")
    b = mt.attention_stack_step_fused(x[:, :1].contiguous(), layers, H, cache)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(b).any()) and torch.equal(_bits(a), _bits(b))


def test_graphed_step_on_a_cache_with_sinks_replays_the_eager_fused_step_bit_for_bit():
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    dtype, E, H, Hkv, L, B, W, S, P, T = "bf16", 128, 4, 2, 2, 2, 160, 4, 300, 8
    x, layers = _stack(np.random.default_rng(31), dtype, B, E, H, Hkv, L, P + T)
    assert (("decode", B, H, Hkv, 1, 1024, E // H, W, S), 2) in GPU_SPLITS   # (the steps run as two splits: the combine is in the graph)
    caches = [mt.PagedKVCache(L, B, 1024, H, E // H, _tdt(dtype), "cuda", n_kv_head=Hkv, page_size=128, window=W, sink=S) for _ in range(2)]
    for c in caches:
        mt.attention_stack_prefill(x[:, :P].contiguous(), layers, H, c)
    graphed = mt.GraphedStep(layers, H, caches[0], T=1)
    for n in range(P, P + T):
        a = graphed.step(x[:, n:n + 1].contiguous()).clone()
        b = mt.attention_stack_step_fused(x[:, n:n + 1].contiguous(), layers, H, caches[1])
        torch.cuda.synchronize()
        assert torch.equal(_bits(a), _bits(b)), n
    assert caches[0].lengths.tolist() == caches[1].lengths.tolist() == [P + T] * B
    for li in range(L):
        assert torch.equal(_bits(caches[0].k[li]), _bits(caches[1].k[li])) and torch.equal(_bits(caches[0].v[li]), _bits(caches[1].v[li]))


# ---- the Python checks ----

def test_sink_python_checks_raise_before_any_launch():
    torch = _torch()
    q = torch.zeros(2, 1, 4, 64, device="cuda")
    qr, cu = torch.zeros(40, 4, 64, device="cuda"), _i32([0, 10, 40])
    kc = torch.zeros(2, 4096, 2, 64, device="cuda")
    for family, args in (("decode", (q, kc, kc)), ("extend", (q, kc, kc)), ("ragged", (qr, kc, kc, cu))):
        out = torch.full(args[0].shape, float("nan"), dtype=torch.float32, device="cuda")
        with pytest.raises(ValueError, match="needs window"):
            _ops(family)(*args, sink=4, out=out)
        with pytest.raises(ValueError, match="negative"):
            _ops(family)(*args, window=64, sink=-1, out=out)
        with pytest.raises(ValueError, match="causal"):
            _ops(family)(*args, causal=False, window=64, sink=4, out=out)
        with pytest.raises(ValueError, match="workspace too small"):   # (64 + 3000 keys are several splits; ragged always needs its map)
            _ops(family)(*args, window=64, sink=3000, out=out, workspace=torch.zeros(4, device="cuda"))
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all())   # (nothing ran)
    assert _splits("decode", 2, 4, 2, 1, 4096, 64, 64, 3000) > 1 and _splits("extend", 2, 4, 2, 1, 4096, 64, 64, 3000) > 1
