"""Sliding-window attention on the GPU (fa_mi355x_fwd_decode_window / _extend_window / _ragged_window,
include/flash_attn_mi355x_decode_window.h) against the fp64 references of tests/test_window_cpu.py on the same (bf16-rounded) inputs, at
the project's tolerances (TOL of tests/test_gpu_decode.py: fp32 1e-4, bf16 1e-3 max-abs on out and lse, the -inf pattern of lse exact).
The NaN discipline of tests/test_gpu_ragged.py: the caches are the front of larger NaN-filled buffers, every row at or past a length
holds NaN, out and lse are pre-filled with NaN -- and every cache row BELOW a sequence's lowest window edge holds NaN too, so one
read below the window shows.  Then: the bits of the unwindowed call where the window is 0 or covers the cache; the bits of the slab
call through a block table, with the slots below the window invalid and their pages NaN; ragged against extend per sequence; the
fused forms; a windowed paged model that gives its pages back; graph capture; and the Python checks."""
import math

import numpy as np
import pytest

import oracle
from gpu_util import maxabs, rand_u, to_np
from test_gpu_decode import TOL, _from_dev, _inputs, _tdt, _to_dev, _torch
from test_gpu_decode_append import _bits, _dev, _stack
from test_gpu_extend import _grouped_inputs, _model_tol, _nan_buffer
from test_gpu_paged import _dev_table, _pool, _table
from test_gpu_ragged import COUNTS, LENS, _cu, _i32, _nan_out, _packed, _rnd
from test_window_cpu import GPU_SPLITS, NCAP, RAGGED_T, WINDOWS, grid_heads, ragged_window_reference, window_reference

pytestmark = pytest.mark.gpu


def _lens(W):
    """Per-batch lengths of one call: empty, one key, around the window (W - 1: the window not yet full; W; W + 1: the first key
    falls out), a length whose last tile is partial, full, and out of range (clamped to Ncap)."""
    return [0, 1, W - 1, W, W + 1, 300, NCAP, 9999]


def _ops(family):
    from flash_attention_minitorch_amd import device_ops
    return {"decode": device_ops.flash_attn_decode, "extend": device_ops.flash_attn_extend, "ragged": device_ops.flash_attn_ragged}[family]


def _splits(family, B, H, Hkv, Nq, Ncap, d, W):
    from flash_attention_minitorch_amd import _lib
    return getattr(_lib.decode(), f"fa_mi355x_{family}_window_splits")(B, H, Hkv, Nq, Ncap, d, 1, W)


def _edge(n, nq, W, Ncap):
    """The lowest key any query of a sequence of (clamped) length n with nq new tokens admits."""
    return max(min(max(n, 0), Ncap) - nq - W + 1, 0) if W > 0 else 0


def _nan_below(k, v, lens, counts, W):
    """NaN in every cache row below each sequence's lowest window edge (k, v (B, Hkv, Ncap, d), in place)."""
    for b, (n, nq) in enumerate(zip(lens, counts)):
        if nq > 0:
            e = _edge(n, nq, W, k.shape[2])
            k[b, :, :e] = np.nan
            v[b, :, :e] = np.nan


def _caches(k, v, layout, dp, dtype):
    return tuple(_to_dev(t, layout, dp, dtype, _nan_buffer(t, dp, dtype)) for t in (k, v))


def _nan_like(tq, B, H, Nq):
    torch = _torch()
    return (torch.full(tq.shape, float("nan"), dtype=torch.float32, device="cuda"),
            torch.full((B, H, Nq), float("nan"), dtype=torch.float32, device="cuda"))


def _uniform(family, q, k, v, lens, W, layout, dtype, dp, **kw):
    """flash_attn_decode / flash_attn_extend with window=W on numpy q (B, H, Nq, d), k / v (B, Hkv, Ncap, d) into NaN-filled out and
    lse.  Returns numpy (out (B, H, Nq, d), lse (B, H, Nq))."""
    torch = _torch()
    B, H, Nq, d = q.shape
    tq = _to_dev(q, layout, d, dtype)
    tk, tv = _caches(k, v, layout, dp, dtype)
    out, lse = _nan_like(tq, B, H, Nq)
    got = _ops(family)(tq, tk, tv, _i32(lens), causal=True, layout=layout, out=out, lse=lse, window=W, **kw)
    torch.cuda.synchronize()
    assert got[0] is out and got[1] is lse
    return _from_dev(out, layout), to_np(lse)


def _picked(H, Hkv):
    """The heads held against the reference: all of an ungrouped call, the first, a middle and the last of a group."""
    return list(range(H)) if H == Hkv else sorted({0, H // 2, H - 1})


def _check_uniform(q, k, v, lens, W, dtype, out, lse, heads=None):
    """out (B, H, Nq, d), lse (B, H, Nq) against window_reference: every value finite (no NaN came in from below the window, from
    past a length or from an unwritten row), the -inf pattern of lse exact, the values within the tolerance."""
    B, H, Nq, d = q.shape
    G = H // k.shape[1]
    assert np.all(np.isfinite(out)) and not np.any(np.isnan(lse))
    for b in range(B):
        for h in (range(H) if heads is None else heads):
            ro, rl = window_reference(q[b, h][None], k[b, h // G][None], v[b, h // G][None], [lens[b]], W, 1.0 / math.sqrt(d))
            assert np.array_equal(np.isneginf(lse[b, h]), np.isneginf(rl[0])), (b, h, W)
            fin = np.isfinite(rl[0])
            assert maxabs(out[b, h], ro[0]) < TOL[dtype], (b, h, W, maxabs(out[b, h], ro[0]))
            if fin.any():
                assert maxabs(lse[b, h][fin], rl[0][fin]) < TOL[dtype], (b, h, W)


def _uniform_case(rng, dtype, H, Hkv, Nq, d, lens, W, Ncap=NCAP):
    q, k, v = _grouped_inputs(rng, dtype, len(lens), H, Hkv, Nq, Ncap, d, lens)
    _nan_below(k, v, lens, [Nq] * len(lens), W)
    return q, k, v


def _grid(family, dtype, layout, d, nqs):
    """Every window of the grid at every length of _lens, G cycling through 1, 4, 8 (grid_heads: the split count of every call is
    held against the policy in tests/test_window_cpu.py).  Returns the set of (several splits?) seen."""
    rng = np.random.default_rng(d + (7 if dtype == "bf16" else 0) + len(family))
    dp = {80: 128}.get(d, d)
    seen = set()
    for wi, W in enumerate(WINDOWS):
        H, Hkv = grid_heads(wi, d)
        for Nq in nqs:
            lens = _lens(W)
            ns = _splits(family, len(lens), H, Hkv, Nq, NCAP, dp, W)
            seen.add(ns > 1)
            assert all(p[1] == ns for p in GPU_SPLITS if p[0] == (family, len(lens), H, Hkv, Nq, NCAP, dp, W))
            q, k, v = _uniform_case(rng, dtype, H, Hkv, Nq, d, lens, W)
            out, lse = _uniform(family, q, k, v, lens, W, layout, dtype, dp)
            _check_uniform(q, k, v, lens, W, dtype, out, lse, heads=_picked(H, Hkv))
    return seen


@pytest.mark.parametrize("d", [32, 64, 128, 80])
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_decode_window_matches_fp64_reference_at_the_edges(dtype, layout, d):
    """A window inside one 32-key sub-tile, on its boundaries, across super tiles; a key range that starts at 0 and one that starts
    above it with a partial last tile; rows at negative positions; one split and several (the combine launch)."""
    assert _grid("decode", dtype, layout, d, (1, 3, 33, 128)) == {True, False}


@pytest.mark.parametrize("Nq", [129, 257, 400])
@pytest.mark.parametrize("d", [32, 64, 128, 80])
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_extend_window_matches_fp64_reference_at_the_edges(dtype, layout, d, Nq):
    """... and row blocks whose key ranges start at different tiles, waves of one block with different window edges."""
    assert _grid("extend", dtype, layout, d, (Nq,)) == {True, False}


def _ragged_case(rng, dtype, H, Hkv, counts, lens, Ncap, d, W, tail=0):
    q = _rnd(rng, dtype, (sum(counts) + tail, H, d))
    _, k, v = _inputs(rng, dtype, len(counts), Hkv, 1, Ncap, d, lens)
    _nan_below(k, v, lens, counts, W)
    return q, k, v, _cu(counts)


def _check_ragged(q, k, v, cu, lens, W, dtype, out, lse):
    out, lse = to_np(out), to_np(lse)
    ro, rl = ragged_window_reference(q, k, v, cu, lens, W, 1.0 / math.sqrt(q.shape[2]))
    owned = ~np.isnan(rl[0])
    assert owned.sum() == int(cu[-1]) - int(cu[0])
    assert np.all(np.isnan(out[~owned])) and np.all(np.isnan(lse[:, ~owned]))   # (the unused tail keeps its NaN)
    assert np.all(np.isfinite(out[owned])) and not np.any(np.isnan(lse[:, owned]))
    assert np.array_equal(np.isneginf(lse[:, owned]), np.isneginf(rl[:, owned]))
    fin = np.isfinite(rl)
    assert maxabs(out[owned], ro[owned]) < TOL[dtype], (W, maxabs(out[owned], ro[owned]))
    assert maxabs(lse[fin], rl[fin]) < TOL[dtype], (W, maxabs(lse[fin], rl[fin]))


@pytest.mark.parametrize("d", [32, 64, 128, 80])
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_ragged_window_matches_fp64_reference_at_the_edges(dtype, layout, d):
    """The COUNTS and LENS of tests/test_gpu_ragged.py (no tokens, one token into an empty cache, fewer keys than tokens, a full and
    an out-of-range length) with seven unused tail rows, at every window of the grid."""
    torch = _torch()
    rng = np.random.default_rng(d + (11 if dtype == "bf16" else 0))
    dp = {80: 128}.get(d, d)
    seen = set()
    for wi, W in enumerate(WINDOWS):
        H, Hkv = grid_heads(wi, d)
        q, k, v, cu = _ragged_case(rng, dtype, H, Hkv, COUNTS, LENS, NCAP, d, W, tail=7)
        T = q.shape[0]
        assert T == RAGGED_T
        ns = _splits("ragged", len(COUNTS), H, Hkv, T, NCAP, dp, W)
        seen.add(ns > 1)
        assert all(p[1] == ns for p in GPU_SPLITS if p[0] == ("ragged", len(COUNTS), H, Hkv, T, NCAP, dp, W))
        tk, tv = _caches(k, v, layout, dp, dtype)
        out, lse = _nan_out(T, H, d)
        _ops("ragged")(_packed(q, dtype), tk, tv, _i32(cu), _i32(LENS), causal=True, layout=layout, out=out, lse=lse, window=W)
        torch.cuda.synchronize()
        _check_ragged(q, k, v, cu, LENS, W, dtype, out, lse)
    assert seen == {True, False}


# ---- a window of 0, and one that covers the cache: the unwindowed call's bits ----

@pytest.mark.parametrize("paged", [False, True], ids=["slab", "paged"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_no_window_and_a_window_over_the_whole_cache_return_the_unwindowed_bits(dtype, paged):
    torch = _torch()
    rng = np.random.default_rng(5 + paged)
    H, Hkv, d, Ncap, ps = 4, 2, 64, 640 if paged else NCAP, 128
    lens = [0, 1, 129, 300, NCAP, 9999]
    for family, Nq in (("decode", 1), ("decode", 33), ("extend", 200), ("ragged", None)):
        if family == "ragged":
            counts = [0, 1, 33, 129, 200, 5]
            q, k, v, cu = _ragged_case(rng, dtype, H, Hkv, counts, lens, Ncap, d, 0)
            tq, head, n = _packed(q, dtype), (_i32(cu), _i32(lens)), q.shape[0]
        else:
            q, k, v = _uniform_case(rng, dtype, H, Hkv, Nq, d, lens, 0, Ncap)
            tq, head, n = _to_dev(q, "bnhd", d, dtype), (_i32(lens),), Nq
        tk, tv = (_to_dev(t, "bnhd", d, dtype) for t in (k, v))
        kw = {}
        if paged:
            table, num_pages = _table(rng, len(lens), Ncap, ps, lens)
            (tk, _), (tv, _) = (_pool(t, "bnhd", ps, table, num_pages, lens) for t in (tk, tv))
            kw = dict(block_table=_dev_table(table))
        want = _ops(family)(tq, tk, tv, *head, causal=True, **kw)
        for W in (0, Ncap + n, Ncap + n + 1, Ncap, 2 ** 31 - 1):
            got = _ops(family)(tq, tk, tv, *head, causal=True, window=W, **kw)
            torch.cuda.synchronize()
            assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(_bits(got[1]), _bits(want[1])), (family, Nq, W)


# ---- paged ----

def _below_window(table, lens, counts, W, ps, Ncap, num_pages):
    """(the table with every slot wholly below its sequence's lowest window edge made invalid, the pages those slots named)."""
    bad, pages = table.copy(), []
    for b, (n, nq) in enumerate(zip(lens, counts)):
        if nq == 0:
            continue
        for s in range(_edge(n, nq, W, Ncap) // ps):
            pages.append(int(table[b, s]))
            bad[b, s] = -1 if (b + s) % 2 else num_pages + 5
    return bad, pages


@pytest.mark.parametrize("ps,permuted", [(128, False), (128, True), (256, True)])
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_paged_window_returns_the_slab_bits_and_never_reads_a_slot_below_the_window(dtype, layout, ps, permuted):
    """Five pages of 128 rows (three of 256): the paged call returns the slab windowed call's bits on the gathered cache; then the
    table entries of the slots wholly below each sequence's window become -1 or num_pages + 5 and their pages NaN, and the bits stay:
    what PagedKVCache.release_behind_window relies on."""
    torch = _torch()
    rng = np.random.default_rng(ps + permuted + len(layout))
    H, Hkv, d, W = 4, 2, 64, 160
    Ncap = 640 if ps == 128 else 768
    lens = [0, 130, 289, 300, NCAP, 9999]
    B, mp = len(lens), Ncap // ps
    released = 0
    for family, Nq in (("decode", 1), ("decode", 33), ("extend", 200), ("ragged", None)):
        if family == "ragged":
            counts = [0, 1, 33, 129, 200, 5]
            q, k, v, cu = _ragged_case(rng, dtype, H, Hkv, counts, lens, Ncap, d, W)
            tq, head = _packed(q, dtype), (_i32(cu), _i32(lens))
        else:
            counts = [Nq] * B
            q, k, v = _uniform_case(rng, dtype, H, Hkv, Nq, d, lens, W, Ncap)
            tq, head = _to_dev(q, layout, d, dtype), (_i32(lens),)
        tk, tv = (_to_dev(t, layout, d, dtype) for t in (k, v))
        table, num_pages = _table(rng, B, Ncap, ps, lens)
        if not permuted:
            table = np.arange(B * mp, dtype=np.int32).reshape(B, mp)
        (kp, _), (vp, _) = (_pool(t, layout, ps, table, num_pages, None if not permuted else lens) for t in (tk, tv))
        want = _ops(family)(tq, tk, tv, *head, causal=True, layout=layout, window=W)
        got = _ops(family)(tq, kp, vp, *head, causal=True, layout=layout, window=W, block_table=_dev_table(table))
        assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(_bits(got[1]), _bits(want[1])), (family, Nq)
        bad, pages = _below_window(table, lens, counts, W, ps, Ncap, num_pages)
        released += len(pages)
        for p in pages:
            kp[p] = float("nan")
            vp[p] = float("nan")
        got = _ops(family)(tq, kp, vp, *head, causal=True, layout=layout, window=W, block_table=_dev_table(bad))
        torch.cuda.synchronize()
        assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(_bits(got[1]), _bits(want[1])), (family, Nq, "released")
        if layout == "bnhd":   # an independent opinion
            if family == "ragged":
                _check_ragged(q, k, v, cu, lens, W, dtype, got[0], got[1])
            else:
                _check_uniform(q, k, v, lens, W, dtype, _from_dev(got[0], layout), to_np(got[1]))
    assert released > 8   # (pages did fall below the windows)


# ---- ragged against extend ----

@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_ragged_window_is_the_extend_window_call_on_each_sequence_alone(dtype, layout):
    """Ncap = 256 with W = 100 is one split under both policies (pinned): the same bits per sequence.  Ncap = 520 with W = 300 is
    three splits of the ragged call: the same values at the tolerance."""
    torch = _torch()
    rng = np.random.default_rng(43)
    H, Hkv, d = 4, 2, 64
    for Ncap, W, counts, lens, one in ((256, 100, [0, 1, 33, 129, 200, 5], [100, 1, 256, 129, 230, 9999], True),
                                       (NCAP, 300, [0, 1, 33, 129, 200, 5], [100, 1, 400, 129, NCAP, 9999], False)):
        T = sum(counts)
        ns = _splits("ragged", len(counts), H, Hkv, T, Ncap, d, W)
        assert (ns == 1) == one
        if one:
            assert (("ragged", 6, H, Hkv, T, Ncap, d, W), 1) in GPU_SPLITS
        q, k, v, cu = _ragged_case(rng, dtype, H, Hkv, counts, lens, Ncap, d, W)
        tq, (tk, tv), tl = _packed(q, dtype), _caches(k, v, layout, d, dtype), _i32(lens)
        out, lse = _nan_out(T, H, d)
        _ops("ragged")(tq, tk, tv, _i32(cu), tl, causal=True, layout=layout, out=out, lse=lse, window=W)
        for b, nq in enumerate(counts):
            if nq == 0:
                continue
            s = int(cu[b])
            qb = tq[s:s + nq][None]
            if layout == "bhnd":
                qb = qb.transpose(1, 2).contiguous()
            o, l = _ops("extend")(qb, tk[b:b + 1], tv[b:b + 1], tl[b:b + 1], causal=True, layout=layout, window=W)
            o = (o[0] if layout == "bnhd" else o[0].transpose(0, 1)).contiguous()
            if one:
                assert _splits("extend", 1, H, Hkv, nq, Ncap, d, W) == 1
                assert torch.equal(_bits(out[s:s + nq]), _bits(o)) and torch.equal(_bits(lse[:, s:s + nq]), _bits(l[0])), b
            else:
                a, bb = to_np(lse[:, s:s + nq]), to_np(l[0])
                assert np.array_equal(np.isneginf(a), np.isneginf(bb))
                fin = np.isfinite(bb)
                assert maxabs(to_np(out[s:s + nq]), to_np(o)) < TOL[dtype] and maxabs(a[fin], bb[fin]) < TOL[dtype], b
        _check_ragged(q, k, v, cu, lens, W, dtype, out, lse)


# ---- fused append ----

def _new_tokens(rng, dtype, shape):
    x = rand_u(rng, shape)
    return oracle.bf16_round(x) if dtype == "bf16" else x


@pytest.mark.parametrize("paged", [False, True], ids=["slab", "paged"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_fused_window_call_is_the_append_then_the_window_call(dtype, paged):
    """The rows the append writes hold NaN before it (and so do the rows below every window): the fused call returns the bits of
    append-then-attend, out and lse, and leaves the caches the plain append leaves, bit for bit."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    rng = np.random.default_rng(19 + paged)
    H, Hkv, d, W, ps = 4, 2, 64, 160, 128
    Ncap = 640 if paged else NCAP
    lens = [0, 2, 161, 300, NCAP, 9999]
    B = len(lens)
    appends = {"decode": device_ops.decode_append, "extend": device_ops.extend_append, "ragged": device_ops.ragged_append}
    for family, Nq in (("decode", 3), ("extend", 200), ("ragged", None)):
        counts = [0, 1, 33, 129, 200, 5] if family == "ragged" else [Nq] * B
        if family == "ragged":
            q, k, v, cu = _ragged_case(rng, dtype, H, Hkv, counts, lens, Ncap, d, W)
            tq, head = _packed(q, dtype), (_i32(cu), _i32(lens))
            kn, vn = (_packed(_new_tokens(rng, dtype, (sum(counts), Hkv, d)), dtype) for _ in range(2))
        else:
            q, k, v = _uniform_case(rng, dtype, H, Hkv, Nq, d, lens, W, Ncap)
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
        o1, l1 = _ops(family)(tq, k1, v1, *head, causal=True, window=W, **kw)
        o2, l2 = _ops(family)(tq, k2, v2, *head, causal=True, window=W, k_new=kn, v_new=vn, **kw)
        torch.cuda.synchronize()
        for a, b in ((o1, o2), (l1, l2), (k1, k2), (v1, v2)):
            assert torch.equal(_bits(a), _bits(b)), family
        assert not torch.equal(_bits(k2), _bits(tk)) and not bool(torch.isnan(o2).any())


# ---- the model ----

def _dense_window_stack(x, layers, n_head, W):
    """The stack with its attention recomputed densely in torch fp32 under the window's mask: projections and the residual as
    modules_transformer makes them, the scores of all N x N pairs."""
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    B, N, E = x.shape
    i = torch.arange(N, device=x.device)
    ok = (i[None, :] <= i[:, None]) & (i[None, :] > i[:, None] - W)
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
def test_windowed_paged_model_releases_its_pages_and_matches_dense_window_attention(dtype):
    """300 tokens through a 2-layer stack on a PagedKVCache(window=160) of 128-row pages: a prompt of 100 (the extend path: the
    square forward has no window), 140 more at once, then 60 single steps, release_behind_window every 16 tokens.  The outputs are
    those of the dense windowed stack, and the pool gets its pages back."""
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    E, H, Hkv, L, B, W, ps, N = 128, 4, 2, 2, 2, 160, 128, 300
    x, layers = _stack(np.random.default_rng(E + W), dtype, B, E, H, Hkv, L, N)
    want = to_np(_dense_window_stack(x, layers, H, W))
    tol = _model_tol(dtype, want)
    cache = mt.PagedKVCache(L, B, 384, H, E // H, _tdt(dtype), "cuda", n_kv_head=Hkv, page_size=ps, window=W)
    assert cache.n_pages == 6
    got = [mt.attention_stack_prefill(x[:, :100].contiguous(), layers, H, cache),
           mt.attention_stack_extend(x[:, 100:240].contiguous(), layers, H, cache)]
    assert len(cache.free) == 2 and cache.release_behind_window([240] * B) == 0
    free = []
    for n in range(240, N):
        got.append(mt.attention_stack_step_fused(x[:, n:n + 1].contiguous(), layers, H, cache))
        if (n + 1) % 16 == 0:
            cache.release_behind_window([n + 1] * B)
            free.append((n + 1, len(cache.free)))
    # three slots each from 257 tokens on; slot 0 (rows 0 .. 127) is behind the window from 287 tokens on: the release at 288
    assert free == [(256, 2), (272, 0), (288, 2)] and cache.released == [1, 1] and [len(p) for p in cache.pages] == [2, 2]
    assert cache.lengths.tolist() == [N] * B
    got = to_np(torch.cat(got, dim=1))
    assert maxabs(got, want) < tol, (maxabs(got, want), tol)
    # the released pages may hold anything: NaN in them changes no later step
    for li in range(L):
        cache.k[li][cache.free] = float("nan")
        cache.v[li][cache.free] = float("nan")
    more = mt.attention_stack_step_fused(x[:, :1].contiguous(), layers, H, cache)
    assert not bool(torch.isnan(more).any())


def test_graphed_step_on_a_windowed_cache_replays_the_eager_fused_step_bit_for_bit():
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    dtype, E, H, Hkv, L, B, W, P, S = "bf16", 128, 4, 2, 2, 2, 160, 250, 8
    x, layers = _stack(np.random.default_rng(31), dtype, B, E, H, Hkv, L, P + S)
    assert (("decode", B, H, Hkv, 1, 1024, E // H, W), 2) in GPU_SPLITS   # (the steps run as two splits: the combine is in the graph)
    caches = [mt.PagedKVCache(L, B, 1024, H, E // H, _tdt(dtype), "cuda", n_kv_head=Hkv, page_size=128, window=W) for _ in range(2)]
    for c in caches:
        mt.attention_stack_prefill(x[:, :P].contiguous(), layers, H, c)
    graphed = mt.GraphedStep(layers, H, caches[0], T=1)
    for n in range(P, P + S):
        a = graphed.step(x[:, n:n + 1].contiguous()).clone()
        b = mt.attention_stack_step_fused(x[:, n:n + 1].contiguous(), layers, H, caches[1])
        torch.cuda.synchronize()
        assert torch.equal(_bits(a), _bits(b)), n
    assert caches[0].lengths.tolist() == caches[1].lengths.tolist() == [P + S] * B
    for li in range(L):
        assert torch.equal(_bits(caches[0].k[li]), _bits(caches[1].k[li])) and torch.equal(_bits(caches[0].v[li]), _bits(caches[1].v[li]))


# ---- the Python checks ----

def test_window_python_checks_raise_before_any_launch():
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    q = torch.zeros(2, 1, 4, 64, device="cuda")
    qr, cu = torch.zeros(40, 4, 64, device="cuda"), _i32([0, 10, 40])
    kc = torch.zeros(2, 4096, 2, 64, device="cuda")
    for family, args in (("decode", (q, kc, kc)), ("extend", (q, kc, kc)), ("ragged", (qr, kc, kc, cu))):
        out = torch.full(args[0].shape, float("nan"), dtype=torch.float32, device="cuda")
        with pytest.raises(ValueError, match="causal"):
            _ops(family)(*args, causal=False, window=64, out=out)
        with pytest.raises(ValueError, match="negative"):
            _ops(family)(*args, window=-1, out=out)
        with pytest.raises(ValueError, match="workspace too small"):   # (decode at W = 3000 is several splits; ragged always needs its map)
            _ops(family)(*args, window=3000, out=out, workspace=torch.zeros(4, device="cuda"))
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all())   # (nothing ran)
    assert _splits("decode", 2, 4, 2, 1, 4096, 64, 3000) > 1 and _splits("extend", 2, 4, 2, 1, 4096, 64, 3000) > 1
