"""The ragged-batch call on the GPU (fa_mi355x_fwd_ragged / _ragged_append / _fwd_ragged_append and their _paged forms,
include/flash_attn_mi355x_decode_ragged.h: every sequence brings its own number of new tokens, packed) against the fp64 reference of
tests/test_ragged_cpu.py on the same (bf16-rounded) inputs, at the project's tolerances (fp32 1e-4, bf16 1e-3 max-abs on out and lse,
the -inf pattern of lse exact).  The caches are the front of larger NaN-filled buffers with NaN in every invalid row; out and lse
are pre-filled with NaN, so a row the call should not write shows, and a row it should write but did not shows too."""
import math

import numpy as np
import pytest

import oracle
from gpu_util import maxabs, rand_u, to_np
from test_gpu_decode import TOL, _inputs, _tdt, _to_dev, _torch
from test_gpu_decode_append import _bits, _dev, _new_and_cache, _stack
from test_gpu_extend import _model_tol, _nan_buffer
from test_gpu_paged import _dev_table, _gather, _pool, _table
from test_ragged_cpu import GPU_SPLITS, ragged_append_reference, ragged_reference, seq_rows

pytestmark = pytest.mark.gpu

NCAP = 520
# one call at the edges: no tokens; one token into an empty cache (length 0: its row sits below position 0); one token after one key
# (count + 1); an empty prefix (length = count); fewer keys than tokens (rows at negative positions); a length whose last 128-key
# tile is partial and whose causal diagonal crosses tiles; a full cache; an out-of-range length (clamped to Ncap)
COUNTS = [0, 1, 1, 33, 129, 200, 257, 5]
LENS = [300, 0, 2, 33, 100, 300, NCAP, 9999]


def _splits(B, H, Hkv, T, Ncap, d, dtype):
    from flash_attention_minitorch_amd import _lib
    return _lib.decode().fa_mi355x_ragged_splits(B, H, Hkv, T, Ncap, d, 1 if dtype == "bf16" else 0)


def _cu(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def _rnd(rng, dtype, shape):
    x = rand_u(rng, shape)
    return oracle.bf16_round(x) if dtype == "bf16" else x


def _batch(rng, dtype, H, Hkv, counts, lens, Ncap, d, tail=0):
    """numpy q (T, H, d) packed (T = sum(counts) + tail), k and v (B, Hkv, Ncap, d) with NaN at and past lens[b], and cu."""
    q = _rnd(rng, dtype, (sum(counts) + tail, H, d))
    _, k, v = _inputs(rng, dtype, len(counts), Hkv, 1, Ncap, d, lens)
    return q, k, v, _cu(counts)


def _i32(x):
    torch = _torch()
    return None if x is None else torch.tensor(np.asarray(x), dtype=torch.int32, device="cuda")


def _packed(x, dtype, slack=0):
    """(T, heads, d) numpy -> a contiguous device tensor, the front of a NaN-filled allocation ``slack`` rows longer."""
    torch = _torch()
    buf = torch.full((x.shape[0] + slack,) + x.shape[1:], float("nan"), dtype=_tdt(dtype), device="cuda")
    buf[:x.shape[0]].copy_(torch.from_numpy(np.ascontiguousarray(x)))
    return buf[:x.shape[0]]


def _nan_out(T, H, d, slack=0):
    torch = _torch()
    out = torch.full((T + slack, H, d), float("nan"), dtype=torch.float32, device="cuda")
    lse = torch.full((H, T), float("nan"), dtype=torch.float32, device="cuda")
    return out[:T], lse


def _caches(k, v, layout, dp, dtype):
    return tuple(_to_dev(t, layout, dp, dtype, _nan_buffer(t, dp, dtype)) for t in (k, v))


def _ragged(q, k, v, cu, lens, causal, layout, dtype, dp, slack=0, **kw):
    """flash_attn_ragged on numpy q (T, H, d), k / v (B, Hkv, Ncap, d) into NaN-filled out and lse.  Returns the device (out, lse)."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    T, H, d = q.shape
    tk, tv = _caches(k, v, layout, dp, dtype)
    out, lse = _nan_out(T, H, d, slack)
    got = device_ops.flash_attn_ragged(_packed(q, dtype, slack), tk, tv, _i32(cu), _i32(lens), causal=causal, layout=layout, out=out, lse=lse,
                                       **kw)
    torch.cuda.synchronize()
    assert got[0] is out and got[1] is lse
    return out, lse


def _check(q, k, v, cu, lens, causal, dtype, out, lse, heads=None):
    """out (T, H, d), lse (H, T) (device) against ragged_reference: the rows no sequence owns still hold NaN (all of them, so the
    call wrote nothing there), every owned row is finite, the -inf pattern of lse is exact, the values within the tolerance."""
    out, lse = to_np(out), to_np(lse)
    ro, rl = ragged_reference(q, k, v, cu, lens, causal, 1.0 / math.sqrt(q.shape[2]))
    heads = list(range(q.shape[1])) if heads is None else list(heads)
    out, lse, ro, rl = out[:, heads], lse[heads], ro[:, heads], rl[heads]
    owned = ~np.isnan(rl[0])
    assert owned.sum() == sum(e - s for s, e in (seq_rows(cu, q.shape[0], b) for b in range(len(cu) - 1)))
    assert np.all(np.isnan(out[~owned])) and np.all(np.isnan(lse[:, ~owned]))
    assert np.all(np.isfinite(out[owned]))
    assert np.array_equal(np.isneginf(lse[:, owned]), np.isneginf(rl[:, owned]))
    fin = np.isfinite(rl)
    assert maxabs(out[owned], ro[owned]) < TOL[dtype], maxabs(out[owned], ro[owned])
    assert maxabs(lse[fin], rl[fin]) < TOL[dtype], maxabs(lse[fin], rl[fin])


@pytest.mark.parametrize("d", [32, 64, 128, 80])
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_ragged_matches_fp64_reference_at_the_edges(dtype, layout, d):
    rng = np.random.default_rng(d + (7 if dtype == "bf16" else 0))
    dp = {80: 128}.get(d, d)
    if d == 64:
        assert ((8, 2, 2, 626, NCAP, 64), _splits(8, 2, 2, 626, NCAP, 64, dtype)) in GPU_SPLITS   # (three chunks: the combine runs)
    for causal in (True, False):
        q, k, v, cu = _batch(rng, dtype, 2, 2, COUNTS, LENS, NCAP, d)
        out, lse = _ragged(q, k, v, cu, LENS, causal, layout, dtype, dp)
        _check(q, k, v, cu, LENS, causal, dtype, out, lse)


def _fused_case(rng, dtype, H, Hkv, counts, lens, Ncap, d, d_new, tail=0):
    """Packed q (T, H, d_new), k_new / v_new (T, Hkv, d_new) and sentinel caches (B, Ncap, Hkv, d) as test_gpu_decode_append makes
    them (NaN in columns d_new .. d-1 and in column 0 of every seventh row), but the valid OLDER rows of every sequence finite with
    zero columns past d_new, as a padded cache holds them."""
    B, T = len(counts), sum(counts) + tail
    q = _rnd(rng, dtype, (T, H, d_new))
    (kn, vn), (kc, vc) = _new_and_cache(rng, dtype, 1, T, Hkv, Ncap, d, d_new)
    kn, vn = kn[0], vn[0]
    kc, vc = (np.repeat(c, B, axis=0) * np.arange(1, B + 1, dtype=np.float32).reshape(B, 1, 1, 1) / B for c in (kc, vc))
    if dtype == "bf16":
        kc, vc = oracle.bf16_round(kc), oracle.bf16_round(vc)
    for b, (n, c) in enumerate(zip(lens, counts)):
        old = max(min(max(n, 0), Ncap) - c, 0)
        for t in (kc, vc):
            t[b, :old, :, d_new:] = 0
            t[b, :old:7, :, 0] = 0.25
    return q, kn, vn, kc, vc, _cu(counts)


def _after_append(kn, vn, kc, vc, cu, lens, d_new):
    """The caches the append leaves, as ragged_reference reads them: (B, Hkv, Ncap, d_new)."""
    return tuple(ragged_append_reference(n, c, cu, lens).transpose(0, 2, 1, 3)[..., :d_new] for n, c in ((kn, kc), (vn, vc)))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_unused_tail_and_every_cache_row_the_append_should_not_touch_keep_their_nan_bits(dtype):
    """T = sum(counts) + 50.  The fused call: out and lse of the tail keep their NaN bit patterns, the caches equal the placement rule
    bit for bit (NaN sentinels included: the rows of the sequence without tokens, the rows in front of and behind the new ones), and
    the values are the reference's although the rows the append wrote held NaN."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    rng = np.random.default_rng(17)
    H, Hkv, d, d_new, tail = 2, 2, 64, 64, 50
    q, kn, vn, kc, vc, cu = _fused_case(rng, dtype, H, Hkv, COUNTS, LENS, NCAP, d, d_new, tail)
    T = q.shape[0]
    assert T == 676 and ((8, 2, 2, T, NCAP, 64), _splits(8, 2, 2, T, NCAP, 64, dtype)) in GPU_SPLITS
    tkc, tvc = _dev(kc, "bnhd", dtype), _dev(vc, "bnhd", dtype)
    out, lse = _nan_out(T, H, d_new)
    nan_o, nan_l = _bits(out[T - tail:]).clone(), _bits(lse[:, T - tail:]).clone()
    device_ops.flash_attn_ragged(_packed(q, dtype), tkc, tvc, _i32(cu), _i32(LENS), causal=True, out=out, lse=lse,
                                 k_new=_packed(kn, dtype), v_new=_packed(vn, dtype))
    torch.cuda.synchronize()
    assert torch.equal(_bits(out[T - tail:]), nan_o) and torch.equal(_bits(lse[:, T - tail:]), nan_l)
    for got, new, cache in ((tkc, kn, kc), (tvc, vn, vc)):
        assert torch.equal(_bits(got), _bits(_dev(ragged_append_reference(new, cache, cu, LENS), "bnhd", dtype)))
    ke, ve = _after_append(kn, vn, kc, vc, cu, LENS, d_new)
    _check(q, ke, ve, cu, LENS, True, dtype, out, lse)


# (H, Hkv): G = 1, 3, 8 with G * nq_b = 43, 129, 7, 1 / 129, 387, 21, 3 / 344, 1032, 56, 8 rows: no multiple of 32 but the last
GROUPED = [(3, 3), (6, 2), (8, 1)]


@pytest.mark.parametrize("H,Hkv", GROUPED, ids=[f"H{h}-Hkv{k}" for h, k in GROUPED])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_grouped_heads_share_their_kv_head(dtype, H, Hkv):
    rng = np.random.default_rng(H * 100 + Hkv)
    counts, lens = [43, 0, 129, 7, 1], [300, 5, NCAP, 7, 200]
    for layout, causal in (("bnhd", True), ("bhnd", True), ("bnhd", False)):
        q, k, v, cu = _batch(rng, dtype, H, Hkv, counts, lens, NCAP, 64)
        out, lse = _ragged(q, k, v, cu, lens, causal, layout, dtype, 64)
        _check(q, k, v, cu, lens, causal, dtype, out, lse)


# (H, Hkv, counts, Ncap, d, splits, lens, every n-th head checked): the counts are pinned in tests/test_ragged_cpu.py
SPLIT_SHAPES = [
    (2, 2, [160, 1], 2048, 64, 8, [2048, 1000], 1),     # eight chunks of 256 keys; the second sequence's last four are past its length
    (2, 2, [160, 1], 2048, 128, 8, [2048, 1000], 1),
    (64, 64, [1, 3, 40, 0, 2, 1, 1, 70], 700, 32, 1, [700, 650, 300, 5, 2, 129, 128, 9999], 13),   # one chunk of six super tiles
]


@pytest.mark.parametrize("case", SPLIT_SHAPES, ids=[f"H{c[0]}-Ncap{c[3]}-d{c[4]}" for c in SPLIT_SHAPES])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_several_splits_and_one_split_of_several_super_tiles(dtype, case):
    H, Hkv, counts, Ncap, d, ns, lens, step = case
    assert _splits(len(counts), H, Hkv, sum(counts), Ncap, d, dtype) == ns
    assert ((len(counts), H, Hkv, sum(counts), Ncap, d), ns) in GPU_SPLITS
    rng = np.random.default_rng(Ncap + d)
    for causal in (True, False):
        q, k, v, cu = _batch(rng, dtype, H, Hkv, counts, lens, Ncap, d)
        out, lse = _ragged(q, k, v, cu, lens, causal, "bnhd", dtype, d)
        _check(q, k, v, cu, lens, causal, dtype, out, lse, heads=range(0, H, step))


@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_one_split_returns_the_bits_of_the_extend_call_on_each_sequence_alone(dtype, layout):
    """Ncap = 256 is one chunk under both policies (asserted), and the loop over a row's tiles is the same code: each sequence's rows
    equal flash_attn_extend on that sequence alone bit for bit."""
    torch = _torch()
    from flash_attention_minitorch_amd import _lib, device_ops
    rng = np.random.default_rng(41)
    H, Hkv, Ncap, d = 4, 2, 256, 64
    counts, lens = [0, 1, 33, 129, 200, 5], [100, 1, 256, 129, 230, 9999]
    T = sum(counts)
    assert _splits(len(counts), H, Hkv, T, Ncap, d, dtype) == 1 and ((6, H, Hkv, T, Ncap, d), 1) in GPU_SPLITS
    for causal in (True, False):
        q, k, v, cu = _batch(rng, dtype, H, Hkv, counts, lens, Ncap, d)
        tq, (tk, tv), tl = _packed(q, dtype), _caches(k, v, layout, d, dtype), _i32(lens)
        out, lse = _nan_out(T, H, d)
        device_ops.flash_attn_ragged(tq, tk, tv, _i32(cu), tl, causal=causal, layout=layout, out=out, lse=lse)
        for b, nq in enumerate(counts):
            if nq == 0:
                continue
            assert _lib.decode().fa_mi355x_extend_splits(1, H, Hkv, nq, Ncap, d, 1 if dtype == "bf16" else 0) == 1
            s = int(cu[b])
            qb = tq[s:s + nq][None]
            if layout == "bhnd":
                qb = qb.transpose(1, 2).contiguous()
            o, l = device_ops.flash_attn_extend(qb, tk[b:b + 1], tv[b:b + 1], tl[b:b + 1], causal=causal, layout=layout)
            o = o[0] if layout == "bnhd" else o[0].transpose(0, 1)
            assert torch.equal(_bits(out[s:s + nq]), _bits(o.contiguous())) and torch.equal(_bits(lse[:, s:s + nq]), _bits(l[0])), (b, causal)
        _check(q, k, v, cu, lens, causal, dtype, out, lse)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_equal_counts_agree_with_the_extend_call_and_ones_with_the_decode_call(dtype):
    """Second opinions at tolerance (several splits on both sides, chunked differently: not bitwise)."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    rng = np.random.default_rng(23)
    B, H, Hkv, Ncap, d = 3, 4, 2, 1300, 64
    lens = [1300, 777, 40]
    for nq, other in ((70, device_ops.flash_attn_extend), (1, device_ops.flash_attn_decode)):
        q, k, v, cu = _batch(rng, dtype, H, Hkv, [nq] * B, lens, Ncap, d)
        tq, (tk, tv), tl = _packed(q, dtype), _caches(k, v, "bnhd", d, dtype), _i32(lens)
        o1, l1 = device_ops.flash_attn_ragged(tq, tk, tv, _i32(cu), tl, causal=True)
        o2, l2 = other(tq.view(B, nq, H, d), tk, tv, tl, causal=True)
        torch.cuda.synchronize()
        l1, l2 = to_np(l1).reshape(H, B, nq).transpose(1, 0, 2), to_np(l2)
        assert np.array_equal(np.isneginf(l1), np.isneginf(l2))
        fin = np.isfinite(l2)
        assert maxabs(to_np(o1).reshape(B, nq, H, d), to_np(o2)) < TOL[dtype] and maxabs(l1[fin], l2[fin]) < TOL[dtype]


def _paged_case(rng, dtype, layout, H, Hkv, counts, lens, Ncap, d, ps, permuted):
    q, k, v, cu = _batch(rng, dtype, H, Hkv, counts, lens, Ncap, d)
    tk, tv = (_to_dev(t, layout, d, dtype) for t in (k, v))
    table, num_pages = _table(rng, len(counts), Ncap, ps, lens)
    if not permuted:   # the identity: sequence b's pages are b * max_pages .. in order (every slot its own page)
        table = np.arange(len(counts) * (Ncap // ps), dtype=np.int32).reshape(len(counts), Ncap // ps)
    (kp, _), (vp, _) = (_pool(t, layout, ps, table, num_pages, None if not permuted else lens) for t in (tk, tv))
    return (q, k, v, cu), (tk, tv), (kp, vp, table)


@pytest.mark.parametrize("ps,permuted", [(128, False), (128, True), (256, False), (256, True)])
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_paged_call_equals_the_contiguous_ragged_call_on_the_gathered_cache_bitwise(dtype, layout, ps, permuted):
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    rng = np.random.default_rng(ps + permuted + len(layout))
    H, Hkv, Ncap, d = 4, 2, 768, 64
    counts, lens = [0, 1, 33, 129, 200, 5], [300, 1, 128, 129, 700, 9999]
    (q, k, v, cu), (tk, tv), (kp, vp, table) = _paged_case(rng, dtype, layout, H, Hkv, counts, lens, Ncap, d, ps, permuted)
    tq, tcu, tl, tt = _packed(q, dtype), _i32(cu), _i32(lens), _dev_table(table)
    for causal in (True, False):
        want = device_ops.flash_attn_ragged(tq, tk, tv, tcu, tl, causal=causal, layout=layout)
        out, lse = _nan_out(q.shape[0], H, d)
        device_ops.flash_attn_ragged(tq, kp, vp, tcu, tl, causal=causal, layout=layout, block_table=tt, out=out, lse=lse)
        assert torch.equal(_bits(out), _bits(want[0])) and torch.equal(_bits(lse), _bits(want[1]))
        if causal and layout == "bnhd":   # an independent opinion, once per geometry
            _check(q, k, v, cu, lens, causal, dtype, out, lse)


def test_two_sequences_share_the_pages_of_a_prefix():
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    rng = np.random.default_rng(3)
    dtype, H, Hkv, Ncap, d, ps = "bf16", 4, 2, 512, 64, 128
    counts, lens = [40, 3, 0], [300, 259, 256]
    q, k, v, cu = _batch(rng, dtype, H, Hkv, counts, lens, Ncap, d)
    k[1, :, :256], v[1, :, :256] = k[0, :, :256], v[0, :, :256]   # sequences 0, 1 and 2 share a prefix of two pages
    k[2, :, :256], v[2, :, :256] = k[0, :, :256], v[0, :, :256]
    tk, tv = (_to_dev(t, "bnhd", d, dtype) for t in (k, v))
    table = np.array([[5, 2, 7, 9], [5, 2, 0, 9], [5, 2, 9, 9]], dtype=np.int32)   # page 9 holds NaN
    (kp, _), (vp, _) = (_pool(t, "bnhd", ps, np.array([[5, 2, 7, 9], [9, 9, 0, 9], [9, 9, 9, 9]], dtype=np.int32), 10, lens) for t in (tk, tv))
    for pool, cache in ((kp, tk), (vp, tv)):
        pool[0] = cache[1, 256:384]
        pool[9] = float("nan")
    tq, tcu, tl = _packed(q, dtype), _i32(cu), _i32(lens)
    want = device_ops.flash_attn_ragged(tq, tk, tv, tcu, tl, causal=True)
    got = device_ops.flash_attn_ragged(tq, kp, vp, tcu, tl, causal=True, block_table=_dev_table(table))
    torch.cuda.synchronize()
    assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(_bits(got[1]), _bits(want[1]))
    assert not bool(torch.isnan(got[0][:43]).any())


@pytest.mark.parametrize("d,d_new", [(64, 64), (64, 48), (32, 20), (128, 128)])
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_append_places_rows_bit_for_bit_and_the_fused_call_is_the_append_then_the_attention(dtype, layout, d, d_new):
    """ragged_append against the placement rule of tests/test_ragged_cpu.py, every cache row compared as bits (zero columns past
    d_new in a written row, NaN sentinels everywhere else), contiguous and through a permuted block table; then the fused call on
    fresh caches returns the bits of append-then-attend and leaves the same caches."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    rng = np.random.default_rng(d + d_new)
    H, Hkv, Ncap = 4, 2, 512
    counts, lens = [0, 1, 1, 33, 129, 200, 5], [300, 0, 2, 33, 100, 333, 9999]
    q, kn, vn, kc, vc, cu = _fused_case(rng, dtype, H, Hkv, counts, lens, Ncap, d, d_new, tail=9)
    tq, tkn, tvn, tcu, tl = _packed(q, dtype), _packed(kn, dtype), _packed(vn, dtype), _i32(cu), _i32(lens)
    tkc, tvc = _dev(kc, layout, dtype), _dev(vc, layout, dtype)
    device_ops.ragged_append(tkn, tvn, tkc, tvc, tcu, tl, layout=layout)
    for got, new, cache in ((tkc, kn, kc), (tvc, vn, vc)):
        assert torch.equal(_bits(got), _bits(_dev(ragged_append_reference(new, cache, cu, lens), layout, dtype)))
    # the paged append writes what the contiguous one writes, in pages of 128 and of 256 rows
    for ps in (128, 256):
        table, num_pages = _table(rng, len(counts), Ncap, ps, None)
        (kp, _), (vp, _) = (_pool(_dev(c, layout, dtype), layout, ps, table, num_pages, None) for c in (kc, vc))
        device_ops.ragged_append(tkn, tvn, kp, vp, tcu, tl, layout=layout, block_table=_dev_table(table))
        assert torch.equal(_bits(_gather(kp, table, layout)), _bits(tkc)) and torch.equal(_bits(_gather(vp, table, layout)), _bits(tvc))
    # append, then attend; and the fused call on fresh caches
    out2, lse2 = device_ops.flash_attn_ragged(tq, tkc, tvc, tcu, tl, causal=True, layout=layout)
    fkc, fvc = _dev(kc, layout, dtype), _dev(vc, layout, dtype)
    out1, lse1 = _nan_out(q.shape[0], H, d_new)
    device_ops.flash_attn_ragged(tq, fkc, fvc, tcu, tl, causal=True, layout=layout, k_new=tkn, v_new=tvn, out=out1, lse=lse1)
    torch.cuda.synchronize()
    owned = int(cu[-1])
    for a, b in ((out1[:owned], out2[:owned]), (lse1[:, :owned], lse2[:, :owned]), (fkc, tkc), (fvc, tvc)):
        assert torch.equal(_bits(a), _bits(b))
    ke, ve = _after_append(kn, vn, kc, vc, cu, lens, d_new)
    _check(q, ke, ve, cu, lens, True, dtype, out1, lse1)


def test_cu_seqlens_q_is_clamped_to_the_packed_buffers():
    """Entries beyond T and a decreasing pair: [0, 40, 9999, 50] at T = 64 is, by the clamp, the sequences 0 .. 39, 40 .. 63 and an
    empty one.  The packed buffers are the fronts of larger NaN-filled allocations: a row read past T would poison the result, and
    the 16 rows behind out must stay NaN."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    rng = np.random.default_rng(77)
    dtype, H, Hkv, d, T, slack = "f32", 4, 2, 64, 64, 16
    lens = [300, NCAP, 100]
    q, kn, vn, kc, vc, _ = _fused_case(rng, dtype, H, Hkv, [40, 24, 0], lens, NCAP, d, d)
    bad, clamped = np.array([0, 40, 9999, 50], dtype=np.int32), np.array([0, 40, 64, 64], dtype=np.int32)
    assert [seq_rows(bad, T, b) for b in range(3)] == [seq_rows(clamped, T, b) for b in range(3)] == [(0, 40), (40, 64), (64, 64)]
    tkc, tvc = _dev(kc, "bnhd", dtype), _dev(vc, "bnhd", dtype)
    out = torch.full((T + slack, H, d), float("nan"), dtype=torch.float32, device="cuda")
    lse = torch.full((H, T), float("nan"), dtype=torch.float32, device="cuda")
    device_ops.flash_attn_ragged(_packed(q, dtype, slack), tkc, tvc, _i32(bad), _i32(lens), causal=True, out=out[:T], lse=lse,
                                 k_new=_packed(kn, dtype, slack), v_new=_packed(vn, dtype, slack))
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[T:]).all())
    for got, new, cache in ((tkc, kn, kc), (tvc, vn, vc)):
        assert torch.equal(_bits(got), _bits(_dev(ragged_append_reference(new, cache, clamped, lens), "bnhd", dtype)))
    ke, ve = _after_append(kn, vn, kc, vc, clamped, lens, d)
    _check(q, ke, ve, clamped, lens, True, dtype, out[:T], lse)
    # an entry below 0 is 0; and a first sequence that starts late: rows 0 .. 9 belong to nobody and are neither read nor written
    out, lse = _ragged(q, ke, ve, np.array([-7, 10, 30, 64], dtype=np.int32), lens, True, "bnhd", dtype, d)
    _check(q, ke, ve, np.array([0, 10, 30, 64]), lens, True, dtype, out, lse)
    late = np.array([10, 30, 30, 64], dtype=np.int32)
    assert seq_rows(late, T, 0) == (10, 30)
    out, lse = _ragged(q, ke, ve, late, lens, True, "bnhd", dtype, d)
    _check(q, ke, ve, late, lens, True, dtype, out, lse)


# B = 3, H = 4, Hkv = 2, T = 400, Ncap = 1000: four chunks (pinned in tests/test_ragged_cpu.py)
def _graph_case(rng, dtype="bf16"):
    H, Hkv, Ncap, d, T = 4, 2, 1000, 64, 400
    assert ((3, H, Hkv, T, Ncap, d), _splits(3, H, Hkv, T, Ncap, d, dtype)) in GPU_SPLITS
    q, kn, vn, kc, vc, _ = _fused_case(rng, dtype, H, Hkv, [400], [0], Ncap, d, d)
    kc, vc = (np.nan_to_num(np.repeat(c, 3, axis=0), nan=0.5) for c in (kc, vc))   # (every row valid for some length)
    return q, kn, vn, kc, vc


def test_repeated_calls_are_bitwise_identical():
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    for dtype in ("bf16", "f32"):
        q, kn, vn, kc, vc = _graph_case(np.random.default_rng(9), dtype)
        tq, tcu, tl = _packed(q, dtype), _i32([0, 200, 201, 390]), _i32([1000, 700, 189])
        tk, tv = _dev(kc, "bnhd", dtype), _dev(vc, "bnhd", dtype)
        a = device_ops.flash_attn_ragged(tq, tk, tv, tcu, tl, causal=True)
        b = device_ops.flash_attn_ragged(tq, tk, tv, tcu, tl, causal=True)
        torch.cuda.synchronize()
        assert torch.equal(_bits(a[0][:390]), _bits(b[0][:390])) and torch.equal(_bits(a[1][:, :390]), _bits(b[1][:, :390]))
        assert not bool(torch.isnan(a[0][:390]).any())


def test_one_fused_call_captured_in_a_graph_replays_the_eager_bits():
    """One capture at T = 400; then cu_seqlens_q, the lengths, q and the new tokens change IN PLACE (other counts, other sequences
    active) and the replay equals the eager call on fresh copies of the same caches, out, lse and cache contents alike."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    dtype = "bf16"
    q, kn, vn, kc, vc = _graph_case(np.random.default_rng(8))
    tq, tkn, tvn = _packed(q, dtype), _packed(kn, dtype), _packed(vn, dtype)
    tk, tv = _dev(kc, "bnhd", dtype), _dev(vc, "bnhd", dtype)
    k0, v0 = tk.clone(), tv.clone()
    tcu, tl = _i32([0, 200, 201, 390]), _i32([1000, 700, 189])
    ws = device_ops.ragged_workspace(tq, tk, tcu)
    out, lse = _nan_out(400, 4, 64)
    call = lambda k, v, o, l: device_ops.flash_attn_ragged(tq, k, v, tcu, tl, causal=True, out=o, lse=l, workspace=ws, k_new=tkn, v_new=tvn)
    call(tk, tv, out, lse)   # (the library is loaded and has launched once before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):   # one stream: append, schedule, split, combine
        call(tk, tv, out, lse)
    tk.copy_(k0), tv.copy_(v0)
    out.fill_(float("nan")), lse.fill_(float("nan"))
    tcu.copy_(torch.tensor([0, 0, 130, 131], dtype=torch.int32))
    tl.copy_(torch.tensor([5, 1000, 1], dtype=torch.int32))
    tq.mul_(-0.5), tkn.mul_(0.75), tvn.mul_(-1.0)
    g.replay()
    torch.cuda.synchronize()
    rk, rv = k0.clone(), v0.clone()
    ro, rl = _nan_out(400, 4, 64)
    call(rk, rv, ro, rl)
    torch.cuda.synchronize()
    for a, b in ((out, ro), (lse, rl), (tk, rk), (tv, rv)):
        assert torch.equal(_bits(a), _bits(b))
    assert bool(torch.isnan(out[131:]).all()) and not bool(torch.isnan(out[:131]).any())
    assert not torch.equal(_bits(tk), _bits(k0))


# (E, heads, kv heads): a grouped stack of head_dim 64, and an ungrouped one of head_dim 48 (rows of dp = 64 in the cache)
MODELS = [(256, 4, 2), (192, 4, 4)]


@pytest.mark.parametrize("paged", [False, True], ids=["slab", "paged"])
@pytest.mark.parametrize("E,H,Hkv", MODELS, ids=["E256-h4-kv2", "E192-h4-kv4-d48"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_model_ragged_step_matches_the_extend_step_on_each_sequence_alone(dtype, E, H, Hkv, paged):
    """Three sequences with prefixes of 100, 30 and 60 tokens take a step of 140, 0 and 1 new tokens in one attention_stack_ragged
    call; each sequence with tokens is held against attention_stack_extend on a cache of its own."""
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    L, B, cap = 4, 3, 384
    x, layers = _stack(np.random.default_rng(E + H + Hkv), dtype, B, E, H, Hkv, L, 240)
    prefix, counts = [100, 30, 60], [140, 0, 1]
    tdt = _tdt(dtype)

    def new_cache(nb):
        if paged:
            return mt.PagedKVCache(L, nb, cap, H, E // H, tdt, "cuda", n_kv_head=Hkv, page_size=128)
        return mt.KVCache(L, nb, cap, H, E // H, tdt, "cuda", n_kv_head=Hkv)
    cache = new_cache(B)
    for b, p in enumerate(prefix):   # ragged prefixes through the ragged call itself, one sequence at a time
        mt.attention_stack_ragged(x[b, :p].contiguous(), [p if i == b else 0 for i in range(B)], layers, H, cache)
    assert cache.lengths.tolist() == prefix
    packed = torch.cat([x[b, p:p + c] for b, (p, c) in enumerate(zip(prefix, counts))] + [x[0, :7]])   # (seven unused rows)
    got = mt.attention_stack_ragged(packed, counts, layers, H, cache)
    assert cache.lengths.tolist() == [p + c for p, c in zip(prefix, counts)]
    s = 0
    for b, (p, c) in enumerate(zip(prefix, counts)):
        if c:
            own = new_cache(1)
            mt.attention_stack_prefill(x[b:b + 1, :p].contiguous(), layers, H, own)
            want = to_np(mt.attention_stack_extend(x[b:b + 1, p:p + c].contiguous(), layers, H, own))[0]
            tol = _model_tol(dtype, want)
            assert maxabs(to_np(got[s:s + c]), want) < tol, (b, maxabs(to_np(got[s:s + c]), want), tol)
        s += c
