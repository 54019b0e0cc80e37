"""Paged KV cache (block tables) on the GPU.  The reference of every attention test is the CONTIGUOUS call on the gathered cache,
compared bit for bit on out and lse: a page boundary only changes where a 128-key tile is fetched from.  One case per kernel is
also held against the fp64 reference of tests/test_decode_cpu.py.  Pools are the front of larger NaN-filled buffers; unreferenced
pages, rows at or past len_b inside referenced pages, and the page that table entries past ceil(len_b / page_size) name hold NaN;
tables are random permutations."""
import numpy as np
import pytest

import oracle
from gpu_util import rand_u, to_np
from test_gpu_decode import _tdt, _to_dev, _torch
from test_gpu_decode_append import _bits, _dev, _new_and_cache, _stack
from test_gpu_extend import _check_grouped, _grouped_inputs

pytestmark = pytest.mark.gpu

HEADS = [(8, 2), (6, 2), (3, 1), (2, 2)]   # grouped (G = 4, 3, 3: a partial last block) and ungrouped: G = 1 through the grouped paged build


def _lens(Nq):
    """Ncap = 640 in pages of 128: empty, one key, around Nq (an empty prefix at Nq), around the first page boundary, a partial third
    page, full, and out of range (clamped)."""
    return [0, 1, Nq - 1, Nq, Nq + 1, 127, 128, 129, 300, 640, 9999]


def _geometry(cache, layout):
    B, dp = cache.shape[0], cache.shape[3]
    Ncap, Hkv = (cache.shape[1], cache.shape[2]) if layout == "bnhd" else (cache.shape[2], cache.shape[1])
    return B, Ncap, Hkv, dp


def _table(rng, B, Ncap, page_size, lens, extra=3):
    """A random block table (numpy int32 (B, max_pages)) for sequences of ``lens`` rows, and the pool's page count: the used slots of
    all sequences name distinct pages of a random permutation, every other slot names one of the ``extra`` unreferenced pages."""
    mp = Ncap // page_size
    assert mp * page_size == Ncap
    num_pages = B * mp + extra
    perm = rng.permutation(num_pages).astype(np.int32)
    table = np.full((B, mp), perm[B * mp], dtype=np.int32)
    for b in range(B):
        n = Ncap if lens is None else min(max(lens[b], 0), Ncap)
        used = -(-n // page_size)
        table[b, :used] = perm[b * mp:b * mp + used]
    return table, num_pages


def _pool(cache, layout, page_size, table, num_pages, lens):
    """The pool (num_pages pages, the front of a NaN buffer two pages longer) that holds the contiguous ``cache`` under ``table``:
    only the used slots' pages are copied, everything else is NaN."""
    torch = _torch()
    B, Ncap, Hkv, dp = _geometry(cache, layout)
    mp = Ncap // page_size
    if layout == "bnhd":
        pages, shape = cache.view(B, mp, page_size, Hkv, dp), (page_size, Hkv, dp)
    else:
        pages, shape = cache.view(B, Hkv, mp, page_size, dp).permute(0, 2, 1, 3, 4), (Hkv, page_size, dp)
    per = page_size * Hkv * dp
    buf = torch.full(((num_pages + 2) * per,), float("nan"), dtype=cache.dtype, device="cuda")
    pool = buf[:num_pages * per].view(num_pages, *shape)
    bi, ji = [], []
    for b in range(B):
        n = Ncap if lens is None else min(max(lens[b], 0), Ncap)
        for j in range(-(-n // page_size)):
            bi.append(b), ji.append(j)
    if bi:
        pool[torch.from_numpy(table[bi, ji]).long().cuda()] = pages[bi, ji]
    return pool, buf


def _gather(pool, table, layout):
    """The contiguous cache a table describes: (B, Ncap, Hkv, dp) or (B, Hkv, Ncap, dp)."""
    torch = _torch()
    g = pool[torch.as_tensor(table).long().to(pool.device)]   # (B, max_pages, page...)
    B, mp = g.shape[:2]
    if layout == "bnhd":
        return g.reshape(B, mp * g.shape[2], g.shape[3], g.shape[4])
    return g.permute(0, 2, 1, 3, 4).reshape(B, g.shape[2], mp * g.shape[3], g.shape[4])


def _dev_table(table):
    return _torch().from_numpy(np.ascontiguousarray(table)).cuda()


def _ops(extend):
    from flash_attention_minitorch_amd import device_ops
    return device_ops.flash_attn_extend if extend else device_ops.flash_attn_decode


def _case(rng, dtype, layout, B, H, Hkv, Nq, Ncap, d, lens, page_size):
    """numpy (q, k, v), the device q and contiguous caches, and the pools and table of the same contents."""
    torch = _torch()
    dp = 128 if d == 80 else d
    q, k, v = _grouped_inputs(rng, dtype, B, H, Hkv, Nq, Ncap, d, lens if lens is not None else [Ncap] * B)
    tq, tk, tv = _to_dev(q, layout, d, dtype), _to_dev(k, layout, dp, dtype), _to_dev(v, layout, dp, dtype)
    table, num_pages = _table(rng, B, Ncap, page_size, lens)
    (kp, _), (vp, _) = (_pool(t, layout, page_size, table, num_pages, lens) for t in (tk, tv))
    tl = None if lens is None else torch.tensor(lens, dtype=torch.int32, device="cuda")
    return (q, k, v), (tq, tk, tv, tl), (kp, vp, _dev_table(table))


def _same(extend, dev, paged, causal, layout):
    """The paged call and the contiguous call on the gathered cache: the same bits.  Returns the paged (out, lse)."""
    torch = _torch()
    tq, tk, tv, tl = dev
    kp, vp, tt = paged
    want = _ops(extend)(tq, tk, tv, tl, causal=causal, layout=layout)
    got = _ops(extend)(tq, kp, vp, tl, causal=causal, layout=layout, block_table=tt)
    for g, w in zip(got, want):
        assert torch.equal(_bits(g), _bits(w))
    assert not bool(torch.isnan(got[0]).any()) and not bool(torch.isnan(got[1]).any())
    return got


def _np_out(out, layout):
    o = to_np(out)
    return o.transpose(0, 2, 1, 3) if layout == "bnhd" else o


def _five_pages(extend, dtype, layout, d, nqs):
    """Five pages of 128 rows (Ncap = 640; by the split policies one to three chunks of 256 keys, two pages to a chunk), eleven
    lengths to a call, every head grouping, causal and not."""
    rng = np.random.default_rng(d + len(layout) + (7 if dtype == "bf16" else 0) + extend)
    Ncap, ps = 640, 128
    for Nq in nqs:
        lens = _lens(Nq)
        for H, Hkv in HEADS:
            host, dev, paged = _case(rng, dtype, layout, len(lens), H, Hkv, Nq, Ncap, d, lens, ps)
            for causal in (True, False):
                out, lse = _same(extend, dev, paged, causal, layout)
                if Nq == nqs[1] and (H, Hkv) == (6, 2) and causal:   # an independent opinion, once per kernel
                    _check_grouped(*host, lens, causal, dtype, _np_out(out, layout), to_np(lse))


@pytest.mark.parametrize("d", [32, 64, 128, 80])
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_paged_decode_equals_the_contiguous_call_bitwise(dtype, layout, d):
    _five_pages(False, dtype, layout, d, (1, 5, 33, 128))


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_paged_extend_equals_the_contiguous_call_bitwise(dtype, layout, d):
    _five_pages(True, dtype, layout, d, (129, 200, 257))


@pytest.mark.parametrize("extend", [False, True], ids=["decode-nq1", "extend-nq160"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_several_splits_and_pages_that_are_not_a_chunk(dtype, extend):
    """B = 1, H = Hkv = 2: pages of 384 rows under 9 chunks of 256 keys (a chunk starts at a page's start, its middle and its
    two-thirds point), and pages of 128 and 256 rows under 8 chunks; full, partial and page-boundary lengths; two calls agree."""
    torch = _torch()
    from flash_attention_minitorch_amd import _lib
    rng = np.random.default_rng(31 + extend)
    B, H, Nq, d = 1, 2, 160 if extend else 1, 64
    query = _lib.decode().fa_mi355x_extend_splits if extend else _lib.decode().fa_mi355x_decode_splits_gqa
    for ps, mp, ns, lens in ((384, 6, 9, (2304, 1000, 385, 384, 383)), (128, 16, 8, (2048, 1000, 129)), (256, 8, 8, (2048, 1000, 257))):
        assert query(B, H, H, Nq, ps * mp, d, 1) == ns
        for n in lens:
            host, dev, paged = _case(rng, dtype, "bnhd", B, H, H, Nq, ps * mp, d, [n], ps)
            for causal in (True, False):
                out, lse = _same(extend, dev, paged, causal, "bnhd")
            again = _ops(extend)(dev[0], paged[0], paged[1], dev[3], causal=False, layout="bnhd", block_table=paged[2])
            assert torch.equal(_bits(again[0]), _bits(out)) and torch.equal(_bits(again[1]), _bits(lse))
        _check_grouped(*host, [lens[-1]], False, dtype, _np_out(out, "bnhd"), to_np(lse))


@pytest.mark.parametrize("extend", [False, True], ids=["decode", "extend"])
def test_two_sequences_share_the_pages_of_a_prefix(extend):
    """Two table rows name the same two pages for a 256-row prefix and own pages behind it: the result is the contiguous call's on a
    cache that holds the prefix twice."""
    torch = _torch()
    rng = np.random.default_rng(5)
    B, H, Hkv, Nq, Ncap, d, ps, lens = 2, 4, 2, 130 if extend else 3, 512, 64, 128, [300, 500]
    q, k, v = _grouped_inputs(rng, "bf16", B, H, Hkv, Nq, Ncap, d, lens)
    k[1, :, :256], v[1, :, :256] = k[0, :, :256], v[0, :, :256]
    tq, tk, tv = (_to_dev(t, "bnhd", d, "bf16") for t in (q, k, v))
    table, num_pages = _table(rng, B, Ncap, ps, lens)
    (kp, _), (vp, _) = (_pool(t, "bnhd", ps, table, num_pages, lens) for t in (tk, tv))
    for pool in (kp, vp):   # the second sequence's own copies of the prefix go away: only the shared pages hold it
        pool[torch.from_numpy(table[1, :2]).long().cuda()] = float("nan")
    table[1, :2] = table[0, :2]
    tl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    _same(extend, (tq, tk, tv, tl), (kp, vp, _dev_table(table)), True, "bnhd")


@pytest.mark.parametrize("extend", [False, True], ids=["decode", "extend"])
def test_page_ids_outside_the_pool_are_clamped(extend):
    """num_pages is smaller than the allocation (the pool is the front of a NaN buffer two pages longer), so the id num_pages + 1
    unclamped would read NaN from inside the allocation: the call must equal the one with num_pages - 1 in that slot, and a negative
    id the one with 0."""
    torch = _torch()
    rng = np.random.default_rng(6)
    B, H, Hkv, Nq, d, ps, mp, num_pages = 2, 4, 2, 130 if extend else 3, 64, 128, 3, 7
    per = ps * Hkv * d
    buf = [torch.full(((num_pages + 2) * per,), float("nan"), dtype=torch.bfloat16, device="cuda") for _ in range(2)]
    kp, vp = (b[:num_pages * per].view(num_pages, ps, Hkv, d) for b in buf)
    for pool in (kp, vp):
        pool.copy_(torch.from_numpy(oracle.bf16_round(rand_u(rng, tuple(pool.shape)))))
    tq = torch.from_numpy(oracle.bf16_round(rand_u(rng, (B, Nq, H, d)))).to("cuda", torch.bfloat16)
    tl = torch.tensor([mp * ps, 200], dtype=torch.int32, device="cuda")
    good = np.array([[2, 5, 1], [3, 4, 9999]], dtype=np.int32)   # (the last slot of the second row is past its length: never read)
    run = lambda t: _ops(extend)(tq, kp, vp, tl, causal=True, block_table=_dev_table(np.array(t, dtype=np.int32)))
    for bad, clamped in ((num_pages + 1, num_pages - 1), (1 << 30, num_pages - 1), (-1, 0), (-(1 << 31), 0)):
        for slot in ((0, 1), (1, 0)):
            t_bad, t_ok = good.copy(), good.copy()
            t_bad[slot], t_ok[slot] = bad, clamped
            got, want = run(t_bad), run(t_ok)
            assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(_bits(got[1]), _bits(want[1])), (bad, slot)
            assert not bool(torch.isnan(got[0]).any())
    ref = run(good)
    assert not torch.equal(_bits(ref[0]), _bits(want[0]))   # (the slot does matter: another page, another result)


# (d, d_new, Nq, source offset in elements): 16-byte lanes, zero columns behind d_new, element lanes (20 of bf16: 40 bytes), a
# source one element past a 16-byte boundary, and 128 tokens
APPENDS = [(64, 64, 3, 0), (64, 48, 3, 0), (32, 20, 3, 0), (64, 64, 3, 1), (128, 128, 128, 0)]


def _offset(t, shift):
    torch = _torch()
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device="cuda")
    view = buf[shift:shift + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == shift * t.element_size()
    return view


def _append_case(dtype, layout, extend, d, d_new, Nq, shift, lens, Ncap, ps, seed):
    """The paged append into a NaN-patterned pool against the contiguous append into the cache of the same contents: the whole
    buffer behind the pool (unreferenced pages and the two pages past num_pages included) equals the paginated contiguous result."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    rng = np.random.default_rng(seed)
    B, Hkv = len(lens), 3
    (kn, vn), (kc, vc) = _new_and_cache(rng, dtype, B, Nq, Hkv, Ncap, d, d_new)
    tkn, tvn = (_offset(_dev(x, layout, dtype), shift) for x in (kn, vn))
    tkc, tvc = _dev(kc, layout, dtype), _dev(vc, layout, dtype)
    table, num_pages = _table(rng, B, Ncap, ps, lens)
    (kp, kbuf), (vp, vbuf) = (_pool(t, layout, ps, table, num_pages, lens) for t in (tkc, tvc))
    tl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    append = device_ops.extend_append if extend else device_ops.decode_append
    append(tkn, tvn, tkc, tvc, tl, layout=layout)
    append(tkn, tvn, kp, vp, tl, layout=layout, block_table=_dev_table(table))
    for cache, pool, buf in ((tkc, kp, kbuf), (tvc, vp, vbuf)):
        want_pool, want_buf = _pool(cache, layout, ps, table, num_pages, lens)
        assert torch.equal(_bits(buf), _bits(want_buf)), (d, d_new, Nq, shift)
        # gathered back, the valid rows are the contiguous cache's
        got = _gather(pool, table, layout)
        for b, n in enumerate(lens):
            n = min(max(n, 0), Ncap)
            rows = (lambda t: t[b, :n]) if layout == "bnhd" else (lambda t: t[b, :, :n])
            assert torch.equal(_bits(rows(got)), _bits(rows(cache))), b


@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_paged_append_places_rows_bit_for_bit(dtype, layout):
    """Three pages of 128 rows: nothing to write, len < Nq, tokens that straddle the first page boundary (len - Nq < 128 <= len), the
    first rows of a page, an interior page, full, out of range."""
    for i, (d, d_new, Nq, shift) in enumerate(APPENDS):
        lens = [0, 1, Nq - 1, 129, 128 + Nq, 300, 384, 9999] if Nq < 128 else [0, 127, 128, 129, 200, 300, 384, 9999]
        _append_case(dtype, layout, False, d, d_new, Nq, shift, lens, 384, 128, 40 + i)


@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_paged_extend_append_of_200_tokens_over_three_pages(dtype, layout):
    _append_case(dtype, layout, True, 64, 48, 200, 0, [200, 384, 330, 100, 0, 9999], 384, 128, 50)
    _append_case(dtype, layout, True, 64, 64, 200, 0, [700, 768, 201], 768, 384, 51)   # pages of 384 rows (not a power of two)


@pytest.mark.parametrize("extend", [False, True], ids=["decode-nq3", "extend-nq200"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_fused_paged_call_is_the_append_then_the_attention(dtype, extend):
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    rng = np.random.default_rng(70 + extend)
    H, Hkv, Nq, Ncap, d, d_new, ps = 6, 3, 200 if extend else 3, 640, 64, 48, 128
    lens = [640, 2, 300, 129, 9999] if not extend else [640, 100, 300, 328, 9999]
    B = len(lens)
    q = rand_u(rng, (B, H, Nq, d_new))
    if dtype == "bf16":
        q = oracle.bf16_round(q)
    (kn, vn), (kc, vc) = _new_and_cache(rng, dtype, B, Nq, Hkv, Ncap, d, d_new)
    for b, n in enumerate(lens):
        first = max(min(n, Ncap) - Nq, 0)
        for c in (kc, vc):
            c[b, first:] = np.nan                 # the rows about to be written, and the invalid ones behind them
            c[b, :first, :, d_new:] = 0           # (valid older rows: zero columns, as a padded cache holds them)
            c[b, :first:7, :, 0] = 0.25
    tq, tkn, tvn = _to_dev(q, "bnhd", d_new, dtype), _dev(kn, "bnhd", dtype), _dev(vn, "bnhd", dtype)
    tl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    table, num_pages = _table(rng, B, Ncap, ps, lens)
    tt = _dev_table(table)
    append = device_ops.extend_append if extend else device_ops.decode_append
    runs = []
    for fused in (True, True, False):
        (kp, kbuf), (vp, vbuf) = (_pool(_dev(c, "bnhd", dtype), "bnhd", ps, table, num_pages, lens) for c in (kc, vc))
        if fused:
            out, lse = _ops(extend)(tq, kp, vp, tl, causal=True, k_new=tkn, v_new=tvn, block_table=tt)
        else:
            append(tkn, tvn, kp, vp, tl, block_table=tt)
            out, lse = _ops(extend)(tq, kp, vp, tl, causal=True, block_table=tt)
        runs.append((out, lse, kbuf, vbuf))
    for other in runs[1:]:   # a repeated fused call, then the two separate calls: the same bits, in the results and in the pools
        for a, b in zip(runs[0], other):
            assert torch.equal(_bits(a), _bits(b))
    # and the contiguous fused call on the gathered cache
    tkc, tvc = _dev(kc, "bnhd", dtype), _dev(vc, "bnhd", dtype)
    want = _ops(extend)(tq, tkc, tvc, tl, causal=True, k_new=tkn, v_new=tvn)
    assert torch.equal(_bits(want[0]), _bits(runs[0][0])) and torch.equal(_bits(want[1]), _bits(runs[0][1]))
    assert not bool(torch.isnan(runs[0][0]).any())


def test_fused_paged_call_replays_in_a_graph_with_lengths_advanced_and_the_table_edited_in_place():
    """Three captured steps of one token (a single-branch graph): the lengths advance inside the graph, and the second sequence
    crosses a page boundary on the way (126 -> 129 rows), its second page written into the table in place between two replays.
    Every replay returns the bits of the eager CONTIGUOUS fused call, and the pools end as its caches."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    rng = np.random.default_rng(12)
    B, H, Hkv, Ncap, d, ps, steps = 2, 8, 2, 4096, 128, 128, 3
    start = [3000, 126]
    final = [s + steps for s in start]
    q = oracle.bf16_round(rand_u(rng, (B, H, steps + 1, d)))
    (kn, vn), (kc, vc) = _new_and_cache(rng, "bf16", B, steps + 1, Hkv, Ncap, d, d)
    for b, n in enumerate(start):
        for c in (kc, vc):
            c[b, n:] = np.nan
            c[b, :n:7, :, 0] = 0.25
    dev = lambda x: _dev(x, "bnhd", "bf16")
    tq_all, tkn_all, tvn_all = _to_dev(q, "bnhd", d, "bf16"), dev(kn), dev(vn)
    sq, sk, sv = (t[:, :1].contiguous() for t in (tq_all, tkn_all, tvn_all))    # the graph's static inputs
    table, num_pages = _table(rng, B, Ncap, ps, final)
    held_back = int(table[1, 1])
    first = table.copy()
    first[1, 1] = table[1, 2]   # (an unreferenced NaN page until the sequence reaches row 128)
    tt = _dev_table(first)
    ws = device_ops.decode_workspace(sq, dev(kc))
    ws_paged = device_ops.decode_workspace(sq, _pool(dev(kc), "bnhd", ps, table, num_pages, final)[0], block_table=tt)
    assert ws is not None and ws_paged.numel() == ws.numel()

    def feed(i):
        for dst, src in ((sq, tq_all), (sk, tkn_all), (sv, tvn_all)):
            dst.copy_(src[:, i:i + 1])

    new_out = lambda: (torch.empty(sq.shape, dtype=torch.float32, device="cuda"), torch.empty((B, H, 1), dtype=torch.float32, device="cuda"))
    eager_c, eager_l, eager = (dev(kc), dev(vc)), torch.tensor(start, dtype=torch.int32, device="cuda"), []
    for i in range(steps):
        feed(i)
        eager_l.add_(1)
        o, l = device_ops.flash_attn_decode(sq, eager_c[0], eager_c[1], eager_l, causal=True, workspace=ws, k_new=sk, v_new=sv)
        eager.append((o.clone(), l.clone()))
    pools = [_pool(dev(c), "bnhd", ps, table, num_pages, start) for c in (kc, vc)]
    graph_l = torch.tensor(start, dtype=torch.int32, device="cuda")
    out, lse = new_out()

    def run():
        return device_ops.flash_attn_decode(sq, pools[0][0], pools[1][0], graph_l, causal=True, out=out, lse=lse, workspace=ws_paged,
                                            k_new=sk, v_new=sv, block_table=tt)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):   # a warm-up call at the length the first replay uses: its row is written again
        feed(steps)
        graph_l.add_(1)
        run()
        graph_l.sub_(1)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graph_l.add_(1)
        run()
    addr = tt.data_ptr()
    for i in range(steps):
        feed(i)
        if start[1] + i + 1 > ps:   # this step writes row 128: the sequence gets its second page, in place
            tt[1, 1] = held_back
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[i][0]) and torch.equal(lse, eager[i][1]), i
    assert tt.data_ptr() == addr and graph_l.tolist() == final
    for (pool, _), cache in zip(pools, eager_c):
        got = _gather(pool, table, "bnhd")
        for b, n in enumerate(final):
            assert torch.equal(_bits(got[b, :n]), _bits(cache[b, :n])), b


MODELS = [(256, 4, 4), (192, 4, 2)]   # (E, heads, kv heads): head_dim 64 ungrouped; head_dim 48 with 2 kv heads, d_new = 48 into rows of 64


def _caches(dtype, E, H, Hkv, L, B, n_pages):
    from flash_attention_minitorch_amd import modules_transformer as mt
    tdt = _tdt(dtype)
    return (mt.PagedKVCache(L, B, 512, H, E // H, tdt, "cuda", n_kv_head=Hkv, page_size=128, n_pages=n_pages),
            mt.KVCache(L, B, 512, H, E // H, tdt, "cuda", n_kv_head=Hkv))


def _same_caches(paged, slab):
    torch = _torch()
    assert paged.lengths.tolist() == slab.lengths.tolist() and paged.length_bound == slab.length_bound
    lens = slab.lengths.tolist()
    table = paged.block_table.cpu().numpy()
    for pool, cache in zip(paged.k + paged.v, slab.k + slab.v):
        for b, n in enumerate(lens):
            own = paged.pages[b]
            assert len(own) >= -(-n // paged.page_size) and table[b, :len(own)].tolist() == own
            got = pool[torch.tensor(own).long().cuda()].reshape(-1, *pool.shape[2:])
            assert torch.equal(_bits(got[:n]), _bits(cache[b, :n])), b


@pytest.mark.parametrize("E,H,Hkv", MODELS, ids=["E256-h4-kv4", "E192-h4-kv2-d48"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_model_on_a_paged_cache_equals_the_model_on_a_slab(dtype, E, H, Hkv):
    """A PagedKVCache with fewer pages than B * max_pages against a KVCache of the same capacity, bit for bit in every output and on
    every valid cache row: prefill and fused steps across a page boundary, an extend of 160 tokens, chunked prefill, and captured
    steps across a page boundary."""
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    rng = np.random.default_rng(E + H)
    B, L, P = 2, 2, 122
    x, layers = _stack(rng, dtype, B, E, H, Hkv, L, 300)
    eq = lambda a, b: torch.equal(_bits(a), _bits(b))

    paged, slab = _caches(dtype, E, H, Hkv, L, B, 6)   # 6 pages for two sequences that could take 4 each
    assert paged.n_pages < B * paged.max_pages
    outs = [mt.attention_stack_prefill(x[:, :P].contiguous(), layers, H, c) for c in (paged, slab)]
    assert eq(*outs) and [len(p) for p in paged.pages] == [1, 1]
    for c in (paged, slab):   # (the second prompt is shorter: lengths differ per batch element)
        c.lengths.copy_(torch.tensor([P, P - 7], dtype=torch.int32))
    for i in range(8):        # rows 122 .. 129 of the first sequence: a second page from the seventh step on
        xi = x[:, P + i:P + i + 1].contiguous()
        assert eq(*[mt.attention_stack_step_fused(xi, layers, H, c) for c in (paged, slab)]), i
    assert [len(p) for p in paged.pages] == [2, 2]
    _same_caches(paged, slab)
    xt = x[:, 130:290].contiguous()   # 160 tokens: the extend kernels, into the second and third page
    assert eq(*[mt.attention_stack_extend(xt, layers, H, c) for c in (paged, slab)])
    assert [len(p) for p in paged.pages] == [3, 3] and not paged.free
    _same_caches(paged, slab)
    with pytest.raises(RuntimeError, match="exhausted"):
        mt.attention_stack_extend(xt, layers, H, paged)
    with pytest.raises(ValueError, match="attention_stack_step_fused"):
        mt.attention_stack_step(x[:, :1].contiguous(), layers, H, paged)

    # chunked prefill into the same caches: the finished sequences' pages come back first
    paged.release(0), paged.release(1)
    assert len(paged.free) == 6
    outs = [mt.attention_stack_prefill_chunked(x, layers, H, c, 130) for c in (paged, slab)]   # pieces of 130, 130 and 40 tokens
    assert eq(*outs)
    _same_caches(paged, slab)

    # captured steps across a page boundary: 126 -> 130 rows
    paged, slab = _caches(dtype, E, H, Hkv, L, B, 5)
    outs = [mt.attention_stack_prefill(x[:, :126].contiguous(), layers, H, c) for c in (paged, slab)]
    assert eq(*outs)
    steppers = [mt.GraphedStep(layers, H, c, 1) for c in (paged, slab)]
    table_addr = paged.block_table.data_ptr()
    for i in range(4):
        xi = x[:, 126 + i:127 + i].contiguous()
        assert eq(*[s.step(xi).clone() for s in steppers]), i
    assert paged.block_table.data_ptr() == table_addr and [len(p) for p in paged.pages] == [2, 2]
    _same_caches(paged, slab)
