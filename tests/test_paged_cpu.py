"""CPU-side checks of the paged KV cache (block tables; include/flash_attn_mi355x_decode_paged.h): the six entry points
declared, exported and bound; every bad argument answered with its code and a message that names it before any HIP call (fake
non-null pointers, as in tests/test_decode_cpu.py: a launch would fail with another code); the Python checks of the four device_ops
functions; PagedKVCache's page bookkeeping on the host; and the model layer's C calls under the recorder."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "flash_attn_mi355x_decode_paged.h")   # (flash_attn_mi355x_decode.h includes it)
PAGED = ["fa_mi355x_fwd_decode_paged", "fa_mi355x_decode_append_paged", "fa_mi355x_fwd_decode_append_paged",
         "fa_mi355x_fwd_extend_paged", "fa_mi355x_extend_append_paged", "fa_mi355x_fwd_extend_append_paged"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from flash_attention_minitorch_amd import _lib
    return _lib


def test_the_six_paged_symbols_are_declared_exported_and_bound(built):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert '#include "flash_attn_mi355x_decode_paged.h"' in open(os.path.join(ROOT, "include", "flash_attn_mi355x_decode.h")).read()
    assert sorted(set(re.findall(r"\b(fa_mi355x_\w+)\s*\(", text))) == sorted(PAGED) == sorted(built.PAGED_ABI)
    lib = built.decode()
    for s in PAGED:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % s, text)
        assert m, s
        params = [p.strip() for p in m.group(1).split(",")]
        assert "const int* block_table" in params and params[params.index("const int* block_table") - 1] == "const int* cache_seqlens", s
        i = params.index("int num_pages")
        assert params[i:i + 3] == ["int num_pages", "int page_size", "int max_pages"] and "int Ncap" not in params, s
        assert hasattr(lib, s), s
        res, args = built.PAGED_ABI[s]
        assert res is ctypes.c_int and len(args) == len(params), s
        assert getattr(lib, s).argtypes == args
    assert re.search(r"#define\s+FA_PAGE_ROWS\s+128\b", open(HEADER).read()) and built.FA_PAGE_ROWS == 128


# one valid call of each form (fake non-null device pointers); one split, so no workspace is needed unless a case asks for one
_ONE = 16
_GOOD = dict(q=_ONE, kn=_ONE, vn=_ONE, k=_ONE, v=_ONE, out=_ONE, lse=_ONE, lens=_ONE, table=_ONE, ws=_ONE, B=1, H=4, Hkv=2, Nq=1,
             num_pages=8, page_size=128, max_pages=2, d_new=64, d=64, layout=1, scale=0.0, causal=1, dtype=1)
_VP = ctypes.c_void_p


def _call(lib, sym, **over):
    a = dict(_GOOD, **over)
    fused, append = "_append_" in sym and "fwd" in sym, "fwd" not in sym
    if append:
        args = [_VP(a[n]) for n in ("kn", "vn", "k", "v", "lens", "table")] + [a[n] for n in (
            "B", "Hkv", "Nq", "num_pages", "page_size", "max_pages", "d_new", "d", "layout", "dtype")] + [None]
    else:
        ptrs = ("q", "kn", "vn", "k", "v", "out", "lse", "lens", "table", "ws") if fused else ("q", "k", "v", "out", "lse", "lens", "table", "ws")
        dims = ("d_new", "d") if fused else ("d",)
        args = [_VP(a[n]) for n in ptrs] + [a[n] for n in ("B", "H", "Hkv", "Nq", "num_pages", "page_size", "max_pages") + dims] + [
            a["layout"], a["scale"], a["causal"], a["dtype"], None]
    rc = getattr(lib, sym)(*args)
    return rc, lib.fa_mi355x_decode_last_error().decode()


# (field, value, code, message) that every form rejects: the paging arguments, and what the forms share with the contiguous ones
_PAGING = [
    ("table", 0, 1, "block_table"),
    ("page_size", 0, 1, "page_size"), ("page_size", 64, 1, "page_size"), ("page_size", 129, 1, "page_size"), ("page_size", -128, 1, "page_size"),
    ("num_pages", 0, 1, "num_pages"), ("num_pages", -3, 1, "num_pages"),
    ("max_pages", 0, 1, "max_pages"), ("max_pages", -1, 1, "max_pages"),
    ("max_pages", 1 << 24, 1, "max_pages * page_size"),    # 2^24 * 128 = 2^31
    ("page_size", 1 << 24, 1, "2 GiB"),                    # 2^24 rows * 2 heads * 64 * 2 bytes = 2^32 bytes in one page
    ("k", 0, 1, "null"), ("v", 0, 1, "null"),
    ("B", 0, 1, "positive"), ("Hkv", 0, 1, "positive"), ("Nq", 0, 1, "positive"), ("d", 0, 1, "positive"),
    ("layout", 2, 1, "layout"), ("dtype", 5, 1, "dtype"),
    ("d", 48, 2, "32, 64, 128"), ("d", 256, 2, "32, 64, 128"),
]
_ATTEND = [
    ("q", 0, 1, "null"), ("out", 0, 1, "null"), ("H", 0, 1, "positive"), ("H", 3, 1, "multiple of Hkv"),
    ("scale", -1.0, 1, "softmax_scale"), ("scale", float("nan"), 1, "softmax_scale"), ("scale", float("inf"), 1, "softmax_scale"),
]
_APPEND = [("kn", 0, 1, "null"), ("vn", 0, 1, "null"), ("d_new", 0, 1, "d_new"), ("d_new", 65, 1, "d_new")]


def _cases():
    out = []
    for sym in PAGED:
        bad = list(_PAGING)
        if "fwd" in sym:
            bad += _ATTEND
        if "append" in sym:   # (the fused forms reject what either half rejects)
            bad += _APPEND
        out += [(sym, f, v, c, m) for f, v, c, m in bad]
    return out


@pytest.mark.parametrize("sym,field,value,code,msg", _cases(), ids=[f"{s[10:]}-{f}={v}" for s, f, v, _, _ in _cases()])
def test_paged_forms_reject_each_bad_argument_before_any_hip_call(built, sym, field, value, code, msg):
    rc, err = _call(built.decode(), sym, **{field: value})
    assert rc == code and err and msg in err, (rc, err)


@pytest.mark.parametrize("sym", PAGED)
def test_more_than_128_queries_only_through_the_extend_forms(built, sym):
    """The extend forms take Nq = 129 past their Nq check: the answer comes from a check BEHIND it (the null workspace of a
    several-split call, d_new out of range), never about Nq.  (A call that passes every check would launch on the fake pointers.)"""
    lib = built.decode()
    behind = dict(max_pages=32, ws=0) if "fwd" in sym else dict(d_new=65)
    rc, err = _call(lib, sym, Nq=129, **behind)
    if "extend" in sym:
        assert rc == 1 and ("workspace" if "fwd" in sym else "d_new") in err and "Nq" not in err, (rc, err)
    else:
        assert rc == 1 and "Nq > 128" in err, (rc, err)


@pytest.mark.parametrize("sym", [s for s in PAGED if "fwd" in s])
def test_a_split_paged_call_needs_the_contiguous_calls_workspace(built, sym):
    """The paged call's splits are the contiguous call's for Ncap = max_pages * page_size: 32 pages of 128 rows are 4096 keys, which
    one sequence of 4 heads takes in several splits, so a null workspace is an error there and the last check made."""
    lib = built.decode()
    query = lib.fa_mi355x_extend_splits if "extend" in sym else lib.fa_mi355x_decode_splits_gqa
    assert query(1, 4, 2, 1, 32 * 128, 64, 1) > 1 and query(1, 4, 2, 1, 2 * 128, 64, 1) == 1
    rc, err = _call(lib, sym, max_pages=32, ws=0, lse=0, lens=0)
    assert rc == 1 and "workspace" in err, (rc, err)


def test_device_ops_python_checks(built):
    import torch
    from flash_attention_minitorch_amd import device_ops

    B, H, Hkv, d = 2, 4, 2, 64
    q = torch.zeros(B, 1, H, d)
    kp, vp = torch.zeros(6, 128, Hkv, d), torch.zeros(6, 128, Hkv, d)
    kn = torch.zeros(B, 1, Hkv, d)
    tbl = torch.zeros(B, 3, dtype=torch.int32)
    attend = [device_ops.flash_attn_decode, device_ops.flash_attn_extend]
    append = [device_ops.decode_append, device_ops.extend_append]
    calls = [lambda k, v, t, f=f: f(q, k, v, block_table=t) for f in attend] + [lambda k, v, t, f=f: f(kn, kn, k, v, block_table=t) for f in append]
    for call in calls:
        with pytest.raises(ValueError, match="4-d"):                      # the pool's rank
            call(kp[0], vp[0], tbl)
        with pytest.raises(ValueError, match="one shape"):                # K and V pools that differ
            call(kp, torch.zeros(5, 128, Hkv, d), tbl)
        with pytest.raises(ValueError, match="page_size"):                # a page of 64 rows, of 192 rows
            call(torch.zeros(6, 64, Hkv, d), torch.zeros(6, 64, Hkv, d), tbl)
        with pytest.raises(ValueError, match="page_size"):
            call(torch.zeros(6, 192, Hkv, d), torch.zeros(6, 192, Hkv, d), tbl)
        with pytest.raises(ValueError, match="block_table"):              # the table's dtype, rank, batch, contiguity, device
            call(kp, vp, tbl.long())
        with pytest.raises(ValueError, match="block_table"):
            call(kp, vp, tbl[0])
        with pytest.raises(ValueError, match="block_table"):
            call(kp, vp, torch.zeros(B + 1, 3, dtype=torch.int32))
        with pytest.raises(ValueError, match="block_table"):
            call(kp, vp, torch.zeros(B, 6, dtype=torch.int32)[:, ::2])
        with pytest.raises(ValueError, match="block_table"):
            call(kp, vp, torch.zeros(B, 3, dtype=torch.int32, device="meta"))
        with pytest.raises(built.FlashAttnLibraryError, match="GPU"):     # all checks passed: CPU tensors are the only thing wrong
            call(kp, vp, tbl)
    # "bhnd": the page size is the pool's third dimension
    with pytest.raises(ValueError, match="page_size"):
        device_ops.flash_attn_decode(q.transpose(1, 2).contiguous(), kp, vp, layout="bhnd", block_table=tbl)
    # the pool's heads must divide q's; the new tokens' heads are the pool's
    with pytest.raises(ValueError, match="heads"):
        device_ops.flash_attn_decode(q, torch.zeros(6, 128, 3, d), torch.zeros(6, 128, 3, d), block_table=tbl)
    with pytest.raises(ValueError, match=r"\(B, Hkv\)"):
        device_ops.decode_append(torch.zeros(B, 1, 4, d), torch.zeros(B, 1, 4, d), kp, vp, block_table=tbl)


def test_workspace_helpers_size_a_paged_call_like_the_contiguous_one(built):
    import torch
    from flash_attention_minitorch_amd import device_ops

    lib = built.decode()
    q = torch.zeros(1, 1, 8, 128)
    pool = torch.zeros(40, 256, 2, 128)
    tbl = torch.zeros(1, 16, dtype=torch.int32)
    want = lib.fa_mi355x_decode_workspace_bytes_gqa(1, 8, 2, 1, 16 * 256, 128)
    assert want > 0
    for kw in (dict(block_table=tbl), dict(max_pages=16)):
        ws = device_ops.decode_workspace(q, pool, "bnhd", **kw)
        assert ws.numel() * 4 == want
    q = torch.zeros(1, 200, 8, 128)
    want = lib.fa_mi355x_extend_workspace_bytes(1, 8, 2, 200, 16 * 256, 128)
    assert want > 0 and device_ops.extend_workspace(q, pool, "bnhd", block_table=tbl).numel() * 4 == want
    assert device_ops.decode_workspace(torch.zeros(64, 1, 8, 128), pool, "bnhd", max_pages=1) is None
    with pytest.raises(ValueError, match="max_pages"):
        device_ops.decode_workspace(q, pool, "bnhd", max_pages=0)


def test_paged_kv_cache_hands_out_and_takes_back_pages(built):
    import torch
    from flash_attention_minitorch_amd import modules_transformer as mt

    c = mt.PagedKVCache(2, 3, 1000, 4, 48, torch.float32, "cpu", n_kv_head=2, page_size=256)
    assert c.max_pages == 4 and c.n_pages == 12 and c.dp == 64
    assert c.block_table.shape == (3, 4) and c.block_table.dtype == torch.int32
    assert len(c.k) == len(c.v) == 2 and all(t.shape == (12, 256, 2, 64) for t in c.k + c.v)
    addr = c.block_table.data_ptr()
    c.reserve(257)                                     # two pages each
    t = c.block_table.tolist()
    owned = [p for row in t for p in row[:2]]
    assert len(set(owned)) == 6 and [row[:2] for row in t] == c.pages and len(c.free) == 6
    c.reserve(256)                                     # already owned: nothing changes
    assert c.block_table.tolist() == t and len(c.free) == 6
    c.reserve(1000, rows=[1])                          # one sequence grows to its four pages; its first two stay
    t2 = c.block_table.tolist()
    assert t2[0] == t[0] and t2[2] == t[2] and t2[1][:2] == t[1][:2] and len(set(t2[1])) == 4 and len(c.free) == 4
    assert c.block_table.data_ptr() == addr
    with pytest.raises(ValueError, match="exceed"):
        c.reserve(1025)

    # a pool smaller than B * max_pages serves ragged reservations, and says what is missing when it runs out
    c = mt.PagedKVCache(1, 3, 1024, 4, 64, torch.float32, "cpu", page_size=128, n_pages=10)
    assert c.max_pages == 8
    c.reserve(1024, rows=[0])
    c.reserve(128, rows=[1, 2])
    assert [len(p) for p in c.pages] == [8, 1, 1] and not c.free
    assert len({p for own in c.pages for p in own}) == 10
    before = c.block_table.clone()
    with pytest.raises(RuntimeError, match=r"2 more pages needed.*0 of 10 free"):
        c.reserve(256, rows=[1, 2])
    assert torch.equal(c.block_table, before) and [len(p) for p in c.pages] == [8, 1, 1]   # nothing handed out
    # release: the pages come back, the length goes to zero, and the next reserve reuses them
    c.lengths.fill_(100)
    gone = list(c.pages[0])
    addr = c.block_table.data_ptr()
    c.release(0)
    assert c.lengths.tolist() == [0, 100, 100] and c.pages[0] == [] and sorted(c.free) == sorted(gone)
    c.reserve(512, rows=[1])
    assert c.pages[1][1:] == gone[:3] and c.block_table[1, :4].tolist() == c.pages[1]
    assert c.block_table.data_ptr() == addr
    with pytest.raises(ValueError, match="page_size"):
        mt.PagedKVCache(1, 1, 256, 4, 64, torch.float32, "cpu", page_size=100)


def test_model_layer_reserves_and_passes_the_table_under_the_recorder(monkeypatch):
    """The C calls of the stack functions on a PagedKVCache under the recorder of tests/test_device_ops_cpu.py (CPU tensors, no
    library): the pages are reserved before a call is made, and every call is the _paged form with the cache's table after the
    lengths and (n_pages, page_size, max_pages) where the capacity stood."""
    import torch
    from flash_attention_minitorch_amd import modules_transformer as mt
    from test_device_ops_cpu import install_recorder

    rec = install_recorder(monkeypatch)
    B, P, T, H, Hkv, d, cap, ps, npg = 2, 16, 200, 4, 2, 48, 512, 128, 7
    g = torch.Generator().manual_seed(0)
    x, xt = (torch.randn(s, generator=g).to(torch.bfloat16) for s in ((B, P, H * d), (B, T, H * d)))
    wq, wk = (torch.randn(s, generator=g).to(torch.bfloat16) for s in ((H * d, H * d), (H * d, Hkv * d)))
    layers = [(wq, wk, wk, wq)] * 2
    cache = mt.PagedKVCache(2, B, cap, H, d, torch.bfloat16, x.device, n_kv_head=Hkv, page_size=ps, n_pages=npg)
    owned = []   # pages per sequence at the time of every library call
    reserve = cache.reserve

    def spy(n, rows=None):
        reserve(n, rows)
        owned.append(("reserve", n))
    cache.reserve = spy

    def own():
        return [len(p) for p in cache.pages]
    geometry = f"{npg},{ps},{cap // ps}"

    rec.reset({"table": cache.block_table, "lens": cache.lengths})
    mt.attention_stack_prefill(x, layers, H, cache)
    calls = [c for c in rec.calls if c.startswith("fa_mi355x_extend_append_paged(")]
    # k_new, v_new, pool, pool, lens, table, B, Hkv, Nq, num_pages, page_size, max_pages, d_new, d, layout, dtype, stream
    assert len(calls) == 2 and all(c.endswith(f",lens,table,{B},{Hkv},{P},{geometry},48,64,1,1,null)") for c in calls), rec.calls
    assert owned[0] == ("reserve", P) and own() == [1, 1] and cache.lengths.tolist() == [P] * B and cache.length_bound == P

    rec.reset({"table": cache.block_table})
    mt.attention_stack_extend(xt, layers, H, cache)   # 216 rows: a second page each
    calls = [c for c in rec.calls if "workspace_bytes" not in c]
    assert len(calls) == 2 and all(c.startswith("fa_mi355x_fwd_extend_append_paged(") for c in calls), calls
    # ... lens, table, workspace, B, H, Hkv, Nq, num_pages, page_size, max_pages, d_new, d, layout, scale, causal, dtype, stream
    assert all(re.search(r",table,\w+,%d,%d,%d,%d,%s,48,64,1,%s,1,1,null\)$" % (B, H, Hkv, T, geometry, re.escape(repr(48 ** -0.5))), c)
               for c in calls), calls
    sizes = [c for c in rec.calls if "workspace_bytes" in c]
    assert sizes and all(c == f"fa_mi355x_extend_workspace_bytes({B},{H},{Hkv},{T},{cap},64)" for c in sizes), sizes
    assert owned[-1] == ("reserve", P + T) and own() == [2, 2] and cache.length_bound == P + T

    rec.reset({"table": cache.block_table})
    mt.attention_stack_step_fused(xt[:, :5].contiguous(), layers, H, cache)
    calls = [c for c in rec.calls if "workspace_bytes" not in c]
    assert len(calls) == 2 and all(c.startswith("fa_mi355x_fwd_decode_append_paged(") and ",table," in c for c in calls), calls
    assert owned[-1] == ("reserve", P + T + 5) and own() == [2, 2]
    with pytest.raises(ValueError, match="attention_stack_step_fused"):
        mt.attention_stack_step(xt[:, :1].contiguous(), layers, H, cache)

    # 421 rows are four pages each, eight of a pool of seven: the error names the shortfall before any call is made
    rec.reset({"table": cache.block_table})
    with pytest.raises(RuntimeError, match="exhausted"):
        mt.attention_stack_extend(torch.zeros(B, 200, H * d, dtype=torch.bfloat16), layers, H, cache)
    assert not [c for c in rec.calls if "workspace_bytes" not in c]

    rec.reset({"table": cache.block_table})
    cache.release(0), cache.release(1)
    y = mt.attention_stack_prefill_chunked(torch.cat([x, xt], 1), layers, H, cache, 130)   # pieces of 130 and 86 tokens
    calls = [c.split("(")[0] for c in rec.calls if "workspace_bytes" not in c]
    assert calls == ["fa_mi355x_fwd_extend_append_paged"] * 2 + ["fa_mi355x_fwd_decode_append_paged"] * 2, calls
    assert y.shape == (B, P + T, H * d) and cache.length_bound == P + T and own() == [2, 2]
