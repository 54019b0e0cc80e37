"""FP8 (e4m3) KV cache on the GPU (include/flash_attn_mi355x_decode_fp8.h).  Most checks are equalities: every e4m3 value is a bf16
value and the kernels widen a staged tile to the bf16 image the bf16 kernels compute on, so an fp8 call must return what the bf16
call returns on the cache cast to bf16 (with power-of-two scales, which commute with every rounding), a paged call what the slab
call returns, the fused call what append-then-attend returns, and the append the bytes of this suite's ``quantize``
(tests/test_fp8_cpu.py).  One group of cases is held against the fp64 reference with scales that are not powers of two.
"Bit for bit" is checked on the int32 view, except where a sum is known to turn a -0 into a +0 (noted there).  Caches hold the NaN
code 0x7F at and past every length and in unreferenced pages: none of it may reach a result."""
import numpy as np
import pytest

from gpu_util import to_np
from test_fp8_cpu import NAN_CODES, TABLE, fp8_reference, quantize
from test_gpu_decode import TOL

pytestmark = pytest.mark.gpu

LOG2E = np.float32(1.4426950408889634)
STALE = 0x7F
NCAP = 384
LENS = [0, 1, 127, 128, 129, 257, NCAP]   # empty, one key, around a super tile, a partial third tile, full (clamped on the device)
HEADS = [(2, 2), (8, 2), (4, 1)]          # G = 1, G = 4, and one cache head (multi-query)


def _torch():
    import torch
    return torch


def _ops(extend):
    from flash_attention_minitorch_amd import device_ops
    return device_ops.flash_attn_extend if extend else device_ops.flash_attn_decode


def _f8(codes):
    """uint8 codes -> the same bytes as a float8_e4m3fn tensor (what device_ops takes)."""
    return codes.view(_torch().float8_e4m3fn)


def _widen(codes):
    """uint8 codes -> bf16 by this suite's decode table (exact: every e4m3 value is a bf16 value; the NaN codes give NaN)."""
    torch = _torch()
    table = torch.from_numpy(TABLE.astype(np.float32)).to(codes.device)
    return table[codes.long()].to(torch.bfloat16)


def _bits(t):
    return t.contiguous().view(_torch().int32)


def _codes(gen, shape):
    """Random bytes with the two NaN codes remapped (to 0x3C and 0xBC: +-1.5)."""
    torch = _torch()
    c = torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=gen)
    return torch.where((c & 0x7F) == 0x7F, (c & 0x80) | 0x3C, c)


def _cache(gen, layout, B, Hkv, Ncap, d, lens):
    """uint8 k, v caches in ``layout`` with random codes below each length and the NaN code at and past it."""
    torch = _torch()
    out = []
    for _ in range(2):
        c = _codes(gen, (B, Ncap, Hkv, d))
        for b, n in enumerate(lens):
            c[b, min(max(n, 0), Ncap):] = STALE
        out.append(c if layout == "bnhd" else c.transpose(1, 2).contiguous())
    return out


def _q(gen, layout, B, H, Nq, d):
    torch = _torch()
    q = (torch.rand((B, Nq, H, d), device="cuda", generator=gen) * 2 - 1).to(torch.bfloat16)
    return q if layout == "bnhd" else q.transpose(1, 2).contiguous()


def _per_head(vs, G, layout):
    """(Hkv,) scales -> a factor for an out tensor in ``layout``: query head h reads cache head h // G."""
    f = vs.repeat_interleave(G)
    return f[None, None, :, None] if layout == "bnhd" else f[None, :, None, None]


def _pow2_scales(Hkv):
    torch = _torch()
    ks = torch.full((Hkv,), 2.0 ** -6, device="cuda")   # one power of two for all heads: scores of order 1 on codes of up to 448
    vs = torch.tensor([2.0 ** (1 - 3 * h) for h in range(Hkv)], device="cuda")   # 2, 1/4, ...
    return ks, vs


def _same_as_bf16(extend, q, k8, v8, tl, ks, vs, causal, layout, tau, G, **paging_of_fp8):
    """fp8_call(q, k8, v8, scales) == bf16_call(q, bf16(k8), bf16(v8), softmax_scale = tau * k_scale) * v_scale[head], out and lse."""
    torch = _torch()
    got = _ops(extend)(q, _f8(k8), _f8(v8), tl, causal=causal, softmax_scale=tau, layout=layout, k_scale=ks, v_scale=vs, **paging_of_fp8)
    want = _ops(extend)(q, _widen(k8), _widen(v8), tl, causal=causal, softmax_scale=tau * float(ks[0]), layout=layout)
    assert torch.equal(_bits(got[0]), _bits(want[0] * _per_head(vs, G, layout)))
    assert torch.equal(_bits(got[1]), _bits(want[1]))
    assert not bool(torch.isnan(got[0]).any()) and not bool(torch.isnan(got[1]).any())
    return got


# ---- 1. every code, exactly ----

def _exact_tau():
    """A softmax scale tau for which c = fp32(tau * log2(e)), the kernels' exp2 constant, is exactly 2^-3 (and so for tau times a
    power of two): m * c is then exact, the row maximum's own weight is exp2(0) = 1 and l = 1 with no rounding, so that
    lse = fp32(m * tau) + ln 1 is the single product the check names.  (With an inexact c the kernel's exp2(fma(s, c, -fp32(m c)))
    is 1 + O(2^-24 m c) for the maximum itself, in the bf16 kernels as well: the lse is then more accurate than one rounded product,
    not equal to it.)  The products near 2^-3 step by 1.44 ulp(tau) and 1.5 such ulps round to 2^-3, so one exists."""
    t = np.float32(0.125) / LOG2E
    for _ in range(8):
        t = np.nextafter(t, np.float32(0))
    for _ in range(16):
        if np.float32(t * LOG2E) == np.float32(0.125):
            return t
        t = np.nextafter(t, np.float32(1))
    raise AssertionError("no fp32 tau with fp32(tau * log2(e)) == 2^-3")


def _one_row_cache(layout, row, Hkv, d, paged):
    """Caches of 128 rows whose row 0 is ``row`` (nb, Hkv, d) uint8 and whose other rows are stale; paged: one page per sequence under
    a reversed table, and two unreferenced stale pages."""
    torch = _torch()
    nb = row.shape[0]
    c = torch.full((nb + (2 if paged else 0), 128, Hkv, d), STALE, dtype=torch.uint8, device="cuda")
    table = None
    if paged:
        ids = torch.arange(nb - 1, -1, -1, device="cuda")
        c[ids, 0] = row
        table = ids.to(torch.int32)[:, None].contiguous()
    else:
        c[:, 0] = row
    return (c if layout == "bnhd" else c.transpose(1, 2).contiguous()), table


@pytest.mark.parametrize("paged", [False, True], ids=["slab", "paged"])
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_every_code_reaches_the_output_exactly_through_v(d, layout, paged):
    """len = 1, Nq = 1, q = 0 and a zero K row: P = 1 exactly, so out = fp32(v_scale * value) of V row 0, which carries the 256 codes
    one per column over ceil(256 / d) batch elements; NaN in the two NaN columns only.  Compared as values: the accumulator starts
    from +0, so the code 0x80 (-0) comes out as +0."""
    torch = _torch()
    nb, H, Hkv = -(-256 // d), 4, 2
    codes = (torch.arange(nb * d, device="cuda") % 256).to(torch.uint8).view(nb, 1, d).expand(nb, Hkv, d).contiguous()
    vs = torch.tensor([0.3, 1.7], device="cuda")
    v8, table = _one_row_cache(layout, codes, Hkv, d, paged)
    k8, _ = _one_row_cache(layout, torch.zeros_like(codes), Hkv, d, paged)
    q = torch.zeros((nb, 1, H, d) if layout == "bnhd" else (nb, H, 1, d), dtype=torch.bfloat16, device="cuda")
    tl = torch.ones(nb, dtype=torch.int32, device="cuda")
    for extend in (False, True):
        out, lse = _ops(extend)(q, _f8(k8), _f8(v8), tl, layout=layout, v_scale=vs, **(dict(block_table=table) if paged else {}))
        o = to_np(out).reshape(nb, H, d)
        want = TABLE[to_np(codes).astype(np.uint8)].astype(np.float32)[:, [0, 0, 1, 1]] * to_np(vs)[[0, 0, 1, 1]][None, :, None].astype(np.float32)
        nan = np.isin(to_np(codes).astype(np.uint8)[:, [0, 0, 1, 1]], NAN_CODES)
        assert nan.sum() == 2 * H and np.array_equal(np.isnan(o), nan)
        assert np.array_equal(o[~nan], want[~nan])
        assert np.all(to_np(lse) == 0)   # (one key with score 0)


@pytest.mark.parametrize("paged", [False, True], ids=["slab", "paged"])
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_every_code_reaches_the_score_exactly_through_k(d, layout, paged):
    """len = 1, Nq = d one-hot queries, not causal: query i's only score is the value of column i of K row 0, and
    lse[i] = fp32(fp32(tau * k_scale) * value) with _exact_tau and power-of-two scales per head.  The 254 finite codes; the two NaN
    codes sit in a batch element of their own, which must come out as a NaN in a valid row of a bf16 cache does: out NaN, and the lse
    the bf16 call gives on the widened row, never a finite one.  (The kernels' row maximum is an fmaxf, which drops a NaN score: l
    becomes NaN, fails the l > 0 test and the lse is stored as that of an empty row; the test prints what it is.)  Compared as
    values: m * tau + ln 1 turns the -0 of code 0x80 into +0."""
    torch = _torch()
    nb, H, Hkv = -(-256 // d), 4, 2
    codes = (torch.arange(nb * d, device="cuda") % 256).to(torch.uint8)
    codes = torch.where((codes & 0x7F) == 0x7F, torch.zeros_like(codes), codes).view(nb, 1, d).expand(nb, Hkv, d)
    own = torch.zeros((1, Hkv, d), dtype=torch.uint8, device="cuda")
    own[0, :, 3], own[0, :, 5] = 0x7F, 0xFF
    codes = torch.cat([codes, own]).contiguous()
    k8, table = _one_row_cache(layout, codes, Hkv, d, paged)
    v8, _ = _one_row_cache(layout, torch.full_like(codes, 0x38), Hkv, d, paged)   # V row 0 = 1.0 everywhere
    eye = torch.eye(d, dtype=torch.bfloat16, device="cuda")
    q = eye[None, :, None, :].expand(nb + 1, d, H, d).contiguous() if layout == "bnhd" else eye[None, None].expand(nb + 1, H, d, d).contiguous()
    tl = torch.ones(nb + 1, dtype=torch.int32, device="cuda")
    tau, ks, vs = _exact_tau(), torch.tensor([0.5, 2.0], device="cuda"), torch.tensor([0.3, 1.7], device="cuda")
    ids = slice(0, 1) if paged else slice(nb, nb + 1)   # the NaN element's slab, or its page under the reversed table
    tau8 = (np.float32(tau) * np.array([0.5, 0.5, 2.0, 2.0], dtype=np.float32)).astype(np.float32)   # per query head
    want = (tau8[None, :, None] * TABLE[to_np(codes).astype(np.uint8)].astype(np.float32)[:nb][:, [0, 0, 1, 1]]).astype(np.float32)
    for extend in (False, True):
        out, lse = _ops(extend)(q, _f8(k8), _f8(v8), tl, causal=False, softmax_scale=float(tau), layout=layout, k_scale=ks, v_scale=vs,
                                **(dict(block_table=table) if paged else {}))
        l = to_np(lse)
        assert l.shape == (nb + 1, H, d) and np.array_equal(l[:nb], want)
        # the NaN codes: what a NaN in a valid row of a bf16 cache gives
        bo, bl = _ops(extend)(q[nb:], _widen(k8)[ids], _widen(v8)[ids], tl[nb:], causal=False, softmax_scale=float(tau), layout=layout)
        print(f"NaN codes in K row 0 ({'extend' if extend else 'decode'}): lse {np.unique(l[nb])}, bf16 cache {np.unique(to_np(bl))}")
        assert bool(torch.isnan(out[nb]).all()) and bool(torch.isnan(bo).all())
        assert np.array_equal(l[nb:], to_np(bl), equal_nan=True) and not np.any(np.isfinite(l[nb]))
        o = to_np(out)[:nb]   # one key: out = v_scale * 1.0
        o = o.transpose(0, 2, 1, 3) if layout == "bnhd" else o
        assert np.array_equal(o, np.broadcast_to(to_np(vs)[[0, 0, 1, 1]][None, :, None, None], o.shape))


# ---- 2. bit for bit against the bf16 call ----

@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("extend", [False, True], ids=["decode", "extend"])
def test_fp8_call_equals_the_bf16_call_on_the_widened_cache(extend, layout):
    torch = _torch()
    gen = torch.Generator(device="cuda").manual_seed(11 + extend)
    from flash_attention_minitorch_amd import _lib
    splits = _lib.decode().fa_mi355x_extend_splits if extend else _lib.decode().fa_mi355x_decode_splits_gqa
    # Ncap = 384: two chunks of 256 keys and the combine kernel; Ncap = 256: one chunk, written directly by the split kernel
    for Ncap, lens in ((NCAP, LENS), (256, [0, 1, 127, 128, 129, 255, 256])):
        tl = torch.tensor(lens, dtype=torch.int32, device="cuda")
        for d in (32, 64, 128):
            for H, Hkv in HEADS:
                ks, vs = _pow2_scales(Hkv)
                k8, v8 = _cache(gen, layout, len(lens), Hkv, Ncap, d, lens)
                for Nq in ((1, 129, 257, 400) if extend else (1, 3, 33, 128)):
                    assert splits(len(lens), H, Hkv, Nq, Ncap, d, 1) == (2 if Ncap == NCAP else 1)
                    q = _q(gen, layout, len(lens), H, Nq, d)
                    for causal in (True, False):
                        _same_as_bf16(extend, q, k8, v8, tl, ks, vs, causal, layout, d ** -0.5, H // Hkv)


def test_fp8_call_equals_the_bf16_call_over_several_splits():
    """The shapes whose partials go through the workspace and the combine kernel (which reads both scales)."""
    torch = _torch()
    from flash_attention_minitorch_amd import _lib
    lib = _lib.decode()
    assert lib.fa_mi355x_decode_splits(1, 2, 1, 4096, 64, 1) > 1 and lib.fa_mi355x_extend_splits(1, 4, 2, 129, 4096, 64, 1) > 1
    assert lib.fa_mi355x_decode_splits_gqa(2, 8, 2, 3, 4096, 128, 1) > 1
    gen = torch.Generator(device="cuda").manual_seed(5)
    for extend, B, H, Hkv, Nq, d, lens in ((False, 1, 2, 2, 1, 64, [4096]), (False, 2, 8, 2, 3, 128, [4000, 700]), (True, 1, 4, 2, 129, 64, [3333])):
        ks, vs = _pow2_scales(Hkv)
        k8, v8 = _cache(gen, "bnhd", B, Hkv, 4096, d, lens)
        tl = torch.tensor(lens, dtype=torch.int32, device="cuda")
        _same_as_bf16(extend, _q(gen, "bnhd", B, H, Nq, d), k8, v8, tl, ks, vs, True, "bnhd", d ** -0.5, H // Hkv)


def _paged_copy(slab, layout, page_size, lens, gen):
    """A pool that holds ``slab`` (uint8, in ``layout``) under a permuted table; unreferenced pages and slots hold the NaN code."""
    torch = _torch()
    s = slab if layout == "bnhd" else slab.transpose(1, 2)
    B, Ncap, Hkv, d = s.shape
    mp = Ncap // page_size
    num_pages = B * mp + 3
    perm = torch.randperm(num_pages, device="cuda", generator=gen)
    table = perm[B * mp].repeat(B, mp)
    pool = torch.full((num_pages, page_size, Hkv, d), STALE, dtype=torch.uint8, device="cuda")
    for b, n in enumerate(lens):
        for j in range(-(-min(max(n, 0), Ncap) // page_size)):
            table[b, j] = perm[b * mp + j]
            pool[perm[b * mp + j]] = s[b, j * page_size:(j + 1) * page_size]
    return (pool if layout == "bnhd" else pool.transpose(1, 2).contiguous()), table.to(torch.int32).contiguous()


@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("page_size", [128, 256])
def test_paged_fp8_call_equals_the_slab_fp8_call(page_size, layout):
    torch = _torch()
    gen = torch.Generator(device="cuda").manual_seed(page_size)
    Ncap, lens = 512, [0, 129, 300, 512, 256]
    tl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    for d, (H, Hkv) in ((32, (8, 2)), (64, (2, 2)), (128, (4, 1))):
        ks, vs = _pow2_scales(Hkv)
        k8, v8 = _cache(gen, layout, len(lens), Hkv, Ncap, d, lens)
        (kp, table), (vp, _) = (_paged_copy(t, layout, page_size, lens, torch.Generator(device="cuda").manual_seed(3)) for t in (k8, v8))
        for extend, Nq in ((False, 1), (False, 33), (True, 257)):
            q = _q(gen, layout, len(lens), H, Nq, d)
            want = _ops(extend)(q, _f8(k8), _f8(v8), tl, layout=layout, k_scale=ks, v_scale=vs)
            got = _ops(extend)(q, _f8(kp), _f8(vp), tl, layout=layout, k_scale=ks, v_scale=vs, block_table=table)
            assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(_bits(got[1]), _bits(want[1]))
            assert not bool(torch.isnan(got[0]).any())


# ---- 3. oracle parity with real scales ----

@pytest.mark.parametrize("extend,B,H,Hkv,Nq,Ncap,d,lens", [
    (False, 3, 4, 2, 3, 256, 64, [256, 1, 131]), (False, 1, 2, 2, 1, 4096, 64, [4096]), (False, 2, 8, 2, 1, 4096, 128, [4096, 2500]),
    (True, 2, 4, 2, 200, 256, 128, [256, 230]), (True, 1, 4, 2, 129, 4096, 64, [3500])],
    ids=["decode-one-split-d64", "decode-splits-d64", "decode-splits-d128", "extend-one-split-d128", "extend-splits-d64"])
def test_fp8_call_against_the_fp64_reference_with_real_scales(extend, B, H, Hkv, Nq, Ncap, d, lens):
    """k, v ~ U(-1, 1), per-head scales amax / 448 (not powers of two), quantised by this suite's reference; out and lse against
    fp8_reference within the suite's bf16 envelope (TOL["bf16"] of tests/test_gpu_decode.py: the same kernel arithmetic on inputs of
    the same magnitude)."""
    torch = _torch()
    from flash_attention_minitorch_amd import _lib
    ns = (_lib.decode().fa_mi355x_extend_splits if extend else _lib.decode().fa_mi355x_decode_splits_gqa)(B, H, Hkv, Nq, Ncap, d, 1)
    assert (ns > 1) == (Ncap == 4096)
    rng = np.random.default_rng(d + Nq)
    G = H // Hkv
    k, v = (rng.uniform(-1, 1, (B, Hkv, Ncap, d)).astype(np.float32) for _ in range(2))
    q = torch.from_numpy(rng.uniform(-1, 1, (B, H, Nq, d)).astype(np.float32)).to(torch.bfloat16)
    ks, vs = (np.abs(t).max(axis=(0, 2, 3)).astype(np.float32) / np.float32(448) for t in (k, v))
    k8, v8 = quantize(k, ks[None, :, None, None]), quantize(v, vs[None, :, None, None])
    for b, n in enumerate(lens):
        k8[b, :, n:] = v8[b, :, n:] = STALE
    dev = lambda a: torch.from_numpy(a).cuda()
    out, lse = _ops(extend)(q.cuda(), _f8(dev(k8)), _f8(dev(v8)), torch.tensor(lens, dtype=torch.int32, device="cuda"), layout="bhnd",
                            k_scale=dev(ks), v_scale=dev(vs))
    rep = lambda a: np.repeat(a, G, axis=1).reshape(B * H, *a.shape[2:])
    ro, rl = fp8_reference(q.float().numpy().reshape(B * H, Nq, d), rep(k8), rep(v8), np.tile(np.repeat(ks, G), B), np.tile(np.repeat(vs, G), B),
                           np.repeat(lens, H), True, d ** -0.5)
    gl = to_np(lse).reshape(B * H, Nq)
    empty = np.isneginf(rl)   # (rows at negative positions: lens[b] < Nq)
    assert np.array_equal(np.isneginf(gl), empty) and empty.sum() == (2 * H if Nq == 3 else 0)
    eo, el = np.abs(to_np(out).reshape(B * H, Nq, d) - ro).max(), np.abs(gl[~empty] - rl[~empty]).max()
    print(f"fp8 vs fp64: out {eo:.3e} lse {el:.3e}")
    assert eo < TOL["bf16"] and el < TOL["bf16"], (eo, el)


# ---- 4. append ----

def _new_tokens(rng, B, Nq, Hkv, d_new, scales):
    """bf16 new tokens (B, Nq, Hkv, d_new) as fp32 numpy: values across each head's whole range, beyond it, tiny ones, and in the
    first row of every head +-448 s, +-500 s, +-0, 2^-9 s, 2^-10 s and NaN."""
    torch = _torch()
    s = np.asarray(scales, dtype=np.float32)[None, None, :, None]
    x = rng.uniform(-1, 1, (B, Nq, Hkv, d_new)).astype(np.float32) * s * np.float32(448 * 1.2)
    x[:, 1::3] *= np.float32(2.0 ** -7)
    x[:, 2::5] *= np.float32(2.0 ** -14)
    special = np.array([448, -448, 500, -500, 0.0, -0.0, 2.0 ** -9, 2.0 ** -10, -2.0 ** -10, np.nan, 1e30, -1e30], dtype=np.float32)
    x[:, 0, :, :len(special)] = special * s[:, 0]   # (s > 0: the zeros keep their signs)
    return torch.from_numpy(x).to(torch.bfloat16)


def _expected_cache(before, x, lens, scales, Ncap):
    """The bnhd cache bytes after the append: row clamp(len) - Nq + i of batch b holds quantize(x[b, i]) and zero columns; rows below
    0 are not written; everything else keeps ``before``."""
    want = before.copy()
    B, Nq, Hkv, d_new = x.shape
    codes = quantize(x, np.asarray(scales, dtype=np.float32)[None, None, :, None])
    for b in range(B):
        L = min(max(lens[b], 0), Ncap)
        for i in range(Nq):
            if L - Nq + i >= 0:
                want[b, L - Nq + i] = 0
                want[b, L - Nq + i, :, :d_new] = codes[b, i]
    return want


@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("scales", [([0.5, 2.0], [4.0, 0.25]), ([0.3, 1.7], [0.0123, 3.3])], ids=["pow2", "real"])
def test_append_stores_the_reference_quantisation_byte_for_byte(scales, layout):
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    rng = np.random.default_rng(7)
    B, Hkv, H, Ncap, d = 4, 2, 4, 256, 64
    ksn, vsn = scales
    ks, vs = torch.tensor(ksn, device="cuda"), torch.tensor(vsn, device="cuda")
    to_layout = lambda t: t if layout == "bnhd" else t.transpose(1, 2).contiguous()
    for Nq, append, lens in ((5, device_ops.decode_append, [256, 3, 100, 5]), (130, device_ops.extend_append, [256, 129, 131, 9999])):
        tl = torch.tensor(lens, dtype=torch.int32, device="cuda")
        for d_new in (d, d - 8, d - 3):   # the vector build, the vector build with zero columns, the element build
            kx, vx = _new_tokens(rng, B, Nq, Hkv, d_new, ksn), _new_tokens(rng, B, Nq, Hkv, d_new, vsn)
            before = rng.integers(0, 256, (2, B, Ncap, Hkv, d)).astype(np.uint8)
            wk, wv = (_expected_cache(before[i], t.float().numpy(), lens, s, Ncap) for i, (t, s) in enumerate(((kx, ksn), (vx, vsn))))
            # slab
            kc, vc = (to_layout(torch.from_numpy(before[i]).cuda()) for i in range(2))
            append(to_layout(kx.cuda()), to_layout(vx.cuda()), _f8(kc), _f8(vc), tl, layout, k_scale=ks, v_scale=vs)
            assert np.array_equal(to_layout(kc).cpu().numpy(), wk) and np.array_equal(to_layout(vc).cpu().numpy(), wv), (Nq, d_new)
            # paged: the same bytes under a permuted table, and nothing written to an unreferenced page
            gen = torch.Generator(device="cuda").manual_seed(d_new)
            full = [Ncap] * B
            (kp, table), (vp, _) = (_paged_copy(to_layout(torch.from_numpy(before[i]).cuda()), layout, 128, full, torch.Generator(device="cuda").manual_seed(1))
                                    for i in range(2))
            append(to_layout(kx.cuda()), to_layout(vx.cuda()), _f8(kp), _f8(vp), tl, layout, block_table=table, k_scale=ks, v_scale=vs)
            for pool, want in ((kp, wk), (vp, wv)):
                pages = (pool if layout == "bnhd" else pool.transpose(1, 2))[table.long()]   # (B, mp, 128, Hkv, d)
                assert np.array_equal(pages.reshape(B, Ncap, Hkv, d).cpu().numpy(), want), (Nq, d_new)
                used = torch.zeros(pool.shape[0], dtype=torch.bool, device="cuda")
                used[table.long().flatten()] = True
                assert bool((pool[~used] == STALE).all())
            # the fused call: append-then-attend, bit for bit, and the same bytes
            q = _q(gen, layout, B, H, Nq, d)
            extend = Nq > 128
            k2, v2 = (to_layout(torch.from_numpy(before[i]).cuda()) for i in range(2))
            got = _ops(extend)(q, _f8(k2), _f8(v2), tl, layout=layout, k_new=to_layout(kx.cuda()), v_new=to_layout(vx.cuda()), k_scale=ks, v_scale=vs)
            want = _ops(extend)(q, _f8(kc), _f8(vc), tl, layout=layout, k_scale=ks, v_scale=vs)
            assert torch.equal(k2, kc) and torch.equal(v2, vc)
            assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(_bits(got[1]), _bits(want[1]))


# ---- 5. the model layer ----

def _requant(t):
    """dequantise(quantise(t)) with torch, scales 1: what an fp8 cache holds of the bf16 rows t."""
    torch = _torch()
    return t.float().clamp(-448, 448).to(torch.float8_e4m3fn).to(torch.bfloat16)


def _shadow_run(x, layers, H, Hkv, cap, P, steps, T):
    """The fp8 stack by hand on a bf16 slab cache: after each append the new rows are replaced by _requant(rows).  Returns the
    outputs of the prefill, of every one-token step and of the T-token extend, and the caches."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops, modules_transformer as mt
    B, _, E = x.shape
    d = E // H
    kc = [torch.zeros((B, cap, Hkv, d), dtype=torch.bfloat16, device="cuda") for _ in layers]
    vc = [torch.zeros((B, cap, Hkv, d), dtype=torch.bfloat16, device="cuda") for _ in layers]
    outs, n, pos = [], P, 0
    for count in [P] + [1] * steps + [T]:
        h = x[:, pos:pos + count].contiguous()
        first = pos == 0
        lo = 0 if first else n
        n = count if first else n + count
        new_len = torch.full((B,), n, dtype=torch.int32, device="cuda")
        for li, (wq, wk, wv, wo) in enumerate(layers):
            q, k, v = mt._project(h, wq, wk, wv, H)
            kc[li][:, lo:n], vc[li][:, lo:n] = _requant(k), _requant(v)
            if first:   # the prompt's own attention: the square forward on the unquantised k, v
                o, _, _ = device_ops.flash_attn_fwd_gqa(q, k, v, True, 2)
            else:
                o, _ = (device_ops.flash_attn_extend if count > 128 else device_ops.flash_attn_decode)(q, kc[li], vc[li], new_len, causal=True, layout="bnhd")
            h = h + (o.reshape(B * count, E).to(h.dtype) @ wo).view(B, count, E)
        outs.append(h)
        pos += count
    return outs, kc, vc


def _model_inputs():
    torch = _torch()
    g = torch.Generator().manual_seed(0)
    B, E, H, Hkv, P, T = 2, 128, 4, 2, 130, 200
    d = E // H
    x = (torch.randn((B, P + 3 + T, E), generator=g) * 0.5).to(torch.bfloat16).cuda()
    mk = lambda n: (torch.randn((E, n), generator=g) * E ** -0.5).to(torch.bfloat16).cuda()
    layers = [(mk(E), mk(Hkv * d), mk(Hkv * d), mk(E)) for _ in range(2)]
    return x, layers, B, E, H, Hkv, P, T


@pytest.mark.parametrize("paged", [False, True], ids=["slab", "paged"])
def test_model_on_an_fp8_cache_equals_the_shadow_loop(paged):
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    x, layers, B, E, H, Hkv, P, T = _model_inputs()
    cap, d = 512, E // H
    want, kc, vc = _shadow_run(x, layers, H, Hkv, cap, P, 3, T)
    kw = dict(n_kv_head=Hkv, kv_dtype=torch.float8_e4m3fn, kv_scale=(torch.ones(2, Hkv), torch.ones(2, Hkv)))
    cache = (mt.PagedKVCache(2, B, cap, H, d, torch.bfloat16, "cuda", page_size=128, **kw) if paged else
             mt.KVCache(2, B, cap, H, d, torch.bfloat16, "cuda", **kw))
    got = [mt.attention_stack_prefill(x[:, :P].contiguous(), layers, H, cache)]
    for s in range(3):
        got.append(mt.attention_stack_step_fused(x[:, P + s:P + s + 1].contiguous(), layers, H, cache))
    got.append(mt.attention_stack_extend(x[:, P + 3:].contiguous(), layers, H, cache))
    for g, w in zip(got, want):
        assert g.shape == w.shape and torch.equal(g.view(torch.int16), w.view(torch.int16))
    n = P + 3 + T
    assert cache.length_bound == n and cache.lengths.tolist() == [n] * B
    for li in range(2):
        for c8, ref in ((cache.k[li], kc[li]), (cache.v[li], vc[li])):
            rows = c8.view(torch.uint8)
            if paged:
                rows = rows[cache.block_table.long()].reshape(B, -1, Hkv, d)
            assert torch.equal(_widen(rows[:, :n]).view(torch.int16), ref[:, :n].view(torch.int16))
    for bad in (lambda: mt.attention_stack_step(x[:, :1].contiguous(), layers, H, cache),
                lambda: mt.attention_stack_ragged(x[0, :8].contiguous(), [4, 4], layers, H, cache),
                lambda: mt.KVCache(2, B, cap, H, d, torch.bfloat16, "cuda", window=64, **kw)):
        with pytest.raises(ValueError):
            bad()


def test_graphed_step_on_an_fp8_cache_equals_the_eager_fused_step():
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    x, layers, B, E, H, Hkv, P, T = _model_inputs()
    kw = dict(n_kv_head=Hkv, kv_dtype=torch.float8_e4m3fn, kv_scale=(torch.full((2, Hkv), 0.5), torch.full((2, Hkv), 2.0)))
    eager, graphed = (mt.KVCache(2, B, 512, H, E // H, torch.bfloat16, "cuda", **kw) for _ in range(2))
    for c in (eager, graphed):
        mt.attention_stack_prefill(x[:, :P].contiguous(), layers, H, c)
    step = mt.GraphedStep(layers, H, graphed)
    for s in range(3):
        tok = x[:, P + s:P + s + 1].contiguous()
        w = mt.attention_stack_step_fused(tok, layers, H, eager)
        g = step.step(tok)
        assert torch.equal(g.view(torch.int16), w.view(torch.int16)), s
    assert graphed.lengths.tolist() == eager.lengths.tolist() == [P + 3] * B
    for li in range(2):
        assert torch.equal(graphed.k[li].view(torch.uint8), eager.k[li].view(torch.uint8))
        assert torch.equal(graphed.v[li].view(torch.uint8), eager.v[li].view(torch.uint8))


# ---- 6. the other calls are untouched ----

def test_a_bf16_call_after_fp8_calls_returns_what_it_returned_before():
    torch = _torch()
    gen = torch.Generator(device="cuda").manual_seed(2)
    lens = [300, 77]
    tl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    k8, v8 = _cache(gen, "bnhd", 2, 2, NCAP, 64, lens)
    q = _q(gen, "bnhd", 2, 8, 3, 64)
    kb, vb = _widen(k8).nan_to_num(0.0), _widen(v8).nan_to_num(0.0)
    before = _ops(False)(q, kb, vb, tl, layout="bnhd")
    ks, vs = _pow2_scales(2)
    _ops(False)(q, _f8(k8), _f8(v8), tl, layout="bnhd", k_scale=ks, v_scale=vs)
    _ops(True)(q, _f8(k8), _f8(v8), tl, layout="bnhd", k_scale=ks, v_scale=vs)
    after = _ops(False)(q, kb, vb, tl, layout="bnhd")
    assert torch.equal(_bits(before[0]), _bits(after[0])) and torch.equal(_bits(before[1]), _bits(after[1]))
