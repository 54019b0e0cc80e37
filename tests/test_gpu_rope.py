"""Rotary embeddings on the GPU (include/flash_attn_mi355x_decode_rope.h).  The rotation itself has a DERIVED tolerance against the
fp64 ``rope_reference`` of tests/test_rope_cpu.py on the same rounded inputs and fp32 tables,
    |err| <= u * |exact| + 2^-22 * (|x1| + |x2|),   u = 2^-8 (bf16: one rounding of an 8-bit significand) or 0 (fp32),
the second term bounding three fp32 roundings with |c|, |s| <= 1.  Everything else is bit for bit: law 1, the fused rope_append is
apply_rotary on q and k_new followed by the family's plain append (q_rot and the ENTIRE caches, pre-filled with a sentinel); law 2, a
roped attention call is the unroped call on the rotated q and k_new (out, lse, caches)."""
import math

import numpy as np
import pytest

import oracle
from gpu_util import maxabs, rand_u, to_np
from test_decode_cpu import decode_reference
from test_rope_cpu import rope_bound, rope_reference, rope_tables

pytestmark = pytest.mark.gpu

U = {"f32": 0.0, "bf16": 2.0 ** -8}
TOL = {"f32": 1e-4, "bf16": 1e-3}   # tests/test_gpu_decode.py, the unroped call
MAX_POS = 256


def _torch():
    import torch
    return torch


def _tdt(dtype):
    torch = _torch()
    return torch.bfloat16 if dtype == "bf16" else torch.float32


def _dev():
    from flash_attention_minitorch_amd import device_ops
    return device_ops


def _bits(t):
    torch = _torch()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _same(a, b):
    return bool(_torch().equal(_bits(a), _bits(b)))


_TABLES = {}


def _tables(rot, max_pos=MAX_POS):
    """(cos, sin) as numpy fp32 and as device tensors, once per shape."""
    if (rot, max_pos) not in _TABLES:
        torch = _torch()
        c, s = rope_tables(max_pos, rot)
        _TABLES[rot, max_pos] = (c, s, torch.from_numpy(c).cuda(), torch.from_numpy(s).cuda())
    return _TABLES[rot, max_pos]


def _rand(rng, shape, dtype, scale=1.0):
    """fp32 numpy values that the dtype holds exactly, and the device tensor."""
    torch = _torch()
    x = rand_u(rng, shape) * np.float32(scale)
    if dtype == "bf16":
        x = oracle.bf16_round(x)
    return x, torch.from_numpy(x).to("cuda", _tdt(dtype))


def _assert_rotated(got, x, c, s, pos, dtype, il, inverse=False, what=""):
    """got (numpy, x's shape) against rope_reference(x) within the derived bound; columns >= rot must be x's, exactly."""
    exact = rope_reference(x, c, s, pos, il, inverse)
    bound = U[dtype] * np.abs(exact) + rope_bound(x, c, U[dtype], il)
    err = np.abs(got.astype(np.float64) - exact)
    assert np.all(err <= bound), (what, float(err.max()), float((err - bound).max()))
    rot = 2 * c.shape[1]
    assert np.array_equal(got[..., rot:], x[..., rot:]), what


# ---- fa_mi355x_rope / apply_rotary ----

@pytest.mark.parametrize("interleaved", [False, True], ids=["neox", "gptj"])
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_apply_rotary_is_the_fp64_rotation_within_the_derived_bound(dtype, layout, interleaved):
    """B = 2, N = 5, H = 3, d in {32, 64, 128}, rot in {d, d / 2, 6} (6: the element build), offsets None, [0, 37] and [-3, 250] (both
    clamps: positions below 0 and, with 256 table rows, above 255); in place; the inverse; columns >= rot bitwise."""
    torch, dev = _torch(), _dev()
    rng = np.random.default_rng(17)
    B, N, H = 2, 5, 3
    for d in (32, 64, 128):
        for rot in (d, d // 2, 6):
            c, s, tc, ts = _tables(rot)
            shape = (B, N, H, d) if layout == "bnhd" else (B, H, N, d)
            x, tx = _rand(rng, shape, dtype, 2.0)
            for offs in (None, [0, 37], [-3, 250]):
                to = None if offs is None else torch.tensor(offs, dtype=torch.int32, device="cuda")
                pos = np.asarray(offs or [0, 0])[:, None] + np.arange(N)[None, :]             # (B, N)
                pos = pos[:, :, None] if layout == "bnhd" else pos[:, None, :]
                what = (d, rot, offs)
                y = dev.apply_rotary(tx, tc, ts, to, interleaved, layout=layout)
                assert y.dtype == tx.dtype and y.shape == tx.shape and y.data_ptr() != tx.data_ptr()
                _assert_rotated(to_np(y), x, c, s, pos, dtype, interleaved, what=what)
                assert np.array_equal(to_np(tx), x)                                            # (the source is left alone)
                yi = dev.apply_rotary(tx, tc, ts, to, interleaved, inverse=True, layout=layout)
                _assert_rotated(to_np(yi), x, c, s, pos, dtype, interleaved, inverse=True, what=what)
                z = tx.clone()
                assert dev.apply_rotary(z, tc, ts, to, interleaved, layout=layout, out=z) is z and _same(z, y), what   # in place: the same bits
                out = torch.full_like(tx, 3.0)
                assert dev.apply_rotary(tx, tc, ts, to, interleaved, layout=layout, out=out) is out and _same(out, y), what


def test_rotary_table_on_the_device_and_a_misaligned_view_takes_the_element_build():
    """rotary_table(device=) is the fp64 table rounded once; a tensor whose storage starts 4 bytes off a 16-byte boundary (legal:
    contiguous, but no vector lane) gives the bits of the aligned call."""
    torch, dev = _torch(), _dev()
    cos, sin = dev.rotary_table(MAX_POS, 64, device="cuda")
    c, s = rope_tables(MAX_POS, 64)
    assert maxabs(to_np(cos), c) <= 2.0 ** -24 and maxabs(to_np(sin), s) <= 2.0 ** -24 and cos.is_cuda
    rng = np.random.default_rng(3)
    for dtype in ("f32", "bf16"):
        x, tx = _rand(rng, (2, 5, 3, 64), dtype)
        buf = torch.zeros(tx.numel() + 8, dtype=tx.dtype, device="cuda")
        off = 4 // tx.element_size()
        view = buf[off:off + tx.numel()].view(tx.shape)
        view.copy_(tx)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        for il in (False, True):
            assert _same(dev.apply_rotary(view, cos, sin, interleaved=il), dev.apply_rotary(tx, cos, sin, interleaved=il)), (dtype, il)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_apply_rotary_backward_is_the_inverse_rotation_of_the_gradient(dtype):
    """The gradient of a random cotangent is apply_rotary(g, inverse=True), bit for bit, and agrees with torch autograd of a
    pure-torch fp64 rotation within the derived bound (on g in the place of x)."""
    torch, dev = _torch(), _dev()
    rng = np.random.default_rng(23)
    B, N, H, d, rot = 2, 5, 3, 64, 32
    c, s, tc, ts = _tables(rot)
    offs = torch.tensor([0, 37], dtype=torch.int32, device="cuda")
    for il in (False, True):
        x, tx = _rand(rng, (B, N, H, d), dtype)
        g, tg = _rand(rng, (B, N, H, d), dtype)
        tx.requires_grad_(True)
        y = dev.apply_rotary(tx, tc, ts, offs, il)
        y.backward(tg)
        assert tx.grad.dtype == tx.dtype and _same(tx.grad, dev.apply_rotary(tg, tc, ts, offs, il, inverse=True))
        # the same function in torch, fp64, under torch's own autograd
        x64 = torch.from_numpy(x).double().requires_grad_(True)
        pos = (torch.tensor([0, 37])[:, None] + torch.arange(N)[None, :]).clamp(0, MAX_POS - 1)
        c64, s64 = (torch.from_numpy(t).double()[pos][:, :, None, :] for t in (c, s))   # (B, N, 1, rot / 2)
        x1, x2 = (x64[..., 0:rot:2], x64[..., 1:rot:2]) if il else (x64[..., :rot // 2], x64[..., rot // 2:rot])
        y1, y2 = x1 * c64 - x2 * s64, x2 * c64 + x1 * s64
        head = torch.stack([y1, y2], dim=-1).flatten(-2) if il else torch.cat([y1, y2], dim=-1)
        y64 = torch.cat([head, x64[..., rot:]], dim=-1)
        assert maxabs(y64.detach().numpy(), rope_reference(x, c, s, pos.numpy()[:, :, None], il)) < 1e-15
        y64.backward(torch.from_numpy(g).double())
        exact = x64.grad.numpy()
        bound = U[dtype] * np.abs(exact) + rope_bound(g, c, U[dtype], il)
        err = np.abs(to_np(tx.grad).astype(np.float64) - exact)
        assert np.all(err <= bound), (il, float(err.max()))
        assert np.array_equal(to_np(tx.grad)[..., rot:], g[..., rot:])


# ---- law 1: rope_append = apply_rotary on q and on k_new, then the family's plain append ----

def _rope_append(q, q_rot, kn, vn, kc, vc, lens, tc, ts, il, layout="bnhd", table=None, scales=(None, None), cu=None):
    """fa_mi355x_rope_append[_ragged] through the C ABI, as device_ops calls it."""
    torch, dev = _torch(), _dev()
    from flash_attention_minitorch_amd import _lib
    p = dev._ptr
    bnhd = layout == "bnhd"
    fp8 = kc.dtype == torch.float8_e4m3fn
    d = kc.shape[3]
    if table is not None:
        geo = (0, kc.shape[0], kc.shape[1] if bnhd else kc.shape[2], table.shape[1])
        Hkv = kc.shape[2] if bnhd else kc.shape[1]
    else:
        geo = (kc.shape[1] if bnhd else kc.shape[2], 0, 0, 0)
        Hkv = kc.shape[2] if bnhd else kc.shape[1]
    rot, max_pos = 2 * tc.shape[1], tc.shape[0]
    some = q if q is not None else kn   # (without a q: H is not used, Hkv stands in)
    dtype = _lib.FA_DTYPE_BF16 if fp8 else dev._dtype_code(some)
    d_new = kn.shape[-1] if kn is not None else d
    lay = dev._DECODE_LAYOUTS[layout]
    if cu is not None:
        T, H = some.shape[0], some.shape[1]
        rc = _lib.decode().fa_mi355x_rope_append_ragged(p(q), p(q_rot), p(kn), p(vn), p(kc), p(vc), p(tc), p(ts), p(cu), p(lens), p(table),
                                                        cu.shape[0] - 1, H, Hkv, T, *geo, d_new, d, rot, max_pos, lay, int(il), dtype,
                                                        dev._stream_ptr())
    else:
        B, Nq, H = (some.shape[0], some.shape[1], some.shape[2]) if bnhd else (some.shape[0], some.shape[2], some.shape[1])
        rc = _lib.decode().fa_mi355x_rope_append(p(q), p(q_rot), p(kn), p(vn), p(kc), p(vc), p(scales[0]), p(scales[1]), p(tc), p(ts), p(lens),
                                                 p(table), B, H, Hkv, Nq, *geo, d_new, d, rot, max_pos, lay, int(il), int(fp8), dtype,
                                                 dev._stream_ptr())
    _lib.decode_check(rc)


def _sentinel(shape, tdt, seed):
    """A cache full of a pattern no append writes: any stray write shows in a comparison of the whole tensor."""
    torch = _torch()
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(1, 120, shape, generator=g, dtype=torch.uint8)
    if tdt == torch.float8_e4m3fn:
        return t.cuda().view(tdt)
    return (t.float() + 0.5).to("cuda", tdt)


SLAB = dict(B=2, H=4, Hkv=2, Ncap=256)


@pytest.mark.parametrize("interleaved", [False, True], ids=["neox", "gptj"])
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_law_1_slab_rope_append_is_apply_rotary_then_the_plain_append(dtype, layout, interleaved):
    """Nq in {1, 3, 128}; lengths below Nq, interior, = Ncap and > Ncap; d_new = d, d_new < d and d_new = 34 (no multiple of a
    vector: the element build).  q_rot and both caches, every bit."""
    torch, dev = _torch(), _dev()
    rng = np.random.default_rng(31)
    B, H, Hkv, Ncap = (SLAB[n] for n in ("B", "H", "Hkv", "Ncap"))
    d, tdt, bnhd = 64, _tdt(dtype), layout == "bnhd"
    for Nq in (1, 3, 128):
        for lens in ([Nq - 1, 150], [Ncap, Ncap + 44]):
            for d_new, rot in ((64, 64), (48, 32), (34, 34), (34, 6)):
                c, s, tc, ts = _tables(rot)
                sh = lambda h, n, w: (B, n, h, w) if bnhd else (B, h, n, w)
                (_, q), (_, kn), (_, vn) = (_rand(rng, sh(h, Nq, w), dtype) for h, w in ((H, d), (Hkv, d_new), (Hkv, d_new)))
                tl = torch.tensor(lens, dtype=torch.int32, device="cuda")
                k0, v0 = _sentinel(sh(Hkv, Ncap, d), tdt, 1), _sentinel(sh(Hkv, Ncap, d), tdt, 2)
                # composed: the two rotations at offsets clamp(len) - Nq, then the plain append
                offs = tl.clamp(0, Ncap) - Nq
                qa, ka = (dev.apply_rotary(t, tc, ts, offs, interleaved, layout=layout) for t in (q, kn))
                k1, v1 = k0.clone(), v0.clone()
                dev.extend_append(ka, vn, k1, v1, tl, layout)
                # fused
                k2, v2, qr = k0.clone(), v0.clone(), torch.full_like(q, 9.0)
                _rope_append(q, qr, kn, vn, k2, v2, tl, tc, ts, interleaved, layout)
                what = (Nq, lens, d_new, rot)
                assert _same(qr, qa), what
                assert _same(k2, k1) and _same(v2, v1), what
                assert not _same(k2, k0) or min(lens) == 0, what
    # q alone, in place (q_rot = q), and the append alone: each is its half of the fused call
    _rope_append(q, q, None, None, k0, v0, tl, tc, ts, interleaved, layout)
    assert _same(q, qa)
    k3, v3 = k0.clone(), v0.clone()
    _rope_append(None, None, kn, vn, k3, v3, tl, tc, ts, interleaved, layout)
    assert _same(k3, k1) and _same(v3, v1)
    # ... and the public append with the tables is that call
    k4, v4 = k0.clone(), v0.clone()
    dev.extend_append(kn, vn, k4, v4, tl, layout, rotary_cos=tc, rotary_sin=ts, rotary_interleaved=interleaved)
    assert _same(k4, k1) and _same(v4, v1)


@pytest.mark.parametrize("interleaved", [False, True], ids=["neox", "gptj"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_law_1_paged_rope_append_across_a_page_boundary(dtype, interleaved):
    """page_size 128, a permuted table; lengths 130 with Nq = 5: the tokens' rows 125 .. 129 cross from the first page to the second."""
    torch, dev = _torch(), _dev()
    rng = np.random.default_rng(37)
    B, H, Hkv, d, Nq, ps = 2, 4, 2, 64, 5, 128
    tdt = _tdt(dtype)
    table = torch.tensor([[3, 1], [0, 4]], dtype=torch.int32, device="cuda")
    tl = torch.tensor([130, 256], dtype=torch.int32, device="cuda")
    for layout in ("bnhd", "bhnd"):
        bnhd = layout == "bnhd"
        for d_new, rot in ((64, 64), (34, 32)):
            c, s, tc, ts = _tables(rot)
            sh = lambda h, w: (B, Nq, h, w) if bnhd else (B, h, Nq, w)
            (_, q), (_, kn), (_, vn) = (_rand(rng, sh(h, w), dtype) for h, w in ((H, d), (Hkv, d_new), (Hkv, d_new)))
            pool = (5, ps, Hkv, d) if bnhd else (5, Hkv, ps, d)
            k0, v0 = _sentinel(pool, tdt, 3), _sentinel(pool, tdt, 4)
            offs = tl.clamp(0, 2 * ps) - Nq
            qa, ka = (dev.apply_rotary(t, tc, ts, offs, interleaved, layout=layout) for t in (q, kn))
            k1, v1 = k0.clone(), v0.clone()
            dev.extend_append(ka, vn, k1, v1, tl, layout, block_table=table)
            k2, v2, qr = k0.clone(), v0.clone(), torch.full_like(q, 9.0)
            _rope_append(q, qr, kn, vn, k2, v2, tl, tc, ts, interleaved, layout, table=table)
            assert _same(qr, qa) and _same(k2, k1) and _same(v2, v1), (layout, d_new)
            assert _same(k2[2], k0[2]) and not _same(k2[3], k0[3]) and not _same(k2[1], k0[1])   # (page 2 is nobody's; 3 and 1: rows 125 .. 129)


@pytest.mark.parametrize("paged", [False, True], ids=["slab", "paged"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_law_1_ragged_rope_append(dtype, paged):
    """T = 40, B = 4, cu = [0, 1, 1, 33, 38]: an empty sequence and an unused tail.  The composed side rotates the packed rows as T
    sequences of one token with per-token offsets, then appends with the plain ragged append; the rows of q_rot that no sequence
    owns keep what they held."""
    torch, dev = _torch(), _dev()
    rng = np.random.default_rng(41)
    T, B, H, Hkv, d, Ncap = 40, 4, 4, 2, 64, 256
    cu_h, lens_h = [0, 1, 1, 33, 38], [10, 5, 200, 3]   # (the last sequence: 5 tokens, length 3: two of them fall below row 0)
    tdt = _tdt(dtype)
    cu = torch.tensor(cu_h, dtype=torch.int32, device="cuda")
    tl = torch.tensor(lens_h, dtype=torch.int32, device="cuda")
    offs_h = np.zeros(T, dtype=np.int32)
    for b in range(B):
        for i, t in enumerate(range(cu_h[b], cu_h[b + 1])):
            offs_h[t] = lens_h[b] - (cu_h[b + 1] - cu_h[b]) + i
    offs = torch.from_numpy(offs_h).cuda()
    table = torch.tensor([[3, 1], [0, 4], [7, 2], [6, 5]], dtype=torch.int32, device="cuda") if paged else None
    kw = dict(block_table=table) if paged else {}
    for il in (False, True):
        for d_new, rot in ((64, 64), (34, 32)):
            c, s, tc, ts = _tables(rot)
            (_, q), (_, kn), (_, vn) = (_rand(rng, (T, h, w), dtype) for h, w in ((H, d), (Hkv, d_new), (Hkv, d_new)))
            shape = (8, 128, Hkv, d) if paged else (B, Ncap, Hkv, d)
            k0, v0 = _sentinel(shape, tdt, 5), _sentinel(shape, tdt, 6)
            qa, ka = (dev.apply_rotary(t[:, None], tc, ts, offs, il)[:, 0] for t in (q, kn))
            k1, v1 = k0.clone(), v0.clone()
            dev.ragged_append(ka.contiguous(), vn, k1, v1, cu, tl, **kw)
            k2, v2, qr = k0.clone(), v0.clone(), torch.full_like(q, 9.0)
            _rope_append(q, qr, kn, vn, k2, v2, tl, tc, ts, il, table=table, cu=cu)
            assert _same(qr[:38], qa[:38]) and bool((qr[38:] == 9.0).all()), (il, d_new)
            assert _same(k2, k1) and _same(v2, v1) and not _same(k2, k0), (il, d_new)
            k3, v3 = k0.clone(), v0.clone()
            dev.ragged_append(kn, vn, k3, v3, cu, tl, rotary_cos=tc, rotary_sin=ts, rotary_interleaved=il, **kw)
            assert _same(k3, k1) and _same(v3, v1), (il, d_new)


@pytest.mark.parametrize("paged", [False, True], ids=["slab", "paged"])
def test_law_1_fp8_rope_append_quantises_the_rotated_k_as_append_fp8_does(paged):
    """Scales [0.5, 2] and a pair that is no power of two; the composed side is apply_rotary (rounded to bf16) followed by
    fa_mi355x_append_fp8.  Every byte of both caches."""
    torch, dev = _torch(), _dev()
    rng = np.random.default_rng(43)
    B, H, Hkv, d, Ncap = 2, 4, 2, 64, 256
    f8 = torch.float8_e4m3fn
    table = torch.tensor([[3, 1], [0, 4]], dtype=torch.int32, device="cuda") if paged else None
    kw = dict(block_table=table) if paged else {}
    for Nq, lens in ((1, [0, 77]), (5, [130, 256]), (128, [127, 300])):
        tl = torch.tensor(lens, dtype=torch.int32, device="cuda")
        for scales in ([0.5, 2.0], [0.3, 1.7]):
            ks = torch.tensor(scales, dtype=torch.float32, device="cuda")
            vs = torch.tensor(scales[::-1], dtype=torch.float32, device="cuda")
            for il, (d_new, rot) in ((False, (64, 64)), (True, (64, 32)), (False, (34, 34)), (True, (48, 6))):
                c, s, tc, ts = _tables(rot)
                (_, q), (_, kn), (_, vn) = (_rand(rng, (B, Nq, h, w), "bf16", 4.0) for h, w in ((H, d), (Hkv, d_new), (Hkv, d_new)))
                shape = (5, 128, Hkv, d) if paged else (B, Ncap, Hkv, d)
                k0, v0 = _sentinel(shape, f8, 7), _sentinel(shape, f8, 8)
                offs = tl.clamp(0, Ncap) - Nq
                qa, ka = (dev.apply_rotary(t, tc, ts, offs, il) for t in (q, kn))
                k1, v1 = k0.clone(), v0.clone()
                dev.extend_append(ka, vn, k1, v1, tl, k_scale=ks, v_scale=vs, **kw)
                k2, v2, qr = k0.clone(), v0.clone(), torch.full_like(q, 9.0)
                _rope_append(q, qr, kn, vn, k2, v2, tl, tc, ts, il, table=table, scales=(ks, vs))
                what = (Nq, scales, il, d_new, rot)
                assert _same(qr, qa) and _same(k2, k1) and _same(v2, v1), what
                assert not _same(k2, k0), what
    k3, v3 = k0.clone(), v0.clone()   # null scales: all ones
    _rope_append(q, qr, kn, vn, k3, v3, tl, tc, ts, il, table=table)
    k1, v1 = k0.clone(), v0.clone()
    dev.extend_append(ka, vn, k1, v1, tl, **kw)
    assert _same(k3, k1) and _same(v3, v1)


# ---- law 2: a roped attention call = the same call without the tables on the rotated q and k_new ----

def _law_2(call, q, kn, vn, caches, tc, ts, il, qa, ka):
    """call(q, kc, vc, k_new=, v_new=) -> (out, lse) on the rotated qa, ka without the tables, and on q, kn with them (q_rot the
    caller's): the caches end with the same bits.  Returns both results and q_rot."""
    torch = _torch()
    k0, v0 = caches
    k1, v1, k2, v2 = k0.clone(), v0.clone(), k0.clone(), v0.clone()
    o1, l1 = call(qa, k1, v1, k_new=ka, v_new=vn)
    qr = torch.full_like(q, 9.0)
    o2, l2 = call(q, k2, v2, k_new=kn, v_new=vn, rotary_cos=tc, rotary_sin=ts, rotary_interleaved=il, q_rot=qr)
    torch.cuda.synchronize()
    assert _same(k2, k1) and _same(v2, v1) and not _same(k2, k0)
    return (o1, l1), (o2, l2), qr


@pytest.mark.parametrize("family", ["decode", "extend"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_law_2_roped_decode_and_extend_are_the_calls_on_rotated_inputs(dtype, family):
    """Slab, at the shapes of law 1 (B = 2, H = 4, Hkv = 2, Ncap = 256, Nq in {1, 3, 128}, a length below Nq), both pairings; then
    once with window = 64, sink = 4 on a paged cache, and q_rot left to the call."""
    torch, dev = _torch(), _dev()
    rng = np.random.default_rng(47)
    B, H, Hkv, Ncap, d = 2, 4, 2, 256, 64
    tdt = _tdt(dtype)
    fn = dev.flash_attn_decode if family == "decode" else dev.flash_attn_extend
    for Nq, lens, il, (d_new, rot) in ((1, [0, 150], False, (64, 64)), (3, [2, 256], True, (64, 32)), (128, [127, 300], False, (48, 32))):
        c, s, tc, ts = _tables(rot)
        (_, q), (_, kn), (_, vn) = (_rand(rng, (B, Nq, h, w), dtype) for h, w in ((H, d), (Hkv, d_new), (Hkv, d_new)))
        (_, k0), (_, v0) = (_rand(rng, (B, Ncap, Hkv, d), dtype) for _ in range(2))
        tl = torch.tensor(lens, dtype=torch.int32, device="cuda")
        offs = tl.clamp(0, Ncap) - Nq
        qa, ka = dev.apply_rotary(q, tc, ts, offs, il), dev.apply_rotary(kn, tc, ts, offs, il)
        (o1, l1), (o2, l2), qr = _law_2(lambda q, kc, vc, **kw: fn(q, kc, vc, tl, **kw), q, kn, vn, (k0, v0), tc, ts, il, qa, ka)
        assert _same(o2, o1) and _same(l2, l1) and _same(qr, qa), (Nq, lens)
        assert bool(torch.isfinite(o2).all())
    # window + sink on a paged cache (page_size 128, a permuted table), the tokens crossing a page boundary
    table = torch.tensor([[3, 1], [0, 4]], dtype=torch.int32, device="cuda")
    tl = torch.tensor([130, 256], dtype=torch.int32, device="cuda")
    Nq = 5
    c, s, tc, ts = _tables(64)
    (_, q), (_, kn), (_, vn) = (_rand(rng, (B, Nq, h, d), dtype) for h in (H, Hkv, Hkv))
    (_, k0), (_, v0) = (_rand(rng, (5, 128, Hkv, d), dtype) for _ in range(2))
    offs = tl.clamp(0, 256) - Nq
    qa, ka = dev.apply_rotary(q, tc, ts, offs), dev.apply_rotary(kn, tc, ts, offs)
    k1, v1, k2, v2 = k0.clone(), v0.clone(), k0.clone(), v0.clone()
    kw = dict(block_table=table, window=64, sink=4)
    o1, l1 = fn(qa, k1, v1, tl, k_new=ka, v_new=vn, **kw)
    o2, l2 = fn(q, k2, v2, tl, k_new=kn, v_new=vn, rotary_cos=tc, rotary_sin=ts, **kw)   # (q_rot allocated by the call)
    assert _same(o2, o1) and _same(l2, l1) and _same(k2, k1) and _same(v2, v1)
    o3, l3 = fn(q, k0.clone(), v0.clone(), tl, k_new=kn, v_new=vn, **kw)
    assert not _same(o3, o2)   # (the rotation matters)


@pytest.mark.parametrize("paged", [False, True], ids=["slab", "paged"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_law_2_roped_ragged_call_is_the_call_on_rotated_inputs(dtype, paged):
    torch, dev = _torch(), _dev()
    rng = np.random.default_rng(53)
    T, B, H, Hkv, d, Ncap = 40, 4, 4, 2, 64, 256
    cu_h, lens_h = [0, 1, 1, 33, 38], [10, 5, 200, 3]
    cu = torch.tensor(cu_h, dtype=torch.int32, device="cuda")
    tl = torch.tensor(lens_h, dtype=torch.int32, device="cuda")
    offs_h = np.zeros(T, dtype=np.int32)
    for b in range(B):
        for i, t in enumerate(range(cu_h[b], cu_h[b + 1])):
            offs_h[t] = lens_h[b] - (cu_h[b + 1] - cu_h[b]) + i
    offs = torch.from_numpy(offs_h).cuda()
    table = torch.tensor([[3, 1], [0, 4], [7, 2], [6, 5]], dtype=torch.int32, device="cuda") if paged else None
    kw = dict(block_table=table) if paged else {}
    for il, (d_new, rot) in ((False, (64, 64)), (True, (48, 32))):
        c, s, tc, ts = _tables(rot)
        (_, q), (_, kn), (_, vn) = (_rand(rng, (T, h, w), dtype) for h, w in ((H, d), (Hkv, d_new), (Hkv, d_new)))
        (_, k0), (_, v0) = (_rand(rng, (8, 128, Hkv, d) if paged else (B, Ncap, Hkv, d), dtype) for _ in range(2))
        qa, ka = (dev.apply_rotary(t[:, None], tc, ts, offs, il)[:, 0].contiguous() for t in (q, kn))
        k1, v1, k2, v2 = k0.clone(), v0.clone(), k0.clone(), v0.clone()
        outs = [torch.zeros((T, H, d), dtype=torch.float32, device="cuda") for _ in range(2)]   # (the unused tail keeps what it held)
        lses = [torch.zeros((H, T), dtype=torch.float32, device="cuda") for _ in range(2)]
        dev.flash_attn_ragged(qa, k1, v1, cu, tl, out=outs[0], lse=lses[0], k_new=ka, v_new=vn, **kw)
        dev.flash_attn_ragged(q, k2, v2, cu, tl, out=outs[1], lse=lses[1], k_new=kn, v_new=vn, rotary_cos=tc, rotary_sin=ts,
                              rotary_interleaved=il, **kw)
        assert _same(outs[1], outs[0]) and _same(lses[1][:, :38], lses[0][:, :38]) and _same(k2, k1) and _same(v2, v1), (il, d_new)
        assert bool((outs[1][:38].abs().sum(dim=(1, 2)) > 0).sum() >= 36)   # (two tokens of the last sequence sit below row 0: empty rows)


@pytest.mark.parametrize("family", ["decode", "extend"])
def test_law_2_on_an_fp8_cache_and_at_a_multi_split_shape(family):
    torch, dev = _torch(), _dev()
    from flash_attention_minitorch_amd import _lib
    rng = np.random.default_rng(59)
    fn = dev.flash_attn_decode if family == "decode" else dev.flash_attn_extend
    f8 = torch.float8_e4m3fn
    # fp8: B = 2, H = 4, Hkv = 2, Ncap = 256, the cache holding e4m3 codes of a random bf16 tensor
    B, H, Hkv, Ncap, d, Nq = 2, 4, 2, 256, 64, 3
    c, s, tc, ts = _tables(64)
    (_, q), (_, kn), (_, vn) = (_rand(rng, (B, Nq, h, d), "bf16") for h in (H, Hkv, Hkv))
    k0, v0 = (_rand(rng, (B, Ncap, Hkv, d), "bf16")[1].to(f8) for _ in range(2))
    tl = torch.tensor([2, 150], dtype=torch.int32, device="cuda")
    ks, vs = torch.tensor([0.5, 0.3], device="cuda"), torch.tensor([2.0, 1.7], device="cuda")
    offs = tl.clamp(0, Ncap) - Nq
    qa, ka = dev.apply_rotary(q, tc, ts, offs), dev.apply_rotary(kn, tc, ts, offs)
    k1, v1, k2, v2 = k0.clone(), v0.clone(), k0.clone(), v0.clone()
    o1, l1 = fn(qa, k1, v1, tl, k_new=ka, v_new=vn, k_scale=ks, v_scale=vs)
    o2, l2 = fn(q, k2, v2, tl, k_new=kn, v_new=vn, k_scale=ks, v_scale=vs, rotary_cos=tc, rotary_sin=ts)
    assert _same(o2, o1) and _same(l2, l1) and _same(k2, k1) and _same(v2, v1) and not _same(k2, k0)
    # many splits: B = 1, H = 2, Hkv = 1, d = 64, Ncap = 4096 (the workspace, the split and the combine launch behind rope_append)
    B, H, Hkv, Ncap, Nq = 1, 2, 1, 4096, 2
    splits = _lib.decode().fa_mi355x_decode_splits_gqa if family == "decode" else _lib.decode().fa_mi355x_extend_splits
    assert splits(B, H, Hkv, Nq, Ncap, d, _lib.FA_DTYPE_BF16) > 1
    c, s, tc, ts = _tables(64, Ncap)
    (_, q), (_, kn), (_, vn) = (_rand(rng, (B, Nq, h, d), "bf16") for h in (H, Hkv, Hkv))
    (_, k0), (_, v0) = (_rand(rng, (B, Ncap, Hkv, d), "bf16") for _ in range(2))
    tl = torch.tensor([4000], dtype=torch.int32, device="cuda")
    offs = tl.clamp(0, Ncap) - Nq
    qa, ka = dev.apply_rotary(q, tc, ts, offs), dev.apply_rotary(kn, tc, ts, offs)
    k1, v1, k2, v2 = k0.clone(), v0.clone(), k0.clone(), v0.clone()
    o1, l1 = fn(qa, k1, v1, tl, k_new=ka, v_new=vn)
    o2, l2 = fn(q, k2, v2, tl, k_new=kn, v_new=vn, rotary_cos=tc, rotary_sin=ts)
    assert _same(o2, o1) and _same(l2, l1) and _same(k2, k1) and _same(v2, v1)
    assert not _same(k2[:, 3998:4000], k0[:, 3998:4000]) and _same(k2[:, :3998], k0[:, :3998])


# ---- end to end against the fp64 oracle ----

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_roped_decode_matches_the_fp64_reference_on_reference_rotated_inputs(dtype):
    """A cache of reference-rotated keys (rounded to the dtype), then one roped fused decode call of Nq = 3 new tokens: out and lse
    against decode_reference on the reference-rotated q and keys, at the tolerance tests/test_gpu_decode.py uses for the unroped
    call."""
    torch, dev = _torch(), _dev()
    rng = np.random.default_rng(61)
    B, H, Hkv, Ncap, d, Nq, rot = 2, 4, 2, 520, 64, 3, 32
    G = H // Hkv
    lens = [257, 520]
    c, s = rope_tables(Ncap, rot)
    tc, ts = torch.from_numpy(c).cuda(), torch.from_numpy(s).cuda()
    q, tq = _rand(rng, (B, Nq, H, d), dtype)
    kn, tkn = _rand(rng, (B, Nq, Hkv, d), dtype)
    vn, tvn = _rand(rng, (B, Nq, Hkv, d), dtype)
    kraw = rand_u(rng, (B, Ncap, Hkv, d))
    v, tv = _rand(rng, (B, Ncap, Hkv, d), dtype)
    krot = rope_reference(kraw, c, s, np.arange(Ncap)[None, :, None]).astype(np.float32)
    if dtype == "bf16":
        krot = oracle.bf16_round(krot)
    tk = torch.from_numpy(krot).to("cuda", _tdt(dtype))
    tl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    out, lse = dev.flash_attn_decode(tq, tk, tv, tl, k_new=tkn, v_new=tvn, rotary_cos=tc, rotary_sin=ts)
    torch.cuda.synchronize()
    # the reference: the cache with the new tokens' reference-rotated k (and v) at rows len - Nq .. len - 1, the reference-rotated q
    kref, vref = krot.astype(np.float64), v.astype(np.float64)
    qref = np.empty((B, Nq, H, d))
    for b, n in enumerate(lens):
        pos = (n - Nq + np.arange(Nq))[:, None]
        kref[b, n - Nq:n] = rope_reference(kn[b], c, s, pos)
        vref[b, n - Nq:n] = vn[b]
        qref[b] = rope_reference(q[b], c, s, pos)
    o, l = to_np(out), to_np(lse)
    worst = 0.0
    for b in range(B):
        for h in range(H):
            ro, rl = decode_reference(qref[b:b + 1, :, h], kref[b:b + 1, :, h // G], vref[b:b + 1, :, h // G], lens[b:b + 1], True, 1.0 / math.sqrt(d))
            worst = max(worst, maxabs(o[b, :, h], ro[0]), maxabs(l[b, h], rl[0]))
    print(f"roped decode {dtype}: max |err| {worst:.3e} (< {TOL[dtype]:.0e})")
    assert worst < TOL[dtype], worst
