"""CPU-side checks of the rotary embeddings (include/flash_attn_mi355x_decode_rope.h: a tensor rotated by position, and the fused
rotate-and-append in front of the attend-only calls): this file's fp64 reference ``rope_reference`` (used by tests/test_gpu_rope.py)
against an independent formulation, complex multiplication; the three symbols declared, exported and bound; the rope builds in the
code object, without scratch; every bad argument answered before any HIP call (fake non-null pointers, as in tests/test_fp8_cpu.py:
a launch would fail with another code); the Python checks that need no GPU and the model layer's calls under the recorder."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_abi_cpu import _device_kernels
from test_decode_cpu import _declared, built  # noqa: F401  (built: the module-scoped build fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "flash_attn_mi355x_decode_rope.h")
ROPE = ["fa_mi355x_rope", "fa_mi355x_rope_append", "fa_mi355x_rope_append_ragged"]


# ---- the fp64 reference (used by tests/test_gpu_rope.py) ----

def rope_tables(max_pos, rot, base=10000.0):
    """fp32 (cos, sin) [max_pos][rot / 2] of the angles p * base^(-2j / rot), computed in fp64 and rounded once."""
    inv = base ** (-np.arange(0, rot, 2, dtype=np.float64) / rot)
    ang = np.arange(max_pos, dtype=np.float64)[:, None] * inv[None, :]
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


def rope_pairs(x, rot, interleaved):
    """(x1, x2): the first and second members of the rot / 2 pairs of every row of x (..., d), as views' copies."""
    if interleaved:
        return x[..., 0:rot:2], x[..., 1:rot:2]
    return x[..., :rot // 2], x[..., rot // 2:rot]


def rope_reference(x, cos, sin, positions, interleaved=False, inverse=False):
    """The rotation in fp64: x (..., d); cos / sin (max_pos, rot / 2); ``positions`` an int array that broadcasts to x.shape[:-1],
    clamped to [0, max_pos - 1].  Pair j of a row at position p turns by (cos[p][j], sin[p][j]): y1 = x1 c - x2 s, y2 = x2 c + x1 s
    (inverse: -s); columns >= rot pass."""
    x = np.asarray(x, dtype=np.float64)
    rot = 2 * cos.shape[1]
    p = np.clip(np.broadcast_to(np.asarray(positions), x.shape[:-1]), 0, cos.shape[0] - 1)
    c, s = cos[p].astype(np.float64), sin[p].astype(np.float64)
    if inverse:
        s = -s
    x1, x2 = rope_pairs(x, rot, interleaved)
    y = x.copy()
    y1, y2 = x1 * c - x2 * s, x2 * c + x1 * s
    if interleaved:
        y[..., 0:rot:2], y[..., 1:rot:2] = y1, y2
    else:
        y[..., :rot // 2], y[..., rot // 2:rot] = y1, y2
    return y


def rope_bound(x, cos, u, interleaved=False):
    """The tolerance of the device rotation against rope_reference on the same inputs and tables: u * |exact| is added by the caller;
    this is the second term, 2^-22 * (|x1| + |x2|) per pair (three fp32 roundings with |c|, |s| <= 1), laid out like x; 0 past rot."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    rot = 2 * cos.shape[1]
    x1, x2 = rope_pairs(x, rot, interleaved)
    b = np.zeros_like(x)
    if interleaved:
        b[..., 0:rot:2] = b[..., 1:rot:2] = x1 + x2
    else:
        b[..., :rot // 2] = b[..., rot // 2:rot] = x1 + x2
    return 2.0 ** -22 * b


@pytest.mark.parametrize("interleaved", [False, True])
def test_rope_reference_is_a_complex_multiplication_and_its_inverse_undoes_it(interleaved):
    rng = np.random.default_rng(5)
    B, N, H, d, rot, max_pos = 2, 7, 3, 16, 10, 40
    cos, sin = rope_tables(max_pos, rot)
    assert cos.dtype == np.float32 and cos.shape == (max_pos, rot // 2) and np.all(cos[0] == 1) and np.all(sin[0] == 0)
    x = rng.standard_normal((B, N, H, d))
    pos = (np.array([-1, 35])[:, None] + np.arange(N))[:, :, None]   # (B, N, 1): -1 .. 5 and 35 .. 41, into both clamps (0 and 39)
    y = rope_reference(x, cos, sin, pos, interleaved)
    # independently: (x1 + i x2) * (c + i s) in complex128, members gathered by index arithmetic
    p = np.maximum(np.minimum(pos, max_pos - 1), 0)[..., 0]
    for j in range(rot // 2):
        i1, i2 = (2 * j, 2 * j + 1) if interleaved else (j, j + rot // 2)
        e = cos[p, j].astype(np.complex128) + 1j * sin[p, j].astype(np.complex128)   # (B, N)
        z = (x[..., i1] + 1j * x[..., i2]) * e[:, :, None]
        assert np.allclose(y[..., i1], z.real, rtol=0, atol=1e-15) and np.allclose(y[..., i2], z.imag, rtol=0, atol=1e-15)
        zi = (x[..., i1] + 1j * x[..., i2]) * np.conj(e)[:, :, None]
        yi = rope_reference(x, cos, sin, pos, interleaved, inverse=True)
        assert np.allclose(yi[..., i1], zi.real, rtol=0, atol=1e-15) and np.allclose(yi[..., i2], zi.imag, rtol=0, atol=1e-15)
    assert np.array_equal(y[..., rot:], x[..., rot:]) and not np.allclose(y[:, 2:, :, :rot], x[:, 2:, :, :rot])
    assert np.array_equal(y[0, :2], x[0, :2])   # (positions -1, clamped, and 0: the identity)
    assert np.array_equal(y[1, -1], rope_reference(x[1, -1], cos, sin, 39, interleaved))   # (41: the clamp holds it at 39)
    # the tables are fp32 roundings of a unit vector: c^2 + s^2 = 1 to 2^-23, so inverse . forward is the identity to that
    back = rope_reference(y, cos, sin, pos, interleaved, inverse=True)
    scale = (cos[p].astype(np.float64) ** 2 + sin[p].astype(np.float64) ** 2)   # (B, N, rot / 2): what the round trip multiplies by
    x1, x2 = rope_pairs(x, rot, interleaved)
    b1, b2 = rope_pairs(back, rot, interleaved)
    assert np.allclose(b1, x1 * scale[:, :, None, :], rtol=0, atol=1e-12) and np.allclose(b2, x2 * scale[:, :, None, :], rtol=0, atol=1e-12)
    # and with exact (fp64) unit vectors for tables it is the identity to 1e-12
    ang = rng.uniform(0, 6.28, (max_pos, rot // 2))
    c64, s64 = np.cos(ang), np.sin(ang)
    again = rope_reference(rope_reference(x, c64, s64, pos, interleaved), c64, s64, pos, interleaved, inverse=True)
    assert np.allclose(again, x, rtol=0, atol=1e-12)
    assert np.all(rope_bound(x, cos, 0, interleaved)[..., rot:] == 0) and np.all(rope_bound(x, cos, 0, interleaved)[..., :rot] > 0)


# ---- the C ABI ----

def test_the_three_rope_symbols_are_declared_exported_and_bound(built):
    from test_lib_cpu import _ctypes_kind, _prototypes
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert '#include "flash_attn_mi355x_decode_rope.h"' in open(os.path.join(ROOT, "include", "flash_attn_mi355x_decode.h")).read()
    assert sorted(set(re.findall(r"\b(fa_mi355x_\w+)\s*\(", text))) == sorted(ROPE) == sorted(built.ROPE_ABI)
    assert not [s for s in _declared() if "rope" in s]   # (the decode header's own text declares none of them)
    for other in ("", "_paged", "_ragged", "_window", "_fp8", "_sink"):
        assert not [s for s in _prototypes(f"flash_attn_mi355x_decode{other}.h") if "rope" in s], other
    protos = _prototypes("flash_attn_mi355x_decode_rope.h")
    lib = built.decode()
    for s in ROPE:
        assert hasattr(lib, s), s
        res, args = built.ROPE_ABI[s]
        ret, kinds = protos[s]
        assert [_ctypes_kind(a) for a in args] == kinds and _ctypes_kind(res) == ret, s
        assert getattr(lib, s).argtypes == args and getattr(lib, s).restype is res, s


def test_the_library_holds_the_rope_builds_without_scratch(built):
    kernels = _device_kernels(built.lib_path(built.DECODE_NAME))
    names = [k[0] for k in kernels]
    count = lambda pat: len([n for n in names if re.search(pat, n)])
    # (element type, elements per lane, interleaved): 16-byte and element builds of both types and pairings
    assert count(r"fa11rope_kernelIDF16bLi[18]ELb[01]EEEv") == 4 and count(r"fa11rope_kernelIfLi[14]ELb[01]EEEv") == 4
    # ... and PAGED, RAGGED, FP8: slab / paged x uniform / ragged for both types, and the four fp8 builds (bf16, uniform) per pairing
    assert count(r"fa18rope_append_kernelIDF16bLi[18]ELb[01]ELb[01]ELb[01]ELb0EEEv") == 16
    assert count(r"fa18rope_append_kernelIfLi[14]ELb[01]ELb[01]ELb[01]ELb0EEEv") == 16
    assert count(r"fa18rope_append_kernelIDF16bLi[18]ELb[01]ELb[01]ELb0ELb1EEEv") == 8
    assert count(r"rope_kernel") == 8 and count(r"rope_append_kernel") == 40
    rope = [k for k in kernels if "rope" in k[0]]
    assert len(rope) == 48
    for name, scratch, vgpr in rope:
        assert scratch == 0, (name, scratch)
        assert vgpr <= 512, (name, vgpr)


# one valid call of each entry point (fake non-null device pointers: a launch would fail, so a code other than the expected one
# shows a HIP call)
_ONE = 16
_GOOD = dict(x=_ONE, y=_ONE, offs=_ONE, q=_ONE, qr=_ONE, kn=_ONE, vn=_ONE, k=_ONE, v=_ONE, ks=_ONE, vs=_ONE, cos=_ONE, sin=_ONE, cu=_ONE,
             lens=_ONE, table=_ONE, B=2, N=100, H=4, Hkv=2, Nq=100, Ncap=2048, num_pages=40, page_size=128, max_pages=16, d_new=64, d=64,
             rot=64, max_pos=2048, layout=1, il=0, inv=0, fp8=0, dtype=1)
_VP = ctypes.c_void_p
BAD_ARG, BAD_D = 1, 2


def _call(lib, entry, **over):
    a = dict(_GOOD, **over)
    geo = [a[n] for n in ("Ncap", "num_pages", "page_size", "max_pages", "d_new", "d", "rot", "max_pos", "layout", "il")]
    if entry == "rope":
        rc = lib.fa_mi355x_rope(*[_VP(a[n]) for n in ("x", "y", "cos", "sin", "offs")], a["B"], a["N"], a["H"], a["d"], a["rot"], a["max_pos"],
                                a["layout"], a["il"], a["inv"], a["dtype"], None)
    elif entry == "append":
        ptrs = [_VP(a[n]) for n in ("q", "qr", "kn", "vn", "k", "v", "ks", "vs", "cos", "sin", "lens", "table")]
        rc = lib.fa_mi355x_rope_append(*ptrs, a["B"], a["H"], a["Hkv"], a["Nq"], *geo, a["fp8"], a["dtype"], None)
    else:
        ptrs = [_VP(a[n]) for n in ("q", "qr", "kn", "vn", "k", "v", "cos", "sin", "cu", "lens", "table")]
        rc = lib.fa_mi355x_rope_append_ragged(*ptrs, a["B"], a["H"], a["Hkv"], a["Nq"], *geo, a["dtype"], None)
    return rc, lib.fa_mi355x_decode_last_error().decode()


_SLAB, _NO_Q, _NO_KV = dict(table=0), dict(q=0, qr=0), dict(kn=0, vn=0)
_BAD_BOTH = [   # the two append forms, slab and paged, with and without q / the new tokens
    (dict(rot=63), BAD_ARG, "rot = 63"), (dict(rot=0, **_SLAB), BAD_ARG, "rot = 0"), (dict(rot=-2), BAD_ARG, "rot = -2"),
    (dict(rot=64, d_new=32), BAD_ARG, "rot = 64"), (dict(rot=34, d_new=32, **_SLAB, **_NO_Q), BAD_ARG, "rot = 34"),
    (dict(rot=66, **_NO_KV), BAD_ARG, "rot = 66"),   # (no k: d alone bounds it)
    (dict(cos=0), BAD_ARG, "cos"), (dict(sin=0, **_SLAB), BAD_ARG, "sin"), (dict(cos=0, **_NO_KV), BAD_ARG, "cos"),
    (dict(max_pos=2047, **_SLAB), BAD_ARG, "max_pos = 2047"), (dict(max_pos=2047), BAD_ARG, "max_pos = 2047"),   # (16 pages of 128 rows)
    (dict(max_pos=2048, max_pages=17), BAD_ARG, "max_pos = 2048"), (dict(max_pos=100, **_NO_KV, **_SLAB), BAD_ARG, "max_pos = 100"),
    (dict(q=0), BAD_ARG, "q and q_rot"), (dict(qr=0, **_SLAB), BAD_ARG, "q and q_rot"), (dict(qr=0, **_NO_KV), BAD_ARG, "q and q_rot"),
    (dict(kn=0), BAD_ARG, "k_new and v_new"), (dict(vn=0, **_SLAB), BAD_ARG, "k_new and v_new"), (dict(vn=0, **_NO_Q), BAD_ARG, "k_new and v_new"),
    (dict(**_NO_Q, **_NO_KV), BAD_ARG, "all null"),
    (dict(il=2), BAD_ARG, "interleaved"), (dict(il=-1, **_SLAB, **_NO_KV), BAD_ARG, "interleaved"),
    # inherited from the append
    (dict(d_new=65), BAD_ARG, "d_new = 65"), (dict(d_new=0, **_SLAB), BAD_ARG, "d_new = 0"), (dict(B=0), BAD_ARG, "positive"),
    (dict(k=0, **_SLAB), BAD_ARG, "null"), (dict(v=0, **_NO_Q), BAD_ARG, "null"), (dict(layout=2), BAD_ARG, "layout"),
    (dict(dtype=5, **_SLAB), BAD_ARG, "dtype"), (dict(d=48, d_new=48, rot=48), BAD_D, "32, 64, 128"),
    (dict(d=48, rot=48, **_NO_KV), BAD_D, "32, 64, 128"), (dict(Nq=0, **_NO_KV), BAD_ARG, "positive"), (dict(H=0), BAD_ARG, "H must"),
    # inherited from the paged form
    (dict(page_size=192), BAD_ARG, "page_size"), (dict(num_pages=0), BAD_ARG, "num_pages"), (dict(max_pages=0, **_NO_Q), BAD_ARG, "max_pages"),
    (dict(max_pages=1 << 24), BAD_ARG, "max_pages * page_size"), (dict(page_size=1 << 24, max_pos=1 << 30), BAD_ARG, "2 GiB"),
]
_BAD_APPEND = [
    (dict(fp8=1, dtype=0), BAD_ARG, "FA_DTYPE_F32"), (dict(fp8=1, dtype=0, **_SLAB, **_NO_Q), BAD_ARG, "FA_DTYPE_F32"),
    (dict(fp8=2), BAD_ARG, "cache_fp8"), (dict(fp8=1, rot=63), BAD_ARG, "rot = 63"), (dict(fp8=1, max_pos=5, ks=0, vs=0), BAD_ARG, "max_pos = 5"),
    (dict(fp8=1, Ncap=1 << 24, max_pos=1 << 24, **_SLAB), BAD_ARG, "2 GiB"),   # (one byte per element: 2^24 rows of 128 bytes)
    (dict(Nq=129, d_new=65), BAD_ARG, "d_new = 65"),   # (any Nq >= 1: 129 new tokens are not what is wrong with this call)
]
_BAD_RAGGED = [(dict(cu=0), BAD_ARG, "cu_seqlens_q"), (dict(cu=0, **_NO_KV, **_SLAB), BAD_ARG, "cu_seqlens_q")]
_BAD_ROPE = [
    (dict(rot=63), BAD_ARG, "rot = 63"), (dict(rot=0), BAD_ARG, "rot = 0"), (dict(rot=66), BAD_ARG, "rot = 66"), (dict(d=6, rot=8), BAD_ARG, "rot = 8"),
    (dict(cos=0), BAD_ARG, "cos"), (dict(sin=0), BAD_ARG, "sin"), (dict(x=0), BAD_ARG, "null"), (dict(y=0), BAD_ARG, "null"),
    (dict(il=2), BAD_ARG, "interleaved"), (dict(inv=2), BAD_ARG, "inverse"), (dict(inv=-1), BAD_ARG, "inverse"), (dict(max_pos=0), BAD_ARG, "max_pos"),
    (dict(B=0), BAD_ARG, "positive"), (dict(N=0), BAD_ARG, "positive"), (dict(d=0), BAD_ARG, "positive"), (dict(layout=3), BAD_ARG, "layout"),
    (dict(dtype=2), BAD_ARG, "dtype"), (dict(B=1 << 15, N=1 << 15, H=1 << 10, d=128, rot=2), BAD_ARG, "too many"),
]


_TWO_FAULTS_BOTH = [   # which error wins: the pairs, the page geometry, the append's checks, q's, the tables', max_pos against the cache
    (dict(qr=0, rot=63), BAD_ARG, "q and q_rot"), (dict(qr=0, kn=0), BAD_ARG, "q and q_rot"), (dict(kn=0, page_size=192), BAD_ARG, "k_new and v_new"),
    (dict(page_size=192, d_new=65), BAD_ARG, "page_size = 192"), (dict(d_new=65, rot=63), BAD_ARG, "d_new = 65"),
    (dict(H=0, cos=0), BAD_ARG, "H must"), (dict(cos=0, il=2), BAD_ARG, "cos"), (dict(il=2, rot=63), BAD_ARG, "interleaved"),
    (dict(rot=63, max_pos=5), BAD_ARG, "rot = 63"), (dict(dtype=5, layout=2, **_NO_KV), BAD_ARG, "unknown dtype"),
]
_TWO_FAULTS_APPEND = [   # cache_fp8, then the fp8 cache's dtype, in front of everything else
    (dict(fp8=2, dtype=0), BAD_ARG, "cache_fp8"), (dict(fp8=2, qr=0), BAD_ARG, "cache_fp8"), (dict(fp8=2, page_size=192), BAD_ARG, "cache_fp8"),
    (dict(fp8=1, dtype=0, qr=0), BAD_ARG, "FA_DTYPE_F32"), (dict(fp8=1, dtype=5, rot=63), BAD_ARG, "unknown dtype"),
    (dict(fp8=1, d_new=65, Ncap=1 << 24, max_pos=1 << 24, **_SLAB), BAD_ARG, "d_new = 65"),
]
_TWO_FAULTS_RAGGED = [
    (dict(cu=0, rot=63), BAD_ARG, "cu_seqlens_q"), (dict(cu=0, d=48, d_new=48, rot=48), BAD_ARG, "null cu_seqlens_q"),
    (dict(cu=0, k=0), BAD_ARG, "null pointer argument"), (dict(cu=0, d=48, rot=48, **_NO_KV), BAD_ARG, "null cu_seqlens_q"),
    (dict(cu=0, layout=2, **_NO_KV), BAD_ARG, "unknown layout"),
]


def _cases():
    out = [(e, o, c, m) for e in ("append", "ragged") for o, c, m in _BAD_BOTH + _TWO_FAULTS_BOTH]
    out += [("append", o, c, m) for o, c, m in _BAD_APPEND + _TWO_FAULTS_APPEND]
    out += [("ragged", o, c, m) for o, c, m in _BAD_RAGGED + _TWO_FAULTS_RAGGED]
    return out + [("rope", o, c, m) for o, c, m in _BAD_ROPE]


def _id(case):
    return case[0] + "-" + ",".join(f"{k}={v}" for k, v in case[1].items())


@pytest.mark.parametrize("entry,over,code,msg", _cases(), ids=[_id(c) for c in _cases()])
def test_rope_forms_reject_each_bad_argument_before_any_hip_call(built, entry, over, code, msg):
    rc, err = _call(built.decode(), entry, **over)
    assert rc == code and err and msg in err, (rc, err)


# ---- the Python layer ----

def test_rotary_table_is_the_fp64_table_rounded_once(built):
    import torch
    from flash_attention_minitorch_amd import device_ops

    for rot, base in ((64, 10000.0), (6, 500000.0)):
        cos, sin = device_ops.rotary_table(300, rot, base)
        c, s = rope_tables(300, rot, base)
        assert cos.dtype == torch.float32 and cos.shape == (300, rot // 2) and cos.is_contiguous() and sin.is_contiguous()
        # (torch and numpy may differ in the last place of an fp64 cosine: one fp32 ulp of a value <= 1 at the very most)
        assert np.abs(cos.numpy().astype(np.float64) - c).max() <= 2.0 ** -24 and np.abs(sin.numpy().astype(np.float64) - s).max() <= 2.0 ** -24
    for bad in (0, 7, -2):
        with pytest.raises(ValueError, match="even"):
            device_ops.rotary_table(16, bad)
    with pytest.raises(ValueError, match="max_pos"):
        device_ops.rotary_table(0, 8)


def test_rope_python_checks_that_need_no_gpu(built):
    import torch
    from flash_attention_minitorch_amd import device_ops

    q, kc = torch.zeros(2, 1, 4, 64), torch.zeros(2, 256, 2, 64)
    kn = torch.zeros(2, 1, 2, 64)
    qr, cu, knr = torch.zeros(40, 4, 64), torch.zeros(3, dtype=torch.int32), torch.zeros(40, 2, 64)
    cos, sin = device_ops.rotary_table(256, 64)
    attends = [lambda **kw: device_ops.flash_attn_decode(q, kc, kc.clone(), **kw), lambda **kw: device_ops.flash_attn_extend(q, kc, kc.clone(), **kw),
               lambda **kw: device_ops.flash_attn_ragged(qr, kc, kc.clone(), cu, **kw)]
    appends = [lambda **kw: device_ops.decode_append(kn, kn, kc, kc.clone(), **kw), lambda **kw: device_ops.extend_append(kn, kn, kc, kc.clone(), **kw),
               lambda **kw: device_ops.ragged_append(knr, knr, kc, kc.clone(), cu, **kw)]
    rotate = lambda **kw: device_ops.apply_rotary(torch.zeros(2, 5, 3, 64), **{"cos": cos, "sin": sin, **kw})
    for call in attends + appends:
        for kw in (dict(rotary_cos=cos), dict(rotary_sin=sin)):
            with pytest.raises(ValueError, match="go together"):
                call(**kw)
        with pytest.raises(TypeError, match="float32"):
            call(rotary_cos=cos.double(), rotary_sin=sin)
        with pytest.raises(TypeError, match="float32"):
            call(rotary_cos=cos, rotary_sin=sin.to(torch.bfloat16))
        with pytest.raises(TypeError, match="float32"):
            call(rotary_cos=cos, rotary_sin=[0.0])
        for bad in (sin[:100], sin[:, :16], sin.reshape(-1), sin.reshape(256, 32, 1)):
            with pytest.raises(ValueError, match="one shape"):
                call(rotary_cos=cos, rotary_sin=bad)
        with pytest.raises(ValueError, match="device"):
            call(rotary_cos=cos, rotary_sin=sin.to("meta"))
        with pytest.raises(ValueError, match="contiguous"):
            call(rotary_cos=torch.zeros(256, 64)[:, ::2], rotary_sin=sin)
        for ok in (dict(), dict(rotary_interleaved=True)):   # past the rotary checks: the next complaint is the missing GPU
            with pytest.raises(built.FlashAttnLibraryError, match="GPU"):
                call(rotary_cos=cos, rotary_sin=sin, **ok)
    for call in attends:
        with pytest.raises(ValueError, match="q_rot"):
            call(q_rot=torch.zeros(2, 1, 4, 64))   # (q_rot without the tables)
    for call in appends:
        with pytest.raises(ValueError, match="q_rot"):
            call(rotary_cos=cos, rotary_sin=sin, q_rot=torch.zeros(2, 1, 4, 64))   # (an append has no q)
    for kw in (dict(cos=None), dict(sin=None)):
        with pytest.raises(ValueError, match="go together|both tables"):
            rotate(**kw)
    with pytest.raises(TypeError, match="float32"):
        rotate(cos=cos.double())
    with pytest.raises(ValueError, match="one shape"):
        rotate(sin=sin[:5])
    with pytest.raises(ValueError, match="exceeds"):
        device_ops.apply_rotary(torch.zeros(2, 5, 3, 32), cos, sin)
    with pytest.raises(ValueError, match="seqlen_offsets"):
        rotate(seqlen_offsets=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="seqlen_offsets"):
        rotate(seqlen_offsets=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="out must"):
        rotate(out=torch.zeros(2, 5, 3, 64, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="layout"):
        rotate(layout="nbhd")
    with pytest.raises(TypeError, match="dtype"):
        device_ops.apply_rotary(torch.zeros(2, 5, 3, 64, dtype=torch.float16), cos, sin)
    with pytest.raises(built.FlashAttnLibraryError, match="GPU"):
        rotate(seqlen_offsets=torch.zeros(2, dtype=torch.int32), interleaved=True, inverse=True)
    # the ragged calls still refuse an fp8 cache, with the tables or without
    if hasattr(torch, "float8_e4m3fn"):
        k8 = torch.zeros(2, 256, 2, 64, dtype=torch.float8_e4m3fn)
        bf = torch.bfloat16
        for kw in (dict(), dict(rotary_cos=cos, rotary_sin=sin)):
            with pytest.raises(TypeError, match="ragged"):
                device_ops.flash_attn_ragged(qr.to(bf), k8, k8.clone(), cu, **kw)
            with pytest.raises(TypeError, match="ragged"):
                device_ops.ragged_append(knr.to(bf), knr.to(bf), k8, k8.clone(), cu, **kw)


def _names(rec):
    return [c.split("(")[0] for c in rec.calls if "workspace_bytes" not in c and "guard" not in c]


def test_calls_without_the_keywords_are_the_calls_they_were_and_roped_calls_attend_only(monkeypatch):
    """Under the recorder of tests/test_device_ops_cpu.py: a call without the rotary keywords makes exactly the library calls it made
    before (the same symbols and arguments as with the keywords passed as None, and no rope symbol); with them it is
    fa_mi355x_rope_append[_ragged] and then the ATTEND-ONLY entry point (null k_new / v_new where the entry point has them) on q_rot."""
    import torch
    from flash_attention_minitorch_amd import device_ops
    from test_device_ops_cpu import install_recorder

    rec = install_recorder(monkeypatch)
    bf = torch.bfloat16
    B, H, Hkv, Nq, Ncap, d = 2, 4, 2, 3, 256, 64
    q, kn = torch.zeros(B, Nq, H, d, dtype=bf), torch.zeros(B, Nq, Hkv, d, dtype=bf)
    kc, vc = torch.zeros(B, Ncap, Hkv, d, dtype=bf), torch.zeros(B, Ncap, Hkv, d, dtype=bf)
    pool, table = torch.zeros(5, 128, Hkv, d, dtype=bf), torch.zeros(B, 2, dtype=torch.int32)
    lens = torch.full((B,), 9, dtype=torch.int32)
    qp, knp, cu = torch.zeros(40, H, d, dtype=bf), torch.zeros(40, Hkv, d, dtype=bf), torch.tensor([0, 7, 40], dtype=torch.int32)
    cos, sin = device_ops.rotary_table(256, 32)
    named = dict(q=q, kn=kn, kc=kc, vc=vc, pool=pool, table=table, lens=lens, qp=qp, knp=knp, cu=cu, cos=cos, sin=sin)
    none = dict(rotary_cos=None, rotary_sin=None, rotary_interleaved=False, q_rot=None)
    rope = dict(rotary_cos=cos, rotary_sin=sin)
    cases = [   # (the call, the attend-only entry point a roped call ends in)
        (lambda **kw: device_ops.flash_attn_decode(q, kc, vc, lens, k_new=kn, v_new=kn, **kw), "fa_mi355x_fwd_decode_gqa"),
        (lambda **kw: device_ops.flash_attn_decode(q, kc, vc, lens, **kw), "fa_mi355x_fwd_decode_gqa"),
        (lambda **kw: device_ops.flash_attn_extend(q, kc, vc, lens, k_new=kn, v_new=kn, **kw), "fa_mi355x_fwd_extend"),
        (lambda **kw: device_ops.flash_attn_decode(q, pool, pool, lens, k_new=kn, v_new=kn, block_table=table, **kw), "fa_mi355x_fwd_decode_paged"),
        (lambda **kw: device_ops.flash_attn_extend(q, pool, pool, lens, k_new=kn, v_new=kn, block_table=table, **kw), "fa_mi355x_fwd_extend_paged"),
        (lambda **kw: device_ops.flash_attn_decode(q, kc, vc, lens, k_new=kn, v_new=kn, window=64, **kw), "fa_mi355x_fwd_decode_window"),
        (lambda **kw: device_ops.flash_attn_extend(q, pool, pool, lens, k_new=kn, v_new=kn, block_table=table, window=64, sink=4, **kw),
         "fa_mi355x_fwd_extend_sink"),
        (lambda **kw: device_ops.flash_attn_ragged(qp, kc, vc, cu, lens, k_new=knp, v_new=knp, **kw), "fa_mi355x_fwd_ragged"),
        (lambda **kw: device_ops.flash_attn_ragged(qp, pool, pool, cu, lens, k_new=knp, v_new=knp, block_table=table, **kw), "fa_mi355x_fwd_ragged_paged"),
        (lambda **kw: device_ops.flash_attn_ragged(qp, kc, vc, cu, lens, k_new=knp, v_new=knp, window=64, **kw), "fa_mi355x_fwd_ragged_window"),
    ]
    if hasattr(torch, "float8_e4m3fn"):
        k8 = torch.zeros(B, Ncap, Hkv, d, dtype=torch.float8_e4m3fn)
        named["k8"] = k8
        cases.append((lambda **kw: device_ops.flash_attn_decode(q, k8, k8, lens, k_new=kn, v_new=kn, **kw), "fa_mi355x_fwd_decode_fp8"))
    for call, attend in cases:
        rec.reset(named)
        call()
        plain = list(rec.calls)
        rec.reset(named)
        call(**none)
        assert rec.calls == plain and not [c for c in plain if "rope" in c], plain
        rec.reset(named)
        call(**rope)
        names = _names(rec)
        ragged = "ragged" in attend
        assert names == ["fa_mi355x_rope_append" + "_ragged" * ragged, attend], names
        first, last = (c for c in rec.calls if "workspace_bytes" not in c)
        a = first.split("(")[1].rstrip(")").split(",")
        src = "qp" if ragged else "q"
        assert a[0] == src and a[1] == "new0" and last.split("(")[1].startswith("new0,"), (first, last)   # q -> q_rot -> the attention
        assert (a[6:8] if ragged else a[8:10]) == ["cos", "sin"], first
        assert (a[-6:-2] if ragged else a[-7:-3]) == ["32", "256", "1", "0"], first   # rot, max_pos, bnhd, NeoX
        assert ragged or a[-3] == ("1" if "fp8" in attend else "0"), first   # cache_fp8
        if "window" in attend or "sink" in attend or "fp8" in attend:
            assert last.split("(")[1].split(",")[1:3] == ["null", "null"], last   # (one entry point per family: attend only)
    # q_rot may be the caller's tensor, q itself included; rotary_interleaved reaches the library
    rec.reset(named)
    device_ops.flash_attn_decode(q, kc, vc, lens, k_new=kn, v_new=kn, q_rot=q, rotary_interleaved=True, **rope)
    first, last = (c for c in rec.calls if "workspace_bytes" not in c)
    a = first.split("(")[1].rstrip(")").split(",")
    assert a[:6] == ["q", "q", "kn", "kn", "kc", "vc"] and a[6:12] == ["null", "null", "cos", "sin", "lens", "null"], first
    assert a[12:] == [str(v) for v in (B, H, Hkv, Nq, Ncap, 0, 0, 0, d, d, 32, 256, 1, 1, 0, 1)] + ["null"], first
    assert last.startswith("fa_mi355x_fwd_decode_gqa(q,kc,vc,"), last
    # the appends: fa_mi355x_rope_append without a q, whatever the cache
    for call, sym in ((lambda **kw: device_ops.decode_append(kn, kn, kc, vc, lens, **kw), "fa_mi355x_decode_append"),
                      (lambda **kw: device_ops.extend_append(kn, kn, pool, pool, lens, block_table=table, **kw), "fa_mi355x_extend_append_paged"),
                      (lambda **kw: device_ops.ragged_append(knp, knp, kc, vc, cu, lens, **kw), "fa_mi355x_ragged_append")):
        rec.reset(named)
        call()
        assert _names(rec) == [sym]
        rec.reset(named)
        call(**rope)
        assert _names(rec) == ["fa_mi355x_rope_append" + "_ragged" * ("ragged" in sym)] and rec.calls[0].split("(")[1].startswith("null,null,kn"), rec.calls
    # a rotary dimension above the head dim is refused here
    big = device_ops.rotary_table(256, 128)
    with pytest.raises(ValueError, match="exceeds"):
        device_ops.flash_attn_decode(q, kc, vc, lens, k_new=kn, v_new=kn, rotary_cos=big[0], rotary_sin=big[1])


def test_model_rope_calls_under_the_recorder(monkeypatch):
    """The stack functions on a cache with rope= under the recorder (CPU tensors, no library): every step, extend, ragged and
    chunked-prefill call is fa_mi355x_rope_append[_ragged] followed by the attend-only entry point that the cache's window / sink /
    fp8 / paging selects; the square prefill calls fa_mi355x_rope twice per layer; with rope=None no rope symbol appears."""
    import torch
    from flash_attention_minitorch_amd import modules_transformer as mt
    from test_device_ops_cpu import install_recorder

    rec = install_recorder(monkeypatch)
    B, P, H, Hkv, d, cap = 2, 130, 4, 2, 64, 512
    g = torch.Generator().manual_seed(0)
    x = torch.randn((B, 200, H * d), generator=g).to(torch.bfloat16)
    wq, wk = (torch.randn(s, generator=g).to(torch.bfloat16) for s in ((H * d, H * d), (H * d, Hkv * d)))
    layers = [(wq, wk, wk, wq)] * 2
    rope = mt.Rotary.table(cap, 32, device=x.device)
    assert (rope.rot, rope.max_pos, rope.interleaved) == (32, cap, False) and set(rope.keywords()) == {"rotary_cos", "rotary_sin", "rotary_interleaved"}
    named = {"cos": rope.cos, "sin": rope.sin}
    pair = lambda first, attend, n: [first, attend] * n

    cache = mt.KVCache(2, B, cap, H, d, torch.bfloat16, x.device, n_kv_head=Hkv, rope=rope)
    assert cache.rotary() == rope.keywords()
    rec.reset(named)
    mt.attention_stack_prefill(x[:, :P].contiguous(), layers, H, cache)
    assert _names(rec) == ["fa_mi355x_rope", "fa_mi355x_rope", "fa_mi355x_fwd_gqa"] * 2, _names(rec)
    for c in rec.calls:
        if c.startswith("fa_mi355x_rope("):   # q, then k: the prompt's rows at positions 0 .. P - 1 (no offsets), NeoX, forward, bf16
            a = c.split("(")[1].rstrip(")").split(",")
            assert a[2:5] == ["cos", "sin", "null"] and a[5:7] == [str(B), str(P)] and a[7] in (str(H), str(Hkv)), c
            assert a[8:] == [str(v) for v in (d, 32, cap, 1, 0, 0, 1)] + ["null"], c
    rec.reset(named)
    mt.attention_stack_step_fused(x[:, :1].contiguous(), layers, H, cache)
    mt.attention_stack_extend(x, layers, H, cache)
    assert _names(rec) == pair("fa_mi355x_rope_append", "fa_mi355x_fwd_decode_gqa", 2) + pair("fa_mi355x_rope_append", "fa_mi355x_fwd_extend", 2)
    for c in rec.calls:
        if c.startswith("fa_mi355x_rope_append("):
            a = c.split("(")[1].rstrip(")").split(",")
            assert "null" not in a[:6] and a[6:10] == ["null", "null", "cos", "sin"] and a[11] == "null", c
            assert a[12:15] == [str(B), str(H), str(Hkv)] and a[16:] == [str(v) for v in (cap, 0, 0, 0, d, d, 32, cap, 1, 0, 0, 1)] + ["null"], c
    rec.reset(named)
    mt.attention_stack_step(x[:, :3].contiguous(), layers, H, cache)   # (unfused: apply_rotary at offsets = lengths, then torch indexing)
    assert _names(rec) == ["fa_mi355x_rope", "fa_mi355x_rope", "fa_mi355x_fwd_decode_gqa"] * 2, _names(rec)
    assert all(c.split(",")[4] != "null" for c in rec.calls if c.startswith("fa_mi355x_rope("))
    rec.reset(named)
    mt.attention_stack_ragged(x[0, :50].contiguous(), [7, 40], layers, H, cache)
    assert _names(rec) == pair("fa_mi355x_rope_append_ragged", "fa_mi355x_fwd_ragged", 2), _names(rec)

    # window + sink on a paged cache: the prefill is the chunked one, and everything attends through the _sink entry points
    paged = mt.PagedKVCache(2, B, cap, H, d, torch.bfloat16, x.device, n_kv_head=Hkv, page_size=128, n_pages=8, window=160, sink=4, rope=rope)
    rec.reset({"table": paged.block_table, **named})
    mt.attention_stack_prefill(x, layers, H, paged)
    mt.attention_stack_step_fused(x[:, :1].contiguous(), layers, H, paged)
    mt.attention_stack_ragged(x[0, :50].contiguous(), [7, 40], layers, H, paged)
    assert _names(rec) == (pair("fa_mi355x_rope_append", "fa_mi355x_fwd_extend_sink", 2) + pair("fa_mi355x_rope_append", "fa_mi355x_fwd_decode_sink", 2) +
                           pair("fa_mi355x_rope_append_ragged", "fa_mi355x_fwd_ragged_sink", 2)), _names(rec)
    assert all(",table," in c for c in rec.calls if "workspace_bytes" not in c)
    assert all(c.split("(")[1].split(",")[1:3] == ["null", "null"] for c in rec.calls if "_sink(" in c)   # (attend only)

    if hasattr(torch, "float8_e4m3fn"):
        f8 = mt.KVCache(2, B, cap, H, d, torch.bfloat16, x.device, n_kv_head=Hkv, kv_dtype=torch.float8_e4m3fn,
                        kv_scale=(torch.full((2, Hkv), 0.5), torch.full((2, Hkv), 0.25)), rope=rope)
        rec.reset(named)
        mt.attention_stack_prefill(x[:, :P].contiguous(), layers, H, f8)
        assert _names(rec) == ["fa_mi355x_rope", "fa_mi355x_rope", "fa_mi355x_append_fp8", "fa_mi355x_fwd_gqa"] * 2, _names(rec)
        rec.reset(named)
        mt.attention_stack_prefill_chunked(x, layers, H, f8, 150)
        assert _names(rec) == pair("fa_mi355x_rope_append", "fa_mi355x_fwd_extend_fp8", 2) + pair("fa_mi355x_rope_append", "fa_mi355x_fwd_decode_fp8", 2)
        for c in rec.calls:
            a = c.split("(")[1].rstrip(")").split(",")
            if c.startswith("fa_mi355x_rope_append("):   # the layer's scales, cache_fp8 = 1
                assert a[6] != "null" and a[7] != "null" and a[-3:] == ["1", "1", "null"], c
            elif "_fp8(" in c:
                assert a[1:3] == ["null", "null"], c

    # the tables must cover the cache, a paged one's logical capacity; the rotary dimension fits the head
    with pytest.raises(ValueError, match="max_pos"):
        mt.KVCache(2, B, cap + 1, H, d, torch.bfloat16, x.device, rope=rope)
    with pytest.raises(ValueError, match="max_pos"):
        mt.PagedKVCache(2, B, cap - 100, H, d, torch.bfloat16, x.device, page_size=256, rope=mt.Rotary.table(cap - 100, 32))   # (2 pages: 512 rows)
    with pytest.raises(ValueError, match="rotary dimension"):
        mt.KVCache(2, B, cap, H, 16, torch.bfloat16, x.device, rope=rope)
    with pytest.raises(TypeError, match="Rotary"):
        mt.KVCache(2, B, cap, H, d, torch.bfloat16, x.device, rope=(rope.cos, rope.sin))
    with pytest.raises(ValueError, match="go together|both tables"):
        mt.Rotary(rope.cos, None)

    # the training stack: two rotations per layer in front of the operator; rope=None is the stack it was
    rec.reset(named)
    mt.attention_stack(x[:, :64].contiguous().float(), [tuple(w.float() for w in l) for l in layers], H, rope=rope)
    assert [n for n in _names(rec) if "rope" in n] == ["fa_mi355x_rope"] * 4, _names(rec)
    plain = mt.KVCache(2, B, cap, H, d, torch.bfloat16, x.device, n_kv_head=Hkv)
    assert plain.rope is None and plain.rotary() == {}
    rec.reset({})
    mt.attention_stack(x[:, :64].contiguous().float(), [tuple(w.float() for w in l) for l in layers], H)
    mt.attention_stack_prefill(x[:, :P].contiguous(), layers, H, plain)
    mt.attention_stack_step_fused(x[:, :1].contiguous(), layers, H, plain)
    mt.attention_stack_step(x[:, :1].contiguous(), layers, H, plain)
    mt.attention_stack_extend(x, layers, H, plain)
    mt.attention_stack_ragged(x[0, :50].contiguous(), [7, 40], layers, H, plain)
    names = [c.split("(")[0] for c in rec.calls]
    assert not [n for n in names if "rope" in n] and "fa_mi355x_fwd_decode_append" in names and "fa_mi355x_fwd_ragged_append" in names, names
