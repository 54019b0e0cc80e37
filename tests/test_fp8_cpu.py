"""CPU-side checks of the fp8 KV cache (include/flash_attn_mi355x_decode_fp8.h: decode and extend on caches of e4m3 bytes with
per-kv-head scales, and the quantising append): this file's e4m3 reference (a decode table written from the format's definition and
``quantize``, both used by tests/test_gpu_fp8.py) against torch's CPU float8_e4m3fn cast; ``fp8_reference`` on decode_reference; the
three symbols declared, exported and bound; the FP8 builds in the code object, without scratch; every bad argument answered before
any HIP call (fake non-null pointers, as in tests/test_window_cpu.py: a launch would fail with another code); the Python checks that
need no GPU and the model layer's calls under the recorder."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_abi_cpu import _device_kernels
from test_decode_cpu import _declared, built, decode_reference  # noqa: F401  (built: the module-scoped build fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "flash_attn_mi355x_decode_fp8.h")
FP8 = ["fa_mi355x_fwd_decode_fp8", "fa_mi355x_fwd_extend_fp8", "fa_mi355x_append_fp8"]
NAN_CODES = (0x7F, 0xFF)


# ---- the e4m3 reference (used by tests/test_gpu_fp8.py) ----

def _decode_table():
    """OCP e4m3fn from its definition: 1 sign bit, 4 exponent bits (bias 7), 3 mantissa bits; exponent 0 is subnormal
    (m / 8 * 2^-6), there is no infinity, and S.1111.111 is NaN (so the largest finite value is 1.75 * 2^8 = 448)."""
    t = np.empty(256, dtype=np.float64)
    for c in range(256):
        s, e, m = c >> 7, (c >> 3) & 15, c & 7
        if e == 15 and m == 7:
            v = np.nan
        elif e == 0:
            v = m / 8.0 * 2.0 ** -6
        else:
            v = (1 + m / 8.0) * 2.0 ** (e - 7)
        t[c] = -v if s else v
    return t


TABLE = _decode_table()
FINITE = np.array([c for c in range(256) if c not in NAN_CODES], dtype=np.uint8)
_POS = TABLE[:0x7F]   # the 127 non-negative finite values, ascending: code = index


def rne_e4m3(p):
    """The code of the e4m3 value nearest to each element of the float32 array p (|p| <= 448; ties to the even code; the sign of a
    zero is kept); NaN -> 0x7F."""
    p = np.asarray(p, dtype=np.float32)
    a = np.abs(p).astype(np.float64)
    nan = np.isnan(a)
    a = np.where(nan, 0.0, a)
    assert np.all(a <= 448.0)
    hi = np.clip(np.searchsorted(_POS, a, side="left"), 1, len(_POS) - 1)   # _POS[hi - 1] <= a <= _POS[hi] (or a = 0: hi = 1)
    lo = hi - 1
    dlo, dhi = a - _POS[lo], _POS[hi] - a   # exact in fp64: both are fp32 values
    code = np.where(dlo < dhi, lo, np.where(dhi < dlo, hi, np.where(lo % 2 == 0, lo, hi)))
    code = (code | np.where(np.signbit(p), 0x80, 0)).astype(np.uint8)
    return np.where(nan, np.uint8(0x7F), code).astype(np.uint8)


def quantize(x, scale):
    """code = rne_e4m3(clamp(fp32(x) * (1.0f / scale), -448, 448)): the reciprocal and the product each rounded to fp32; the clamp in
    front of the conversion (overflow saturates to +-448); NaN -> 0x7F.  x: any float array (bf16 values), scale: broadcastable."""
    x = np.asarray(x, dtype=np.float32)
    r = (np.float32(1.0) / np.asarray(scale, dtype=np.float32)).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        p = (x * r).astype(np.float32)
    return rne_e4m3(np.where(np.isnan(p), p, np.clip(p, np.float32(-448), np.float32(448))))


def dequantize(codes, scale=1.0):
    """scale * e4m3 value of every code, fp64."""
    return TABLE[np.asarray(codes, dtype=np.uint8)] * np.asarray(scale, dtype=np.float64)


def fp8_reference(q, k8, v8, k_scale, v_scale, lens, causal, scale):
    """decode_reference on the dequantised, scaled cache: q (BH, Nq, d), k8 / v8 (BH, Ncap, d) uint8 codes, k_scale / v_scale (BH,)
    (the scale of each row's kv head).  Returns (out (BH, Nq, d), lse (BH, Nq))."""
    k = dequantize(k8, np.asarray(k_scale, dtype=np.float64)[:, None, None])
    v = dequantize(v8, np.asarray(v_scale, dtype=np.float64)[:, None, None])
    return decode_reference(q, k, v, lens, causal, scale)


def _grid():
    pos = TABLE[:0x7F]
    mids = (pos[:-1] + pos[1:]) / 2
    rng = np.random.default_rng(0)
    g = np.concatenate([pos, mids, np.nextafter(mids.astype(np.float32), np.float32(1e9)), np.nextafter(mids.astype(np.float32), np.float32(0)),
                        [448, 449, 500, 1e9, 2.0 ** -9, 2.0 ** -10, 1.5 * 2.0 ** -10, 2.0 ** -11, 1e-30, 0.0],
                        rng.uniform(0, 2, 2000), rng.uniform(0, 448, 2000)]).astype(np.float32)
    return np.concatenate([g, -g, [np.nan]]).astype(np.float32)


def test_decode_table_and_quantize_agree_with_torch():
    import torch
    # every code decodes as torch decodes it (NaN exactly at the two NaN codes)
    got = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).to(torch.float64).numpy()
    assert np.array_equal(np.isnan(got), np.isnan(TABLE)) and sorted(np.flatnonzero(np.isnan(TABLE))) == list(NAN_CODES)
    assert np.array_equal(got[FINITE], TABLE[FINITE]) and TABLE[0x7E] == 448 and TABLE[0xFE] == -448 and TABLE[1] == 2.0 ** -9
    assert np.array_equal(np.signbit(got[FINITE]), np.signbit(TABLE[FINITE]))   # (0x80 is -0)
    # every finite code survives a round trip through bf16: the kernels' widening loses nothing
    t = torch.from_numpy(TABLE[FINITE]).to(torch.bfloat16)
    assert np.array_equal(t.to(torch.float64).numpy(), TABLE[FINITE])
    assert np.array_equal(quantize(t.float().numpy(), 1.0), FINITE)
    # quantize on a grid (every value, every midpoint and its neighbours, the format's edges) is torch's cast of the clamped product
    g = _grid()
    for scale in (1.0, 0.5, 4.0, 0.3, 1.7, 448.0 / 3.0):
        r = np.float32(1.0) / np.float32(scale)
        p = torch.from_numpy((g * r).astype(np.float32))
        want = torch.where(torch.isnan(p), p, p.clamp(-448, 448)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
        assert np.array_equal(quantize(g, scale), want), scale
    q1 = lambda x: int(quantize(np.float32(x), 1.0))
    assert q1(448) == q1(449) == q1(500) == q1(1e9) == 0x7E and q1(-449) == q1(-1e9) == 0xFE
    assert q1(2.0 ** -9) == 1 and q1(2.0 ** -10) == 0 and q1(-2.0 ** -10) == 0x80 and q1(1.5 * 2.0 ** -10) == 1
    assert q1(0.0) == 0 and q1(-0.0) == 0x80 and q1(np.nan) == 0x7F
    assert int(quantize(np.float32(3.0), 0.5)) == int(quantize(np.float32(6.0), 1.0))   # (the scale divides)


def test_fp8_reference_is_decode_reference_on_the_scaled_cache():
    rng = np.random.default_rng(3)
    BH, Ncap, d, Nq = 4, 70, 16, 3
    k8, v8 = (FINITE[rng.integers(0, len(FINITE), (BH, Ncap, d))] for _ in range(2))
    q = rng.uniform(-1, 1, (BH, Nq, d))
    ks, vs = rng.uniform(0.01, 0.1, BH), rng.uniform(0.01, 0.1, BH)
    lens = [70, 0, 1, 33]
    out, lse = fp8_reference(q, k8, v8, ks, vs, lens, True, 0.25)
    o1, l1 = fp8_reference(q, k8, v8, np.ones(BH), np.ones(BH), lens, True, 0.25)
    # k_scale is a factor of the softmax scale, v_scale a factor of the output.  (The scale reaches the score by another order of
    # fp64 roundings: a few ulps of 2.2e-16 on scores of up to 0.25 * 16 * 448 * 0.1 = 180 move a weight by some 1e-13 relative.)
    for b in range(BH):
        ob, lb = decode_reference(q[b:b + 1], TABLE[k8[b:b + 1]], TABLE[v8[b:b + 1]], lens[b:b + 1], True, 0.25 * ks[b])
        assert np.allclose(out[b], ob[0] * vs[b], rtol=1e-11, atol=1e-13) and np.allclose(lse[b], lb[0], rtol=1e-11, atol=0)
    assert np.all(out[1] == 0) and np.all(np.isneginf(lse[1])) and np.all(np.isfinite(o1[0])) and not np.array_equal(out[0], o1[0])


# ---- the C ABI ----

def test_the_three_fp8_symbols_are_declared_exported_and_bound(built):
    from test_lib_cpu import _ctypes_kind, _prototypes
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert '#include "flash_attn_mi355x_decode_fp8.h"' in open(os.path.join(ROOT, "include", "flash_attn_mi355x_decode.h")).read()
    assert sorted(set(re.findall(r"\b(fa_mi355x_\w+)\s*\(", text))) == sorted(FP8) == sorted(built.FP8_ABI)
    assert not [s for s in _declared() if "fp8" in s]   # (the decode header's own text declares none of them)
    protos = _prototypes("flash_attn_mi355x_decode_fp8.h")
    lib = built.decode()
    for s in FP8:
        assert hasattr(lib, s), s
        res, args = built.FP8_ABI[s]
        ret, kinds = protos[s]
        assert [_ctypes_kind(a) for a in args] == kinds and _ctypes_kind(res) == ret, s
        assert getattr(lib, s).argtypes == args and getattr(lib, s).restype is res, s


def test_the_library_holds_the_fp8_builds_without_scratch(built):
    kernels = _device_kernels(built.lib_path(built.DECODE_NAME))
    names = [k[0] for k in kernels]
    count = lambda pat: len([n for n in names if re.search(pat, n)])
    # bf16 queries, d in {32, 64, 128}, slab and paged: the last template argument is FP8
    assert count(r"decode_split_kernelIDF16bLi(32|64|128)ELb1ELb[01]ELb0ELb1EEEv") == 6    # grouped, PAGED in {0, 1}, no window
    assert count(r"extend_split_kernelIDF16bLi(32|64|128)ELb[01]ELb0ELb0ELb1EEEv") == 6    # PAGED in {0, 1}, not ragged, no window
    assert count(r"decode_combine_kernelILi(32|64|128)ELb0ELb1EEEv") == 3
    assert count(r"append_fp8_kernelILi[18]ELb[01]EEEv") == 4                              # vector and element builds, slab and paged
    for name, scratch, vgpr in kernels:
        assert scratch == 0, (name, scratch)
        assert vgpr <= 512, (name, vgpr)


# one valid call of each entry point (fake non-null device pointers: a launch would fail, so a code other than the expected one
# shows a HIP call)
_ONE = 16
_GOOD = dict(q=_ONE, kn=_ONE, vn=_ONE, k=_ONE, v=_ONE, ks=_ONE, vs=_ONE, out=_ONE, lse=_ONE, lens=_ONE, table=_ONE, ws=_ONE, B=2, H=4, Hkv=2,
             Nq=100, Ncap=2048, num_pages=40, page_size=128, max_pages=16, d_new=64, d=64, layout=1, scale=0.0, causal=1, dtype=1)
_VP = ctypes.c_void_p
BAD_ARG, BAD_D = 1, 2


def _call(lib, entry, **over):
    a = dict(_GOOD, **over)
    geo = [a[n] for n in ("Ncap", "num_pages", "page_size", "max_pages", "d_new", "d", "layout")]
    if entry == "append":
        args = [_VP(a[n]) for n in ("kn", "vn", "k", "v", "ks", "vs", "lens", "table")] + [a["B"], a["Hkv"], a["Nq"]] + geo + [a["dtype"], None]
        rc = lib.fa_mi355x_append_fp8(*args)
    else:
        args = ([_VP(a[n]) for n in ("q", "kn", "vn", "k", "v", "ks", "vs", "out", "lse", "lens", "table", "ws")] +
                [a["B"], a["H"], a["Hkv"], a["Nq"]] + geo + [a["scale"], a["causal"], a["dtype"], None])
        rc = getattr(lib, f"fa_mi355x_fwd_{entry}_fp8")(*args)
    return rc, lib.fa_mi355x_decode_last_error().decode()


_SLAB, _ATTEND_ONLY, _NO_SCALES = dict(table=0), dict(kn=0, vn=0), dict(ks=0, vs=0)
_BAD_ATTEND = [   # the family's checks through the fp8 entry points: attend-only and fused, slab and paged
    (dict(dtype=0), BAD_ARG, "FA_DTYPE_F32"), (dict(dtype=0, **_SLAB, **_ATTEND_ONLY), BAD_ARG, "FA_DTYPE_F32"), (dict(dtype=5), BAD_ARG, "dtype"),
    (dict(kn=0), BAD_ARG, "null"), (dict(vn=0, **_SLAB), BAD_ARG, "null"),
    (dict(q=0), BAD_ARG, "null"), (dict(k=0, **_SLAB), BAD_ARG, "null"), (dict(out=0, **_ATTEND_ONLY), BAD_ARG, "null"),
    (dict(B=0), BAD_ARG, "positive"), (dict(Nq=0, **_SLAB), BAD_ARG, "positive"), (dict(Ncap=0, **_SLAB), BAD_ARG, "positive"),
    (dict(H=8, Hkv=3), BAD_ARG, "Hkv = 3"), (dict(layout=2), BAD_ARG, "layout"),
    (dict(d=48, d_new=48), BAD_D, "32, 64, 128"), (dict(d=256, d_new=256, **_SLAB, **_ATTEND_ONLY), BAD_D, "32, 64, 128"),
    (dict(scale=-1.0), BAD_ARG, "softmax_scale"), (dict(scale=float("nan"), **_SLAB), BAD_ARG, "softmax_scale"),
    (dict(d_new=65), BAD_ARG, "d_new = 65"), (dict(d_new=0, **_SLAB), BAD_ARG, "d_new = 0"),
    (dict(page_size=192), BAD_ARG, "page_size"), (dict(page_size=64), BAD_ARG, "page_size"), (dict(num_pages=0), BAD_ARG, "num_pages"),
    (dict(max_pages=0), BAD_ARG, "max_pages"), (dict(max_pages=1 << 24), BAD_ARG, "max_pages * page_size"),
    # the bounds count one byte per element: 2^24 rows of Hkv * d = 128 bytes are 2 GiB, 2^23 rows are legal (and illegal at two
    # bytes: test_the_cache_bounds_count_one_byte_per_element), so that call gets as far as the last check, the workspace
    (dict(Ncap=1 << 24, **_SLAB), BAD_ARG, "2 GiB"), (dict(page_size=1 << 24), BAD_ARG, "2 GiB"),
    (dict(Ncap=1 << 23, ws=0, **_SLAB), BAD_ARG, "workspace"), (dict(page_size=1 << 23, ws=0), BAD_ARG, "workspace"),
    # null scales are accepted (all ones): the call gets as far as the workspace check as well
    (dict(ws=0, Ncap=65536, **_SLAB, **_NO_SCALES), BAD_ARG, "workspace"), (dict(ws=0, max_pages=512, **_NO_SCALES), BAD_ARG, "workspace"),
    (dict(ws=0, Ncap=65536, ks=0, **_SLAB, **_ATTEND_ONLY), BAD_ARG, "workspace"),
]
_BAD_APPEND = [
    (dict(dtype=0), BAD_ARG, "FA_DTYPE_F32"), (dict(dtype=5, **_SLAB), BAD_ARG, "dtype"),
    (dict(kn=0), BAD_ARG, "null"), (dict(vn=0, **_SLAB), BAD_ARG, "null"), (dict(k=0), BAD_ARG, "null"), (dict(v=0, **_SLAB), BAD_ARG, "null"),
    (dict(B=0), BAD_ARG, "positive"), (dict(Nq=0, **_SLAB), BAD_ARG, "positive"), (dict(Ncap=0, **_SLAB), BAD_ARG, "positive"),
    (dict(layout=2), BAD_ARG, "layout"), (dict(d=48, d_new=48), BAD_D, "32, 64, 128"),
    (dict(d_new=65, **_NO_SCALES), BAD_ARG, "d_new = 65"), (dict(d_new=0, **_SLAB), BAD_ARG, "d_new = 0"),
    (dict(page_size=192), BAD_ARG, "page_size"), (dict(num_pages=0), BAD_ARG, "num_pages"), (dict(max_pages=0), BAD_ARG, "max_pages"),
    (dict(Ncap=1 << 24, **_SLAB), BAD_ARG, "2 GiB"), (dict(page_size=1 << 24), BAD_ARG, "2 GiB"),
    (dict(Nq=129, d_new=65), BAD_ARG, "d_new = 65"),   # (any Nq >= 1: 129 new tokens are not what is wrong with this call)
]
_TWO_FAULTS = [   # which error wins: the dtype prelude, the page geometry, then the family's checks (all three entry points)
    (dict(dtype=0, kn=0), BAD_ARG, "FA_DTYPE_F32"), (dict(dtype=0, page_size=64), BAD_ARG, "FA_DTYPE_F32"), (dict(dtype=0, B=0), BAD_ARG, "FA_DTYPE_F32"),
    (dict(dtype=5, num_pages=0), BAD_ARG, "unknown dtype"), (dict(dtype=5, d=48, d_new=48, **_SLAB), BAD_ARG, "unknown dtype"),
    (dict(page_size=192, kn=0), BAD_ARG, "page_size = 192"), (dict(max_pages=0, layout=2), BAD_ARG, "max_pages"),
    (dict(layout=2, k=0), BAD_ARG, "unknown layout"),
]


def _cases():
    out = [(e, o, c, m) for e in ("decode", "extend") for o, c, m in _BAD_ATTEND] + [("append", o, c, m) for o, c, m in _BAD_APPEND]
    out += [(e, o, c, m) for e in ("decode", "extend", "append") for o, c, m in _TWO_FAULTS]
    out += [(e, dict(q=0, d_new=65), BAD_ARG, "null pointer argument") for e in ("decode", "extend")]   # (the attention's before the append's)
    # the cache bound: the attention's own check in the fused calls, after the append's checks in the append alone
    out += [(e, dict(d_new=65, Ncap=1 << 24, **_SLAB), BAD_ARG, "2 GiB") for e in ("decode", "extend")]
    out.append(("append", dict(d_new=65, Ncap=1 << 24, **_SLAB), BAD_ARG, "d_new = 65"))
    out += [("decode", dict(Nq=129), BAD_ARG, "Nq > 128"), ("decode", dict(Nq=129, **_SLAB, **_ATTEND_ONLY), BAD_ARG, "Nq > 128"),
            ("extend", dict(Nq=129, d_new=65), BAD_ARG, "d_new = 65"),
            ("extend", dict(H=1 << 12, Hkv=1, Nq=1 << 13, d=32, d_new=32), BAD_ARG, "2^25")]
    return out


def _id(case):
    return case[0] + "-" + ",".join(f"{k}={v}" for k, v in case[1].items())


@pytest.mark.parametrize("entry,over,code,msg", _cases(), ids=[_id(c) for c in _cases()])
def test_fp8_forms_reject_each_bad_argument_before_any_hip_call(built, entry, over, code, msg):
    rc, err = _call(built.decode(), entry, **over)
    assert rc == code and err and msg in err, (rc, err)


def test_the_cache_bounds_count_one_byte_per_element(built):
    """A slab of 2^23 rows of Hkv * d = 128 elements is 1 GiB of e4m3 bytes and 2 GiB of bf16: the bf16 call refuses it, the fp8 call
    takes it (and stops at the null workspace, the last check in front of the launches).  The same for one page of a pool."""
    lib = built.decode()
    a = dict(_GOOD, Ncap=1 << 23, ws=0)
    vp = lambda n: _VP(a[n])
    bf16 = lib.fa_mi355x_fwd_decode_gqa(vp("q"), vp("k"), vp("v"), vp("out"), vp("lse"), vp("lens"), vp("ws"), a["B"], a["H"], a["Hkv"], 1,
                                        a["Ncap"], a["d"], a["layout"], 0.0, 1, 1, None)
    assert bf16 == BAD_ARG and "2 GiB" in lib.fa_mi355x_decode_last_error().decode()
    for entry in ("decode", "extend"):
        rc, err = _call(lib, entry, Ncap=1 << 23, ws=0, Nq=1, table=0)
        assert rc == BAD_ARG and "workspace" in err, err
    paged = lib.fa_mi355x_fwd_decode_paged(vp("q"), vp("k"), vp("v"), vp("out"), vp("lse"), vp("lens"), vp("table"), vp("ws"), a["B"], a["H"],
                                           a["Hkv"], 1, 40, 1 << 23, 16, a["d"], a["layout"], 0.0, 1, 1, None)
    assert paged == BAD_ARG and "2 GiB" in lib.fa_mi355x_decode_last_error().decode()
    rc, err = _call(lib, "decode", page_size=1 << 23, ws=0, Nq=1)
    assert rc == BAD_ARG and "workspace" in err, err
    # the splits and the workspace of an fp8 call are the bf16 call's: the existing queries answer, for either dtype code
    assert lib.fa_mi355x_decode_splits_gqa(2, 4, 2, 1, 4096, 64, 1) == lib.fa_mi355x_decode_splits_gqa(2, 4, 2, 1, 4096, 64, 0) > 1
    assert lib.fa_mi355x_decode_splits(1, 2, 1, 4096, 64, 1) > 1   # (the multi-split shape of tests/test_gpu_fp8.py)


# ---- the Python layer ----

def test_fp8_python_checks_that_need_no_gpu(built):
    import torch
    from flash_attention_minitorch_amd import device_ops

    f8, bf = torch.float8_e4m3fn, torch.bfloat16
    q, kc = torch.zeros(2, 1, 4, 64, dtype=bf), torch.zeros(2, 256, 2, 64, dtype=f8)
    kn = torch.zeros(2, 1, 2, 64, dtype=bf)
    ones = torch.ones(2)
    calls = [lambda q=q, **kw: device_ops.flash_attn_decode(q, kc, kc.clone(), **kw), lambda q=q, **kw: device_ops.flash_attn_extend(q, kc, kc.clone(), **kw)]
    appends = [device_ops.decode_append, device_ops.extend_append]
    for call in calls:
        with pytest.raises(TypeError, match="bfloat16"):
            call(q=q.float())
        with pytest.raises(TypeError, match="share one dtype"):
            device_ops.flash_attn_decode(q, kc, kc.to(bf))
        with pytest.raises(TypeError, match="float32"):
            call(k_scale=ones.double())
        with pytest.raises(TypeError, match="float32"):
            call(v_scale=[1.0, 1.0])
        for bad in (torch.ones(3), torch.ones(2, 1), torch.ones(4)[::2], torch.ones(2, device="meta")):
            with pytest.raises(ValueError, match="Hkv"):
                call(k_scale=bad)
            with pytest.raises(ValueError, match="Hkv"):
                call(k_scale=ones, v_scale=bad)
        with pytest.raises(ValueError, match="window"):
            call(window=8)
        with pytest.raises(TypeError, match="bfloat16"):
            call(k_new=kn.float(), v_new=kn.float())
        for ok in (dict(), dict(k_scale=ones), dict(k_scale=ones, v_scale=ones * 0.5), dict(k_new=kn, v_new=kn, v_scale=ones)):
            with pytest.raises(built.FlashAttnLibraryError, match="GPU"):   # past the fp8 checks: the next complaint is the missing GPU
                call(**ok)
    # scales with a cache that is not fp8 are an error, not ignored
    kb = torch.zeros(2, 256, 2, 64, dtype=bf)
    for kw in (dict(k_scale=ones), dict(v_scale=ones)):
        with pytest.raises(ValueError, match="fp8"):
            device_ops.flash_attn_decode(q, kb, kb.clone(), **kw)
        with pytest.raises(ValueError, match="fp8"):
            device_ops.flash_attn_extend(q, kb, kb.clone(), **kw)
        for append in appends:
            with pytest.raises(ValueError, match="fp8"):
                append(kn, kn, kb, kb.clone(), **kw)
    for append in appends:
        with pytest.raises(TypeError, match="bfloat16"):
            append(kn.float(), kn.float(), kc, kc.clone())
        with pytest.raises(ValueError, match="Hkv"):
            append(kn, kn, kc, kc.clone(), k_scale=torch.ones(3))
        with pytest.raises(built.FlashAttnLibraryError, match="GPU"):
            append(kn, kn, kc, kc.clone(), k_scale=ones, v_scale=ones)
    # the ragged calls do not take an fp8 cache
    qr, cu = torch.zeros(40, 4, 64, dtype=bf), torch.zeros(3, dtype=torch.int32)
    with pytest.raises(TypeError, match="ragged"):
        device_ops.flash_attn_ragged(qr, kc, kc.clone(), cu)
    with pytest.raises(TypeError, match="ragged"):
        device_ops.ragged_append(torch.zeros(40, 2, 64, dtype=bf), torch.zeros(40, 2, 64, dtype=bf), kc, kc.clone(), cu)
    # the workspace queries take an fp8 cache and give the bf16 call's size
    big8, bigb = torch.zeros(2, 4096, 2, 64, dtype=f8), torch.zeros(2, 4096, 2, 64, dtype=bf)
    n = lambda t: 0 if t is None else t.numel() * 4
    assert n(device_ops.decode_workspace(q, big8)) == n(device_ops.decode_workspace(q, bigb)) > 0
    assert n(device_ops.extend_workspace(q, big8)) == n(device_ops.extend_workspace(q, bigb)) > 0


def test_model_fp8_calls_under_the_recorder(monkeypatch):
    """The stack functions on an fp8 cache under the recorder of tests/test_device_ops_cpu.py (CPU tensors, no library): a prompt is
    appended through fa_mi355x_append_fp8 and attends through the square forward; every step and extend call is the family's _fp8
    entry point, fused with the append, with the layer's scales; the paths that are not built raise; a cache that is not fp8 makes
    the calls it made before."""
    import torch
    from flash_attention_minitorch_amd import modules_transformer as mt
    from test_device_ops_cpu import install_recorder

    rec = install_recorder(monkeypatch)
    f8 = torch.float8_e4m3fn
    B, P, H, Hkv, d, cap = 2, 130, 4, 2, 64, 512
    g = torch.Generator().manual_seed(0)
    x = torch.randn((B, 200, H * d), generator=g).to(torch.bfloat16)
    wq, wk = (torch.randn(s, generator=g).to(torch.bfloat16) for s in ((H * d, H * d), (H * d, Hkv * d)))
    layers = [(wq, wk, wk, wq)] * 2
    scales = (torch.full((2, Hkv), 0.5), torch.full((2, Hkv), 0.25))

    cache = mt.KVCache(2, B, cap, H, d, torch.bfloat16, x.device, n_kv_head=Hkv, kv_dtype=f8, kv_scale=scales)
    assert cache.fp8 and cache.k[0].dtype == f8 and cache.k[0].shape == (B, cap, Hkv, d) and cache.quant(1)["v_scale"].shape == (Hkv,)
    named = {"ks0": cache.kv_scale[0][0], "ks1": cache.kv_scale[0][1], "vs0": cache.kv_scale[1][0], "vs1": cache.kv_scale[1][1],
             "k0": cache.k[0], "v0": cache.v[0], "k1": cache.k[1], "v1": cache.v[1], "lens": cache.lengths}
    rec.reset(named)
    mt.attention_stack_prefill(x[:, :P].contiguous(), layers, H, cache)
    calls = [c for c in rec.calls if "workspace_bytes" not in c and "guard" not in c]
    assert [c.split("(")[0] for c in calls] == ["fa_mi355x_append_fp8", "fa_mi355x_fwd_gqa"] * 2, calls
    for li in (0, 1):
        args = calls[2 * li].split("(")[1].rstrip(")").split(",")
        assert args[2:8] == [f"k{li}", f"v{li}", f"ks{li}", f"vs{li}", "lens", "null"], args
        assert args[8:] == [str(v) for v in (B, Hkv, P, cap, 0, 0, 0, d, d, 1, 1)] + ["null"], args
    assert cache.length_bound == P

    rec.reset(named)
    mt.attention_stack_step_fused(x[:, :1].contiguous(), layers, H, cache)
    mt.attention_stack_extend(x, layers, H, cache)
    calls = [c for c in rec.calls if "workspace_bytes" not in c]
    assert [c.split("(")[0] for c in calls] == ["fa_mi355x_fwd_decode_fp8"] * 2 + ["fa_mi355x_fwd_extend_fp8"] * 2, calls
    for i, c in enumerate(calls):
        li, n = i % 2, 1 if i < 2 else 200
        args = c.split("(")[1].rstrip(")").split(",")
        assert args[1] != "null" and args[2] != "null" and args[3:7] == [f"k{li}", f"v{li}", f"ks{li}", f"vs{li}"], args
        assert args[10] == "null" and args[12:] == [str(v) for v in (B, H, Hkv, n, cap, 0, 0, 0, d, d, 1)] + ["0.0", "1", "1", "null"], args
    assert cache.length_bound == P + 201
    with pytest.raises(ValueError, match="attention_stack_step_fused"):
        mt.attention_stack_step(x[:, :1].contiguous(), layers, H, cache)
    with pytest.raises(ValueError, match="ragged"):
        mt.attention_stack_ragged(x[0, :50].contiguous(), [7, 40], layers, H, cache)
    with pytest.raises(ValueError, match="window"):
        mt.KVCache(2, B, cap, H, d, torch.bfloat16, x.device, n_kv_head=Hkv, kv_dtype=f8, window=64)
    with pytest.raises(ValueError, match="window"):
        mt.PagedKVCache(2, B, cap, H, d, torch.bfloat16, x.device, n_kv_head=Hkv, kv_dtype=f8, window=64)
    with pytest.raises(TypeError, match="bfloat16"):
        mt.KVCache(2, B, cap, H, d, torch.float32, x.device, n_kv_head=Hkv, kv_dtype=f8)
    with pytest.raises(ValueError, match="kv_scale"):
        mt.KVCache(2, B, cap, H, d, torch.bfloat16, x.device, n_kv_head=Hkv, kv_scale=scales)
    with pytest.raises(ValueError, match="kv_scale"):
        mt.KVCache(2, B, cap, H, d, torch.bfloat16, x.device, n_kv_head=Hkv, kv_dtype=f8, kv_scale=(scales[0], torch.ones(2, 3)))
    with pytest.raises(ValueError, match="kv_dtype"):
        mt.KVCache(2, B, cap, H, d, torch.bfloat16, x.device, n_kv_head=Hkv, kv_dtype=torch.float16)

    # a paged fp8 cache without scales: the table and the pool's geometry, null scales; the chunked prefill and a graph-sized step
    paged = mt.PagedKVCache(2, B, cap, H, d, torch.bfloat16, x.device, n_kv_head=Hkv, page_size=128, n_pages=7, kv_dtype=f8)
    assert paged.quant(0) == {} and paged.k[0].dtype == f8
    rec.reset({"table": paged.block_table})
    mt.attention_stack_prefill(x[:, :P].contiguous(), layers, H, paged)
    mt.attention_stack_prefill_chunked(x, layers, H, paged, 150)
    calls = [c for c in rec.calls if "workspace_bytes" not in c and "guard" not in c]
    assert [c.split("(")[0] for c in calls] == (["fa_mi355x_append_fp8", "fa_mi355x_fwd_gqa"] * 2 + ["fa_mi355x_fwd_extend_fp8"] * 2 +
                                                 ["fa_mi355x_fwd_decode_fp8"] * 2), calls
    tail = lambda n: f",{B},{H},{Hkv},{n},0,7,128,4,64,64,1,0.0,1,1,null)"
    assert all(",null,null," in c and ",table," in c for c in calls if "fwd_" in c and "gqa" not in c)
    args = calls[0].split("(")[1].rstrip(")").split(",")   # the paged append: null scales, the table, the pool's geometry for Ncap
    assert args[4:6] == ["null", "null"] and args[7:] == ["table"] + [str(v) for v in (B, Hkv, P, 0, 7, 128, 4, d, d, 1, 1)] + ["null"], args
    assert calls[4].endswith(tail(150)) and calls[6].endswith(tail(50)), (calls[4], calls[6])

    plain = mt.KVCache(2, B, cap, H, d, torch.bfloat16, x.device, n_kv_head=Hkv)
    assert not plain.fp8 and plain.quant(0) == {} and plain.kv_scale is None
    rec.reset({})
    mt.attention_stack_prefill(x[:, :P].contiguous(), layers, H, plain)
    mt.attention_stack_step_fused(x[:, :1].contiguous(), layers, H, plain)
    names = [c.split("(")[0] for c in rec.calls]
    assert not [n for n in names if "fp8" in n] and "fa_mi355x_fwd_decode_append" in names, names
