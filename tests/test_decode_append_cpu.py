"""CPU-side checks of the fused KV-cache append (fa_mi355x_decode_append / fa_mi355x_fwd_decode_append of
include/flash_attn_mi355x_decode.h): exported symbols, argument validation before any HIP call (the append's own table, and the
ungrouped table of tests/test_decode_cpu.py through the fused entry point), the Python layer's checks, and this file's NumPy statement
of the placement rule (used by tests/test_gpu_decode_append.py) on hand-made cases."""
import ctypes

import numpy as np
import pytest

from test_decode_cpu import _BAD, _GOOD, _declared, built  # noqa: F401  (built: the module-scoped build fixture)

APPEND_SYMBOLS = {"fa_mi355x_decode_append", "fa_mi355x_fwd_decode_append"}


def append_reference(k_new, cache, lens, Nq):
    """The placement rule: k_new (B, Nq, Hkv, d_new) into a copy of cache (B, Ncap, Hkv, d), lens (B,) or None (= Ncap), the valid rows
    COUNTING the Nq new tokens.  With L = clamp(len, 0, Ncap), token i goes to row L - Nq + i when that is >= 0; columns d_new .. d-1
    of a written row become zero; every other row keeps its bits."""
    B, n, Hkv, d_new = k_new.shape
    Ncap = cache.shape[1]
    assert n == Nq and cache.shape[0] == B and cache.shape[2] == Hkv and d_new <= cache.shape[3]
    out = cache.copy()
    for b in range(B):
        L = Ncap if lens is None else min(max(int(lens[b]), 0), Ncap)
        for i in range(Nq):
            row = L - Nq + i
            if row >= 0:
                out[b, row] = 0
                out[b, row, :, :d_new] = k_new[b, i]
    return out


def test_append_symbols_are_declared_exported_and_bound(built):
    assert APPEND_SYMBOLS <= set(_declared())
    lib = built.decode()
    for s in APPEND_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in built.DECODE_ABI


# one valid append (fake non-null device pointers: a launch would fail, so a code other than the expected one shows a HIP call)
_ONE = 16
_GOOD_APP = dict(k_new=_ONE, v_new=_ONE, k=_ONE, v=_ONE, lens=_ONE, B=1, Hkv=2, Nq=1, Ncap=4096, d_new=64, d=64, layout=1, dtype=1)
_BAD_APP = [
    ("k_new", 0, 1, "null"), ("v_new", 0, 1, "null"), ("k", 0, 1, "null"), ("v", 0, 1, "null"),
    ("B", 0, 1, "positive"), ("Hkv", -1, 1, "positive"), ("Nq", 0, 1, "positive"), ("Ncap", 0, 1, "positive"), ("d", 0, 1, "positive"),
    ("Nq", 129, 1, "128"),
    ("layout", 2, 1, "layout"), ("dtype", 5, 1, "dtype"),
    ("d", 48, 2, "32, 64, 128"), ("d", 256, 2, "32, 64, 128"),
    ("d_new", 0, 1, "d_new = 0"), ("d_new", -3, 1, "d_new = -3"), ("d_new", 65, 1, "d_new = 65"),
    ("B", 1 << 30, 1, "too many"),
]


def _append(lib, **over):
    a = dict(_GOOD_APP, **over)
    vp = ctypes.c_void_p
    return lib.fa_mi355x_decode_append(vp(a["k_new"]), vp(a["v_new"]), vp(a["k"]), vp(a["v"]), vp(a["lens"]), a["B"], a["Hkv"], a["Nq"],
                                       a["Ncap"], a["d_new"], a["d"], a["layout"], a["dtype"], None)


@pytest.mark.parametrize("field,value,code,msg", _BAD_APP, ids=[f"{f}={v}" for f, v, _, _ in _BAD_APP])
def test_append_rejects_each_bad_argument_before_any_hip_call(built, field, value, code, msg):
    lib = built.decode()
    over = {field: value}
    if (field, value) == ("B", 1 << 30):   # 2^30 * 128 tokens * 64 heads of 64 elements: more workgroups than a launch takes
        over.update(Nq=128, Hkv=64)
    assert _append(lib, **over) == code
    err = lib.fa_mi355x_decode_last_error().decode()
    assert err and msg in err, err


def _fused(lib, **over):
    a = dict(_GOOD, Hkv=_GOOD["H"], k_new=_ONE, v_new=_ONE, d_new=_GOOD["d"])
    a.update(over)
    if "H" in over and "Hkv" not in over:   # the ungrouped table's cases: Hkv follows H
        a["Hkv"] = a["H"]
    if "d" in over and "d_new" not in over and over["d"] > 0:   # ... and the new rows are as long as the cache's
        a["d_new"] = a["d"]
    vp = ctypes.c_void_p
    return lib.fa_mi355x_fwd_decode_append(vp(a["q"]), vp(a["k_new"]), vp(a["v_new"]), vp(a["k"]), vp(a["v"]), vp(a["out"]), vp(a["lse"]),
                                           vp(a["lens"]), vp(a["ws"]), a["B"], a["H"], a["Hkv"], a["Nq"], a["Ncap"], a["d_new"], a["d"],
                                           a["layout"], a["scale"], a["causal"], a["dtype"], None)


@pytest.mark.parametrize("field,value,code,msg", _BAD, ids=[f"{f}={v}" for f, v, _, _ in _BAD])
def test_fused_entry_point_answers_the_ungrouped_table_as_the_gqa_one_does(built, field, value, code, msg):
    from test_decode_gqa_cpu import _call as gqa_call
    lib = built.decode()
    assert gqa_call(lib, **{field: value}) == code
    want = lib.fa_mi355x_decode_last_error().decode()
    assert _fused(lib, **{field: value}) == code
    err = lib.fa_mi355x_decode_last_error().decode()
    assert err == want and msg in err, (err, want)


_BAD_FUSED = [
    (dict(k_new=0), 1, "null"), (dict(v_new=0), 1, "null"),
    (dict(d_new=0), 1, "d_new = 0"), (dict(d_new=65), 1, "d_new = 65"), (dict(d=128, d_new=129), 1, "d_new = 129"),
    (dict(H=8, Hkv=3), 1, "Hkv = 3"), (dict(Hkv=0), 1, "Hkv"),
    (dict(H=16, Hkv=1, Ncap=1 << 21, ws=0), 1, "workspace"),
]


@pytest.mark.parametrize("over,code,msg", _BAD_FUSED, ids=[",".join(f"{k}={v}" for k, v in o.items()) for o, _, _ in _BAD_FUSED])
def test_fused_entry_point_rejects_the_appends_bad_arguments_before_any_hip_call(built, over, code, msg):
    lib = built.decode()
    assert _fused(lib, **over) == code
    err = lib.fa_mi355x_decode_last_error().decode()
    assert err and msg in err, err


def test_flash_attn_decode_checks_k_new_and_v_new_without_a_gpu(built):
    import torch
    from flash_attention_minitorch_amd import device_ops

    q = torch.zeros(2, 3, 4, 64)
    kc, vc = torch.zeros(2, 256, 2, 64), torch.zeros(2, 256, 2, 64)
    kn = torch.zeros(2, 3, 2, 48)
    call = lambda k_new, v_new, **kw: device_ops.flash_attn_decode(q, kc, vc, k_new=k_new, v_new=v_new, **kw)
    for a, b in ((kn, None), (None, kn)):
        with pytest.raises(ValueError, match="together"):
            call(a, b)
    with pytest.raises(ValueError, match=r"\(B, Hkv\)"):
        call(torch.zeros(2, 3, 4, 48), torch.zeros(2, 3, 4, 48))
    with pytest.raises(ValueError, match=r"\(B, Hkv\)"):
        call(torch.zeros(3, 3, 2, 48), torch.zeros(3, 3, 2, 48))
    with pytest.raises(TypeError, match="dtype"):
        call(kn.bfloat16(), kn.bfloat16())
    with pytest.raises(TypeError, match="dtype"):
        call(kn, kn.bfloat16())
    for dn in (0, 65):
        with pytest.raises(ValueError, match="head dim"):
            call(torch.zeros(2, 3, 2, dn), torch.zeros(2, 3, 2, dn))
    with pytest.raises(ValueError, match="one shape"):
        call(kn, torch.zeros(2, 3, 2, 64))
    with pytest.raises(ValueError, match="new tokens"):
        call(torch.zeros(2, 1, 2, 48), torch.zeros(2, 1, 2, 48))
    with pytest.raises(ValueError, match="contiguous"):
        call(torch.zeros(2, 3, 2, 96)[..., :48], kn)
    with pytest.raises(ValueError, match="contiguous"):
        call(kn, torch.zeros(2, 2, 3, 48).transpose(1, 2))
    with pytest.raises(ValueError, match="device"):
        call(kn, torch.zeros(2, 3, 2, 48, device="meta"))
    # "bhnd": the new tokens are (B, Hkv, Nq, d_new)
    qh, kh = q.transpose(1, 2).contiguous(), kc.transpose(1, 2).contiguous()
    with pytest.raises(ValueError, match=r"\(B, Hkv\)"):
        device_ops.flash_attn_decode(qh, kh, kh.clone(), k_new=kn, v_new=kn, layout="bhnd")
    # past every check: the tensors are not on a GPU.  Without k_new the call is the one it was.
    for kw in (dict(k_new=kn, v_new=kn.clone()), dict(k_new=torch.zeros(2, 3, 2, 64), v_new=torch.zeros(2, 3, 2, 64)), dict()):
        with pytest.raises(built.FlashAttnLibraryError, match="GPU"):
            device_ops.flash_attn_decode(q, kc, vc, **kw)
    with pytest.raises(built.FlashAttnLibraryError, match="GPU"):
        device_ops.flash_attn_decode(qh, kh, kh.clone(), k_new=kn.transpose(1, 2).contiguous(), v_new=kn.transpose(1, 2).contiguous(),
                                     layout="bhnd")


def test_decode_append_python_checks(built):
    import torch
    from flash_attention_minitorch_amd import device_ops

    kc, vc = torch.zeros(2, 256, 2, 64), torch.zeros(2, 256, 2, 64)
    kn = torch.zeros(2, 3, 2, 48)
    with pytest.raises(ValueError, match="layout"):
        device_ops.decode_append(kn, kn, kc, vc, layout="nbhd")
    with pytest.raises(ValueError, match="one shape"):
        device_ops.decode_append(kn, kn, kc, torch.zeros(2, 128, 2, 64))
    with pytest.raises(TypeError, match="dtype"):
        device_ops.decode_append(kn, kn, kc, vc.bfloat16())
    with pytest.raises(TypeError, match="dtype"):
        device_ops.decode_append(kn.double(), kn.double(), kc.double(), vc.double())
    with pytest.raises(ValueError, match=r"\(B, Hkv\)"):
        device_ops.decode_append(kn, kn, torch.zeros(2, 256, 4, 64), torch.zeros(2, 256, 4, 64))
    with pytest.raises(ValueError, match="head dim"):
        device_ops.decode_append(torch.zeros(2, 3, 2, 80), torch.zeros(2, 3, 2, 80), kc, vc)
    with pytest.raises(ValueError, match="cache_seqlens"):
        device_ops.decode_append(kn, kn, kc, vc, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="contiguous"):
        device_ops.decode_append(kn, kn, torch.zeros(2, 256, 2, 128)[..., :64], torch.zeros(2, 256, 2, 128)[..., :64])
    with pytest.raises(built.FlashAttnLibraryError, match="GPU"):
        device_ops.decode_append(kn, kn.clone(), kc, vc, torch.zeros(2, dtype=torch.int32))


def test_fused_step_makes_one_fused_call_per_layer_and_the_plain_step_none(monkeypatch):
    """The C calls of the two model steps under the recorder of tests/test_device_ops_cpu.py (CPU tensors, no library): the fused step
    hands the projections' k and v (48 columns into rows of 64) to fa_mi355x_fwd_decode_append, attention_stack_step keeps its calls."""
    import torch
    from flash_attention_minitorch_amd import modules_transformer as mt
    from test_device_ops_cpu import install_recorder

    rec = install_recorder(monkeypatch)
    B, P, H, d, cap = 2, 16, 2, 48, 64
    g = torch.Generator().manual_seed(0)
    x, x1, w = (torch.randn(s, generator=g).to(torch.bfloat16) for s in ((B, P, H * d), (B, 1, H * d), (H * d, H * d)))
    layers = [(w, w, w, w)] * 2
    for step, symbol in ((mt.attention_stack_step_fused, "fa_mi355x_fwd_decode_append"), (mt.attention_stack_step, "fa_mi355x_fwd_decode")):
        cache = mt.KVCache(2, B, cap, H, d, torch.bfloat16, x.device)
        mt.attention_stack_prefill(x, layers, H, cache)
        rec.reset({})
        y = step(x1, layers, H, cache)
        calls = [c for c in rec.calls if "workspace_bytes" not in c]
        assert len(calls) == 2 and all(c.startswith(symbol + "(") for c in calls), calls
        if step is mt.attention_stack_step_fused:   # ... B, H, Hkv, Nq, Ncap, d_new, d, layout, scale, causal, dtype, stream
            assert all(c.endswith(f",2,2,2,1,64,48,64,1,{48 ** -0.5!r},1,1,null)") for c in calls), calls
        assert y.shape == (B, 1, H * d) and cache.length_bound == P + 1 and cache.lengths.tolist() == [P + 1] * B


def test_append_reference_on_hand_made_cases():
    B, Nq, Hkv, Ncap, d, d_new = 5, 3, 2, 6, 4, 3
    rng = np.random.default_rng(0)
    k_new = rng.uniform(1, 2, (B, Nq, Hkv, d_new)).astype(np.float32)
    cache = np.full((B, Ncap, Hkv, d), -7.0, dtype=np.float32)
    lens = [2, 0, 9, 6, 4]   # len < Nq, len = 0, len > Ncap, len = Ncap, an interior length
    got = append_reference(k_new, cache, lens, Nq)
    assert np.all(cache == -7.0)   # (the input is left alone)
    padded = np.concatenate([k_new, np.zeros((B, Nq, Hkv, d - d_new), np.float32)], axis=-1)
    # len = 2 < Nq = 3: token 0 would sit at row -1 and is dropped; tokens 1, 2 are rows 0, 1
    assert np.array_equal(got[0, :2], padded[0, 1:]) and np.all(got[0, 2:] == -7.0)
    # len = 0: nothing is written
    assert np.all(got[1] == -7.0)
    # len = 9 > Ncap and len = Ncap alike: the last Nq rows
    for b in (2, 3):
        assert np.all(got[b, :Ncap - Nq] == -7.0) and np.array_equal(got[b, Ncap - Nq:], padded[b])
    # len = 4: rows 1 .. 3
    assert np.all(got[4, :1] == -7.0) and np.array_equal(got[4, 1:4], padded[4]) and np.all(got[4, 4:] == -7.0)
    # no lengths: every batch element is full
    full = append_reference(k_new, cache, None, Nq)
    assert all(np.array_equal(full[b], got[3] if b == 3 else append_reference(k_new[b:b + 1], cache[b:b + 1], [Ncap], Nq)[0])
               for b in range(B))
    # zero columns replace whatever the cache held there, NaN included; d_new = d leaves none
    nan_cache = np.full((1, Ncap, Hkv, d), np.nan, dtype=np.float32)
    got = append_reference(k_new[:1], nan_cache, [5], Nq)
    assert np.array_equal(got[0, 2:5], padded[0]) and np.all(np.isnan(got[0, :2])) and np.all(np.isnan(got[0, 5:]))
    whole = rng.uniform(1, 2, (1, 1, Hkv, d)).astype(np.float32)
    assert np.array_equal(append_reference(whole, nan_cache, [1], 1)[0, 0], whole[0, 0])
    # a key lands on its own query's causal position: row L - Nq + i is where decode_reference places query i
    for L in range(Ncap + 1):
        rows = [L - Nq + i for i in range(Nq) if L - Nq + i >= 0]
        marked = append_reference(np.ones((1, Nq, 1, 1), np.float32), np.zeros((1, Ncap, 1, 1), np.float32), [L], Nq)
        assert np.flatnonzero(marked[0, :, 0, 0]).tolist() == rows
