"""Logit soft-capping on the GPU (fa_mi355x_fwd_decode_softcap / _extend_softcap / _ragged_softcap,
include/flash_attn_mi355x_decode_softcap.h) against the fp64 references of tests/test_softcap_cpu.py, which cap BEFORE masking, on the
same (bf16-rounded) inputs at the family's own tolerances (TOL of tests/test_gpu_decode.py: fp32 1e-4, bf16 1e-3 max-abs on out and
lse, the -inf pattern of lse exact; the cap's slope is at most 1, so it amplifies nothing).  Inputs U(-1, 1) with softcap = 0.25, where
the capped and the uncapped reference differ by far more than the tolerance: that is asserted in every parity case, so a kernel that
ignores the cap cannot pass.  The caches are the front of larger NaN-filled buffers, every row at or past a length holds NaN, out and
lse are pre-filled with NaN.  Then saturation (scores far above the cap, and Gemma-2's regime), and the laws that hold bit for bit:
paged against slab, ragged against extend, fused against append-then-attend, softcap = 0 through the new C entry points against the
_window call, roped against apply_rotary, a graphed step against the eager one; and a model on caches with a cap."""
import ctypes
import math

import numpy as np
import pytest

from gpu_util import maxabs, to_np
from test_gpu_decode import TOL, _from_dev, _inputs, _tdt, _to_dev, _torch
from test_gpu_decode_append import _bits, _dev, _stack
from test_gpu_extend import _grouped_inputs, _model_tol
from test_gpu_paged import _dev_table, _pool, _table
from test_gpu_ragged import _cu, _i32, _nan_out, _packed, _rnd
from test_gpu_window import _caches, _nan_like, _new_tokens, _ops, _picked
from test_softcap_cpu import GPU_SPLITS, ragged_softcap_reference, softcap_reference

pytestmark = pytest.mark.gpu

CAP = 0.25
NCAP = 384                                   # three 128-key super tiles
LENS = [0, 1, 127, 128, 129, 300, 9999]      # empty, one key, around a tile edge, several tiles with a partial last one, clamped
H, HKV = 4, 2
MODES = [(True, 0), (True, 100), (False, 0)]   # (causal, window): a window needs the causal mask, a cap does not
COUNTS = [0, 1, 1, 33, 129, 5]               # ragged: no token, one token (twice), part of a block, more than a block
RLENS = [300, 0, 1, 127, 300, 9999]          # ... against these lengths: one token into an empty cache; fewer keys than tokens
TAIL = 3                                     # unused rows behind the last sequence


def _splits(family, B, Nq, Ncap, d, W):
    from flash_attention_minitorch_amd import _lib
    ns = getattr(_lib.decode(), f"fa_mi355x_{family}_window_splits")(B, H, HKV, Nq, Ncap, d, 1, W)
    assert all(p[1] == ns for p in GPU_SPLITS if p[0] == (family, B, H, HKV, Nq, Ncap, d, W))
    return ns


def _kw(W, cap):
    return dict(softcap=cap, **(dict(window=W) if W else {}))


def _discriminates(capped, plain, dtype, what):
    """The condition on the REFERENCES: with and without the cap they differ by at least 10 x TOL in lse and 3 x TOL in out (max over
    the rows of the case), so the tolerance tells a kernel that caps from one that does not."""
    fin = np.isfinite(capped[1])
    assert np.array_equal(fin, np.isfinite(plain[1])) and (~fin).any(), what   # (and the case holds a row with no admissible key)
    dl, do = maxabs(capped[1][fin], plain[1][fin]), maxabs(capped[0], plain[0])
    assert dl >= 10 * TOL[dtype] and do >= 3 * TOL[dtype], (what, dl, do)


def _check_uniform(q, k, v, lens, causal, W, cap, dtype, out, lse, tol=None, discriminate=True):
    """out (B, H, Nq, d), lse (B, H, Nq) against softcap_reference on the picked heads: everything finite but the -inf of the empty
    rows, whose pattern is exact (out = 0 there), the values within the tolerance.  Returns (max error of out, of lse)."""
    B, _, Nq, d = q.shape
    G = H // k.shape[1]
    assert np.all(np.isfinite(out)) and not np.any(np.isnan(lse))
    heads = _picked(H, k.shape[1])
    qs, ks, vs = (np.concatenate([t[b, [h // g for h in heads]] for b in range(B)]) for t, g in ((q, 1), (k, G), (v, G)))
    ls = np.repeat(np.asarray(lens), len(heads))
    ro, rl = softcap_reference(qs, ks, vs, ls, W, 1.0 / math.sqrt(d), cap, causal)
    if discriminate:
        _discriminates((ro, rl), softcap_reference(qs, ks, vs, ls, W, 1.0 / math.sqrt(d), 0.0, causal), dtype, (causal, W, Nq))
    go = np.concatenate([out[b, heads] for b in range(B)])
    gl = np.concatenate([lse[b, heads] for b in range(B)])
    assert np.array_equal(np.isneginf(gl), np.isneginf(rl)), (causal, W, Nq)
    assert not go[np.isneginf(rl)].any()
    fin = np.isfinite(rl)
    eo, el = maxabs(go, ro), maxabs(gl[fin], rl[fin])
    if tol is None:
        assert eo < TOL[dtype] and el < TOL[dtype], (causal, W, Nq, eo, el)
    return eo, el, ro, rl


def _uniform(family, q, k, v, lens, causal, W, cap, layout, dtype):
    torch = _torch()
    B, _, Nq, d = q.shape
    tq = _to_dev(q, layout, d, dtype)
    tk, tv = _caches(k, v, layout, d, dtype)
    out, lse = _nan_like(tq, B, H, Nq)
    got = _ops(family)(tq, tk, tv, _i32(lens), causal=causal, layout=layout, out=out, lse=lse, **_kw(W, cap))
    torch.cuda.synchronize()
    assert got[0] is out and got[1] is lse
    return _from_dev(out, layout), to_np(lse)


def _parity(family, dtype, layout, d, nqs):
    rng = np.random.default_rng(d + (7 if dtype == "bf16" else 0) + len(family) + len(layout))
    seen = set()
    for Nq in nqs:
        for causal, W in MODES:
            seen.add(_splits(family, len(LENS), Nq, NCAP, d, W) > 1)
            q, k, v = _grouped_inputs(rng, dtype, len(LENS), H, HKV, Nq, NCAP, d, LENS)
            out, lse = _uniform(family, q, k, v, LENS, causal, W, CAP, layout, dtype)
            _check_uniform(q, k, v, LENS, causal, W, CAP, dtype, out, lse)
    return seen


@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_decode_softcap_matches_fp64_reference(dtype, layout, d):
    """Nq = 1, 3 and 33 (one lane of a block, a group's rows, two 32-row blocks) at every length of LENS; causal, windowed and
    non-causal; the unwindowed calls run as two splits (the combine launch with tau = 1), the windowed ones of few queries as one."""
    assert _parity("decode", dtype, layout, d, (1, 3, 33)) == {True, False}


@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_extend_softcap_matches_fp64_reference(dtype, layout, d):
    """Nq = 129 and 130: G * Nq = 258 and 260 rows per kv head, three 128-row blocks with a last one of 2 and 4 rows; every call runs
    as two splits (the one-split extend build is held bit for bit against the ragged call below, which is held against this)."""
    assert _parity("extend", dtype, layout, d, (129, 130)) == {True}


def _ragged_case(rng, dtype, counts, lens, Ncap, d, tail=0):
    q = _rnd(rng, dtype, (sum(counts) + tail, H, d))
    _, k, v = _inputs(rng, dtype, len(counts), HKV, 1, Ncap, d, lens)
    return q, k, v, _cu(counts)


def _check_ragged(q, k, v, cu, lens, causal, W, cap, dtype, out, lse):
    out, lse = to_np(out), to_np(lse)
    scale = 1.0 / math.sqrt(q.shape[2])
    ro, rl = ragged_softcap_reference(q, k, v, cu, lens, W, scale, cap, causal)
    owned = ~np.isnan(rl[0])
    assert owned.sum() == int(cu[-1]) - int(cu[0])
    po, pl = ragged_softcap_reference(q, k, v, cu, lens, W, scale, 0.0, causal)
    _discriminates((ro[owned], rl[:, owned]), (po[owned], pl[:, owned]), dtype, (causal, W))
    assert np.all(np.isnan(out[~owned])) and np.all(np.isnan(lse[:, ~owned]))   # (the unused tail keeps its NaN)
    assert np.all(np.isfinite(out[owned])) and not np.any(np.isnan(lse[:, owned]))
    assert np.array_equal(np.isneginf(lse[:, owned]), np.isneginf(rl[:, owned]))
    fin = np.isfinite(rl)
    assert not out[owned][np.isneginf(rl[:, owned]).T].any()
    assert maxabs(out[owned], ro[owned]) < TOL[dtype], (causal, W, maxabs(out[owned], ro[owned]))
    assert maxabs(lse[fin], rl[fin]) < TOL[dtype], (causal, W, maxabs(lse[fin], rl[fin]))


@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_ragged_softcap_matches_fp64_reference(dtype, layout, d):
    """Counts 0, 1, 1, 33, 129, 5 with three unused tail rows: two splits, so the ragged combine instance with tau = 1."""
    torch = _torch()
    rng = np.random.default_rng(d + (11 if dtype == "bf16" else 0) + len(layout))
    for causal, W in MODES:
        q, k, v, cu = _ragged_case(rng, dtype, COUNTS, RLENS, NCAP, d, tail=TAIL)
        T = q.shape[0]
        assert _splits("ragged", len(COUNTS), T, NCAP, d, W) >= 2
        tk, tv = _caches(k, v, layout, d, dtype)
        out, lse = _nan_out(T, H, d)
        _ops("ragged")(_packed(q, dtype), tk, tv, _i32(cu), _i32(RLENS), causal=causal, layout=layout, out=out, lse=lse, **_kw(W, CAP))
        torch.cuda.synchronize()
        _check_ragged(q, k, v, cu, RLENS, causal, W, CAP, dtype, out, lse)


# ---- saturation ----

@pytest.mark.parametrize("amp,cap", [(64.0, 0.5), (16.0, 50.0)], ids=["x64-cap0.5", "x16-cap50"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_softcap_saturates_cleanly(dtype, amp, cap):
    """q x 64 (exact in bf16) with softcap = 0.5: tau * q.k / softcap reaches hundreds, the exp2 argument overflows and nearly every
    logit sits at +-softcap.  q x 16 with softcap = 50: Gemma-2's regime, logits of tens, the cap nearly linear.  out and lse stay
    finite and inside the project's large-magnitude envelope, 5e-3 x the tensor's scale (README "Accuracy envelope").  Measured
    maxima: profiles/softcap_accuracy.txt."""
    rng = np.random.default_rng(int(amp) + (3 if dtype == "bf16" else 0))
    d = 64
    for family, Nq in (("decode", 3), ("decode", 33), ("extend", 130)):
        for causal, W in MODES:
            q, k, v = _grouped_inputs(rng, dtype, len(LENS), H, HKV, Nq, NCAP, d, LENS)
            q = q * np.float32(amp)
            smax = float(np.nanmax(np.abs(np.einsum("bhid,bhjd->bhij", q[:, ::2], np.nan_to_num(k))))) / math.sqrt(d)
            assert smax / cap > (100 if cap < 1 else 0.2)
            out, lse = _uniform(family, q, k, v, LENS, causal, W, cap, "bnhd", dtype)
            eo, el, ro, rl = _check_uniform(q, k, v, LENS, causal, W, cap, dtype, out, lse, tol=5e-3, discriminate=False)
            so, sl = max(1.0, float(np.max(np.abs(ro)))), max(1.0, float(np.max(np.abs(rl[np.isfinite(rl)]))))
            print(f"softcap_accuracy {dtype} amp={amp:g} cap={cap:g} {family} Nq={Nq} causal={int(causal)} W={W}: "
                  f"max|tau*s|/cap={smax / cap:.1f} out {eo:.3e} (scale {so:.2f}) lse {el:.3e} (scale {sl:.2f})")
            assert eo < 5e-3 * so and el < 5e-3 * sl, (family, Nq, causal, W, eo, el)


# ---- bit for bit ----

def _same(a, b):
    return bool(_torch().equal(_bits(a), _bits(b)))


def _family_case(rng, dtype, family, layout, lens, Ncap, d, counts=None, Nq=None):
    """(device q, the arguments between the caches and the keywords, numpy k and v, the counts)."""
    if family == "ragged":
        q, k, v, cu = _ragged_case(rng, dtype, counts, lens, Ncap, d)
        return _packed(q, dtype), (_i32(cu), _i32(lens)), k, v, counts
    q, k, v = _grouped_inputs(rng, dtype, len(lens), H, HKV, Nq, Ncap, d, lens)
    return _to_dev(q, layout, d, dtype), (_i32(lens),), k, v, [Nq] * len(lens)


@pytest.mark.parametrize("permuted", [False, True], ids=["identity", "permuted"])
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_paged_softcap_returns_the_slab_bits(dtype, layout, permuted):
    torch = _torch()
    rng = np.random.default_rng(128 + permuted + len(layout))
    d, ps = 64, 128
    mp = NCAP // ps
    for family, Nq in (("decode", 1), ("decode", 33), ("extend", 130), ("ragged", None)):
        lens = RLENS if family == "ragged" else LENS
        tq, head, k, v, _ = _family_case(rng, dtype, family, layout, lens, NCAP, d, COUNTS, Nq)
        tk, tv = (_to_dev(t, layout, d, dtype) for t in (k, v))
        table, num_pages = _table(rng, len(lens), NCAP, ps, lens)
        if not permuted:
            table = np.arange(len(lens) * mp, dtype=np.int32).reshape(len(lens), mp)
        (kp, _), (vp, _) = (_pool(t, layout, ps, table, num_pages, None if not permuted else lens) for t in (tk, tv))
        for causal, W in MODES:
            want = _ops(family)(tq, tk, tv, *head, causal=causal, layout=layout, **_kw(W, CAP))
            got = _ops(family)(tq, kp, vp, *head, causal=causal, layout=layout, block_table=_dev_table(table), **_kw(W, CAP))
            torch.cuda.synchronize()
            assert _same(got[0], want[0]) and _same(got[1], want[1]), (family, Nq, causal, W)
            assert not bool(torch.isnan(got[0]).any())


@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_ragged_softcap_is_the_extend_softcap_call_on_each_sequence_alone(dtype, layout):
    """A cache of 256 rows is one split under both policies (pinned in tests/test_softcap_cpu.py): the same bits per sequence."""
    rng = np.random.default_rng(43)
    d, Ncap, counts, lens = 64, 256, [0, 1, 33, 129, 5, 1], [100, 1, 256, 129, 9999, 0]
    T = sum(counts)
    for causal, W in MODES:
        assert _splits("ragged", len(counts), T, Ncap, d, W) == 1
        q, k, v, cu = _ragged_case(rng, dtype, counts, lens, Ncap, d)
        tq, (tk, tv), tl = _packed(q, dtype), _caches(k, v, layout, d, dtype), _i32(lens)
        out, lse = _nan_out(T, H, d)
        _ops("ragged")(tq, tk, tv, _i32(cu), tl, causal=causal, layout=layout, out=out, lse=lse, **_kw(W, CAP))
        for b, nq in enumerate(counts):
            if nq == 0:
                continue
            s = int(cu[b])
            qb = tq[s:s + nq][None]
            if layout == "bhnd":
                qb = qb.transpose(1, 2).contiguous()
            assert _splits("extend", 1, nq, Ncap, d, W) == 1
            o, l = _ops("extend")(qb, tk[b:b + 1], tv[b:b + 1], tl[b:b + 1], causal=causal, layout=layout, **_kw(W, CAP))
            o = (o[0] if layout == "bnhd" else o[0].transpose(0, 1)).contiguous()
            assert _same(out[s:s + nq], o) and _same(lse[:, s:s + nq].contiguous(), l[0].contiguous()), (b, causal, W)
        _check_ragged(q, k, v, cu, lens, causal, W, CAP, dtype, out, lse)


@pytest.mark.parametrize("paged", [False, True], ids=["slab", "paged"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_fused_softcap_call_is_the_append_then_the_softcap_call(dtype, paged):
    """The rows the append writes hold NaN before it: the fused call returns the bits of append-then-attend, out and lse, and leaves
    the whole caches as the plain append leaves them."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    rng = np.random.default_rng(19 + paged)
    d, ps = 64, 128
    appends = {"decode": device_ops.decode_append, "extend": device_ops.extend_append, "ragged": device_ops.ragged_append}
    for family, Nq in (("decode", 3), ("extend", 130), ("ragged", None)):
        lens = RLENS if family == "ragged" else LENS
        tq, head, k, v, counts = _family_case(rng, dtype, family, "bnhd", lens, NCAP, d, COUNTS, Nq)
        if family == "ragged":
            kn, vn = (_packed(_new_tokens(rng, dtype, (sum(counts), HKV, d)), dtype) for _ in range(2))
        else:
            kn, vn = (_dev(_new_tokens(rng, dtype, (len(lens), Nq, HKV, d)), "bnhd", dtype) for _ in range(2))
        for b, (n, nq) in enumerate(zip(lens, counts)):   # the new tokens' rows are not there yet
            n = min(max(n, 0), NCAP)
            k[b, :, max(n - nq, 0):n] = np.nan
            v[b, :, max(n - nq, 0):n] = np.nan
        tk, tv = (_to_dev(t, "bnhd", d, dtype) for t in (k, v))
        kw = {}
        if paged:
            table, num_pages = _table(rng, len(lens), NCAP, ps, lens)
            (tk, _), (tv, _) = (_pool(t, "bnhd", ps, table, num_pages, lens) for t in (tk, tv))
            kw = dict(block_table=_dev_table(table))
        for causal, W in MODES:
            k1, v1, k2, v2 = tk.clone(), tv.clone(), tk.clone(), tv.clone()
            appends[family](kn, vn, k1, v1, *head, **kw)
            o1, l1 = _ops(family)(tq, k1, v1, *head, causal=causal, **_kw(W, CAP), **kw)
            o2, l2 = _ops(family)(tq, k2, v2, *head, causal=causal, k_new=kn, v_new=vn, **_kw(W, CAP), **kw)
            torch.cuda.synchronize()
            for a, b in ((o1, o2), (l1, l2), (k1, k2), (v1, v2)):
                assert _same(a, b), (family, causal, W)
            assert not _same(k2, tk) and not bool(torch.isnan(o2).any())


def _c_call(family, tq, tk, tv, head, Nq, Ncap, d, causal, W, cap, dtype, ws):
    """The softcap C entry point itself, attend only on slab caches ("bnhd"), into fresh NaN-filled out and lse."""
    torch = _torch()
    from flash_attention_minitorch_amd import _lib
    B = tk.shape[0]
    out = torch.full(tq.shape, float("nan"), dtype=torch.float32, device="cuda")
    lse = torch.full((H, Nq) if family == "ragged" else (B, H, Nq), float("nan"), dtype=torch.float32, device="cuda")
    p = lambda t: ctypes.c_void_p(None if t is None else t.data_ptr())
    args = [p(tq), None, None, p(tk), p(tv), p(out), p(lse)] + [p(t) for t in head] + [None, p(ws), B, H, HKV, Nq, Ncap, 0, 0, 0, d, d,
                                                                                       _lib.FA_LAYOUT_BNHD, 0.0, int(causal), W, cap,
                                                                                       _lib.FA_DTYPE_BF16 if dtype == "bf16" else _lib.FA_DTYPE_F32,
                                                                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)]
    _lib.decode_check(getattr(_lib.decode(), f"fa_mi355x_fwd_{family}_softcap")(*args))
    torch.cuda.synchronize()
    return out, lse


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_softcap_zero_through_the_new_entry_points_is_the_window_call(dtype):
    """softcap = 0 is the _window call exactly (the same launches, splits, workspace and bits); and the entry point with a cap is
    what device_ops calls."""
    from flash_attention_minitorch_amd import device_ops
    rng = np.random.default_rng(77)
    d = 64
    sizes = {"decode": device_ops.decode_workspace, "extend": device_ops.extend_workspace, "ragged": device_ops.ragged_workspace}
    for family, Nq in (("decode", 3), ("extend", 130), ("ragged", None)):
        lens = RLENS if family == "ragged" else LENS
        tq, head, k, v, counts = _family_case(rng, dtype, family, "bnhd", lens, NCAP, d, COUNTS, Nq)
        n = tq.shape[0] if family == "ragged" else Nq
        tk, tv = (_to_dev(t, "bnhd", d, dtype) for t in (k, v))
        for W in (0, 100):
            ws = sizes[family](tq, tk, *head[:-1], window=W)
            want = _ops(family)(tq, tk, tv, *head, causal=True, window=W)   # (window = 0 included: the _window symbol)
            got = _c_call(family, tq, tk, tv, head, n, NCAP, d, True, W, 0.0, dtype, ws)
            assert _same(got[0], want[0]) and _same(got[1], want[1]), (family, W)
            capped = _ops(family)(tq, tk, tv, *head, causal=True, **_kw(W, CAP))
            got = _c_call(family, tq, tk, tv, head, n, NCAP, d, True, W, CAP, dtype, ws)
            assert _same(got[0], capped[0]) and _same(got[1], capped[1]) and not _same(capped[1], want[1]), (family, W)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_roped_softcap_call_is_the_softcap_call_on_rotated_q_and_k_new(dtype):
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    rng = np.random.default_rng(5)
    d, lens = 64, [3, 127, 128, 129, 300, 9999]
    cos, sin = device_ops.rotary_table(NCAP, 32, device="cuda")
    for family, Nq in (("decode", 3), ("extend", 130)):
        lens_f = [max(n, Nq) for n in lens]
        tq, head, k, v, _ = _family_case(rng, dtype, family, "bnhd", lens_f, NCAP, d, None, Nq)
        kn, vn = (_dev(_new_tokens(rng, dtype, (len(lens), Nq, HKV, d)), "bnhd", dtype) for _ in range(2))
        tk, tv = (_to_dev(np.nan_to_num(t), "bnhd", d, dtype) for t in (k, v))
        offs = head[0].clamp(0, NCAP) - Nq
        qa, ka = (device_ops.apply_rotary(t, cos, sin, offs) for t in (tq, kn))
        for W in (0, 100):
            k1, v1, k2, v2 = tk.clone(), tv.clone(), tk.clone(), tv.clone()
            o1, l1 = _ops(family)(qa, k1, v1, *head, causal=True, k_new=ka, v_new=vn, **_kw(W, CAP))
            o2, l2 = _ops(family)(tq, k2, v2, *head, causal=True, k_new=kn, v_new=vn, rotary_cos=cos, rotary_sin=sin, **_kw(W, CAP))
            torch.cuda.synchronize()
            for a, b in ((o1, o2), (l1, l2), (k1, k2), (v1, v2)):
                assert _same(a, b), (family, W)
            assert not _same(qa, tq) and not bool(torch.isnan(o2).any())


# ---- the model ----

def _dense_softcap_stack(x, layers, n_head, W, cap):
    """The stack with its attention recomputed densely in torch fp32: the scores of all N x N pairs, capped, then the causal (and
    window) mask; projections and the residual as modules_transformer makes them."""
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    B, N, E = x.shape
    i = torch.arange(N, device=x.device)
    ok = i[None, :] <= i[:, None]
    if W:
        ok &= i[None, :] > i[:, None] - W
    for wq, wk, wv, wo in layers:
        q, k, v = mt._project(x, wq, wk, wv, n_head)
        G = n_head // k.shape[2]
        qf, kf, vf = (t.float().permute(0, 2, 1, 3) for t in (q, k.repeat_interleave(G, 2), v.repeat_interleave(G, 2)))
        s = cap * torch.tanh((qf @ kf.transpose(2, 3)) * q.shape[3] ** -0.5 / cap)
        p = torch.softmax(s.masked_fill(~ok, float("-inf")), dim=-1)
        o = (p @ vf).permute(0, 2, 1, 3)
        x = x + (o.reshape(B * N, E).to(x.dtype) @ wo).view(B, N, E)
    return x


@pytest.mark.parametrize("paged", [False, True], ids=["slab", "paged-window"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_model_on_a_capped_cache_matches_the_dense_capped_stack(dtype, paged):
    """260 tokens through a 2-layer stack on KVCache(softcap=) and on PagedKVCache(window=, softcap=): a prompt of 150 (the extend
    path: the square forward has no cap), 100 more at once (the fused decode step), a ragged step, then single steps.  The cap is
    0.5, inside the stack's scores: in fp32 the uncapped stack is many tolerances away from the capped one (asserted).  The bf16
    model tolerance is wider than the cap's effect on these activations; there the kernels are held by the parity tests above."""
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    E, L, B, N, W, cap = 128, 2, 2, 260, 160 if paged else 0, 0.5
    x, layers = _stack(np.random.default_rng(E + paged), dtype, B, E, H, HKV, L, N)
    want = to_np(_dense_softcap_stack(x, layers, H, W, cap))
    tol = _model_tol(dtype, want)
    if dtype == "f32":
        assert maxabs(want, to_np(_dense_softcap_stack(x, layers, H, W, 1e4))) > 5 * tol   # (the cap matters at this tolerance)
    if paged:
        cache = mt.PagedKVCache(L, B, 384, H, E // H, _tdt(dtype), "cuda", n_kv_head=HKV, page_size=128, window=W, softcap=cap)
    else:
        cache = mt.KVCache(L, B, 384, H, E // H, _tdt(dtype), "cuda", n_kv_head=HKV, softcap=cap)
    got = [mt.attention_stack_prefill(x[:, :150].contiguous(), layers, H, cache),
           mt.attention_stack_extend(x[:, 150:250].contiguous(), layers, H, cache)]
    packed = torch.cat([x[0, 250:253], x[1, 250:253]]).contiguous()
    r = mt.attention_stack_ragged(packed, [3, 3], layers, H, cache)
    got.append(torch.stack([r[:3], r[3:6]]))
    for n in range(253, N):
        got.append(mt.attention_stack_step_fused(x[:, n:n + 1].contiguous(), layers, H, cache))
    assert cache.lengths.tolist() == [N] * B
    got = to_np(torch.cat(got, dim=1))
    assert maxabs(got, want) < tol, (maxabs(got, want), tol)


def test_graphed_step_on_a_capped_cache_replays_the_eager_fused_step_bit_for_bit():
    torch = _torch()
    from flash_attention_minitorch_amd import modules_transformer as mt
    dtype, E, L, B, P, S, cap = "bf16", 128, 2, 2, 250, 6, 0.5
    x, layers = _stack(np.random.default_rng(31), dtype, B, E, H, HKV, L, P + S)
    assert _splits("decode", B, 1, 1024, E // H, 0) == 4   # (the steps run as four splits: the combine with tau = 1 is in the graph)
    caches = [mt.KVCache(L, B, 1024, H, E // H, _tdt(dtype), "cuda", n_kv_head=HKV, softcap=cap) for _ in range(2)]
    plain = mt.KVCache(L, B, 1024, H, E // H, _tdt(dtype), "cuda", n_kv_head=HKV)
    for c in caches + [plain]:
        mt.attention_stack_prefill(x[:, :P].contiguous(), layers, H, c)
    graphed = mt.GraphedStep(layers, H, caches[0], T=1)
    for n in range(P, P + S):
        a = graphed.step(x[:, n:n + 1].contiguous()).clone()
        b = mt.attention_stack_step_fused(x[:, n:n + 1].contiguous(), layers, H, caches[1])
        c = mt.attention_stack_step_fused(x[:, n:n + 1].contiguous(), layers, H, plain)
        torch.cuda.synchronize()
        assert _same(a, b) and not _same(b, c), n
    assert caches[0].lengths.tolist() == caches[1].lengths.tolist() == [P + S] * B
    for li in range(L):
        assert _same(caches[0].k[li], caches[1].k[li]) and _same(caches[0].v[li], caches[1].v[li])
