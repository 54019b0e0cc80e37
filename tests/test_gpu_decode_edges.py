"""The paths and edges of KV-cache decode (csrc/fa_decode.h, csrc/fa_decode.hip) that tests/test_gpu_decode.py and
tests/test_gpu_decode_gqa.py do not reach, each against the fp64 decode reference of tests/test_decode_cpu.py on the same
(bf16-rounded) inputs with NaN past every valid length, out and lse at TOL of tests/test_gpu_decode.py, the same -inf pattern in lse
and out = 0 on rows without an admissible key.  Every shape asserts its split count, so a change of the split policy cannot move a
case onto another path unseen (tests/test_decode_cpu.py holds the same counts wherever the library builds):
the one-split result path (short caches of one chunk; chunks of six super tiles, ungrouped and grouped); long chunks over eight
splits in the ungrouped build; a grid of lengths on and next to every wave, super-tile and chunk boundary; group sizes 3, 5, 6, 7,
12, 71 and, at the far end of row_query's range, 4096; scores that are steep by construction (the running maximum moves with every
tile, alpha and the wave / split weights underflow); hostile caller buffers (NaN, oversized and stale workspaces, lse = NULL,
caller-supplied out / lse through the unpad path); and a batch element just under 2 GiB with rows at byte offset 2^30 and next to
2^31.  profiles/decode_edges.txt: which of eight arithmetic mutations of the kernels each test catches."""
import math

import numpy as np
import pytest

import oracle
from gpu_util import maxabs, rand_u, to_np
from test_gpu_decode import LENS, TOL, _check, _decode, _from_dev, _inputs, _to_dev, _torch
from test_gpu_decode_gqa import _check_grouped, _raw
from test_gpu_decode_gqa import _decode as _decode_gqa
from test_gpu_decode_gqa import _inputs as _inputs_gqa

pytestmark = pytest.mark.gpu


def _splits(B, H, Hkv, Nq, Ncap, d, dtype):
    from flash_attention_minitorch_amd import _lib
    lib, code = _lib.decode(), 1 if dtype == "bf16" else 0
    ns = lib.fa_mi355x_decode_splits_gqa(B, H, Hkv, Nq, Ncap, d, code)
    if H == Hkv:
        assert ns == lib.fa_mi355x_decode_splits(B, H, Nq, Ncap, d, code)
    return ns


def _call(tq, tk, tv, lens, causal, layout, scale=None, **kw):
    """flash_attn_decode on device tensors (so that one upload of a large cache serves several calls); numpy (B, H, Nq, d), lse."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    tl = None if lens is None else torch.tensor(lens, dtype=torch.int32, device="cuda")
    out, lse = device_ops.flash_attn_decode(tq, tk, tv, tl, causal=causal, softmax_scale=scale, layout=layout, **kw)
    torch.cuda.synchronize()
    return _from_dev(out, layout), to_np(lse)


def _dead_rows_are_zero(out, lse):
    assert np.all(out[np.isneginf(lse)] == 0)


# ---------------------------------------------------------------------------------------------------------------- A. one split

@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_one_split_short_caches_match_fp64_reference(dtype, layout, d):
    """A cache of one chunk: the split kernel writes out = O / l and lse = m tau + ln l itself.  Ncap = 100: one super tile, wave 3
    holds no key; 200: a ragged second super tile; 256: exactly full."""
    rng = np.random.default_rng(100 + d + (7 if dtype == "bf16" else 0))
    B, H = 3, 2
    for Ncap in (100, 200, 256):
        for Nq in (1, 3, 33):
            assert _splits(B, H, H, Nq, Ncap, d, dtype) == 1
            for lens in ([Ncap, 1, 0], [Nq - 1, Ncap - 1, Ncap]):
                for causal in (True, False):
                    q, k, v = _inputs(rng, dtype, B, H, Nq, Ncap, d, lens)
                    out, lse = _decode(q, k, v, lens, causal, layout, dtype, d, d)
                    _check(q, k, v, lens, causal, dtype, out, lse)
                    _dead_rows_are_zero(out, lse)


LONG_LENS = [700, 699, 641, 640, 513, 512, 385, 129, 128, 127, 1, 0]


@pytest.mark.parametrize("dtype,d", [("f32", 64), ("bf16", 64), ("bf16", 128)])
def test_one_split_over_six_super_tiles_ungrouped(dtype, d):
    """B * H = 1024 workgroups already: chunk = 768 = Ncap's six super tiles (the last one ragged) in ONE split, the serving shape.
    The register-staged prefetch reaches its steady state, and the G = 1 build's one-split epilogue meets the reference."""
    B, H, Ncap = 128, 8, 700
    assert _splits(B, H, H, 1, Ncap, d, dtype) == 1 and _splits(B, H, H, 3, Ncap, d, dtype) == 1
    rng = np.random.default_rng(200 + d + (7 if dtype == "bf16" else 0))
    lens = [LONG_LENS[b % len(LONG_LENS)] for b in range(B)]
    q3, k, v = _inputs_gqa(rng, dtype, B, H, H, 3, Ncap, d, lens, coarse=True)
    q1 = np.ascontiguousarray(q3[:, :, 2:])
    for layout in ("bnhd", "bhnd"):
        tk, tv = (_to_dev(t, layout, d, dtype) for t in (k, v))
        for q, causal in ((q1, False), (q1, True), (q3, True)):
            out, lse = _call(_to_dev(q, layout, d, dtype), tk, tv, lens, causal, layout)
            _check(q, k, v, lens, causal, dtype, out, lse)
            _dead_rows_are_zero(out, lse)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_one_split_over_six_super_tiles_grouped(dtype):
    """The same one chunk of six super tiles in the G > 1 build: 32 heads on 8 kv heads, 1024 workgroups of one live row block, the
    one-split epilogue writing out and lse by query head.  Every head of every call is compared."""
    B, H, Hkv, Nq, Ncap, d = 128, 32, 8, 1, 700, 64
    assert _splits(B, H, Hkv, Nq, Ncap, d, dtype) == 1
    rng = np.random.default_rng(300 + (7 if dtype == "bf16" else 0))
    lens = [LONG_LENS[b % len(LONG_LENS)] for b in range(B)]
    q, k, v = _inputs_gqa(rng, dtype, B, H, Hkv, Nq, Ncap, d, lens, coarse=True)
    for layout, causal in (("bnhd", True), ("bhnd", False), ("bnhd", False), ("bhnd", True)):
        tq, tk, tv = (_to_dev(t, layout, d, dtype) for t in (q, k, v))
        out, lse = _call(tq, tk, tv, lens, causal, layout)
        _check_grouped(q, k, v, lens, causal, dtype, out, lse)
        _dead_rows_are_zero(out, lse)


# ------------------------------------------------------------------------------------ B. long chunks over several splits, G = 1

B_LENS = [1024, 2048, 8192, 1025, 1023, 1030, 5000, 8191, 1, 0, 3333, 7777, 4097, 6001, 2047, 7169]


@pytest.mark.parametrize("dtype,d", [("bf16", 128), ("f32", 64)])
def test_chunks_of_eight_super_tiles_over_eight_splits_ungrouped(dtype, d):
    """chunk = 1024: eight super tiles per workgroup in the G = 1 build, lengths on, one before and one past a chunk boundary, inside
    a chunk's first super tile, and whole chunks empty."""
    B, H, Ncap = 16, 8, 8192
    assert all(n % 32 for n in B_LENS[10:])
    assert _splits(B, H, H, 1, Ncap, d, dtype) == 8
    ns5 = _splits(B, H, H, 5, Ncap, d, dtype)
    chunk5 = -(-(-(-Ncap // ns5)) // 256) * 256   # ceil(Ncap / nsplit) rounded up to the policy's multiple of 256 keys
    assert ns5 == 8 and chunk5 == 1024 and chunk5 > 256
    rng = np.random.default_rng(400 + d)
    q5, k, v = _inputs_gqa(rng, dtype, B, H, H, 5, Ncap, d, B_LENS, coarse=True)
    q1 = np.ascontiguousarray(q5[:, :, 4:])
    tk, tv = (_to_dev(t, "bnhd", d, dtype) for t in (k, v))
    for q, causal in ((q1, True), (q1, False), (q5, True)):
        out, lse = _call(_to_dev(q, "bnhd", d, dtype), tk, tv, B_LENS, causal, "bnhd")
        _check(q, k, v, B_LENS, causal, dtype, out, lse)
        _dead_rows_are_zero(out, lse)


# -------------------------------------------------------------------------------------------------------- C. length boundaries

C_LENS = [0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512, 513, 767, 768, 769, 1023, 1024,
          1025, 1279, 1280, 1281, 1299, 1300, 1301, -1, 640, 641, 96, 97, 160, 1152]


def _length_grid(dtype, d, Nq, causals):
    B, H, Ncap = len(C_LENS), 2, 1300
    assert B == 40 and _splits(B, H, H, Nq, Ncap, d, dtype) == 6
    rng = np.random.default_rng(500 + 10 * Nq + d + (7 if dtype == "bf16" else 0))
    q, k, v = _inputs(rng, dtype, B, H, Nq, Ncap, d, C_LENS)
    for causal in causals:
        layout = "bnhd" if causal else "bhnd"
        out, lse = _decode(q, k, v, C_LENS, causal, layout, dtype, d, d)
        _check(q, k, v, C_LENS, causal, dtype, out, lse)
        _dead_rows_are_zero(out, lse)
        assert np.all(out[0] == 0) and np.all(out[33] == 0)   # len = 0 and len = -1


@pytest.mark.parametrize("Nq", [1, 3, 32, 33])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_lengths_on_and_next_to_wave_tile_and_chunk_boundaries(dtype, Nq):
    """Forty lengths in one call: 32 k, 128 k and 256 k with both neighbours, 0, 1, Ncap and the two out-of-range values, over six
    chunks of 256 keys.  Where c1, kbase + 32 > c1 and the empty partial (m = -inf, l = 0) change behaviour."""
    _length_grid(dtype, 64, Nq, (True, False))


@pytest.mark.parametrize("d", [32, 128])
def test_length_grid_at_the_other_head_dims(d):
    """The same forty lengths through the d = 32 and d = 128 builds (other tile images and staging maps), Nq = 33: two row blocks,
    dead rows wherever the length is below 33."""
    _length_grid("bf16", d, 33, (True,))


# ------------------------------------------------------------------------------------------------------------ D. group sizes

ODD_GROUPS = [(6, 2), (10, 2), (12, 2), (28, 4), (24, 2), (71, 1)]


def _odd_group(dtype, layout, d, H, Hkv, nqs):
    B, Ncap = len(LENS), 520
    rng = np.random.default_rng(600 + 10 * H + Hkv + d + (7 if dtype == "bf16" else 0))
    for Nq in nqs:
        # (G = 7 at Nq = 128 has 672 workgroups per split: two chunks of 512)
        assert _splits(B, H, Hkv, Nq, Ncap, d, dtype) == (2 if Nq == 128 else 3)
        for causal in (True, False):
            q, k, v = _inputs_gqa(rng, dtype, B, H, Hkv, Nq, Ncap, d, LENS)
            out, lse = _decode_gqa(q, k, v, LENS, causal, layout, dtype, d, d, nan_buffers=True)
            _check_grouped(q, k, v, LENS, causal, dtype, out, lse)
            _dead_rows_are_zero(out, lse)


@pytest.mark.parametrize("heads", ODD_GROUPS, ids=lambda t: f"G{t[0] // t[1]}")
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_group_sizes_that_are_no_power_of_two(dtype, layout, heads):
    """G = 3, 5, 6, 7, 12, 71 with Nq = 1, 5, 11: G * Nq is no multiple of 32, a query's heads straddle row blocks, and at G = 71 the
    heads of ONE query span three row blocks.  row_query's reciprocal, pos_lo / pos_hi and the head index on the device."""
    H, Hkv = heads
    _odd_group(dtype, layout, 64, H, Hkv, (1, 5, 11) + ((128,) if H // Hkv == 7 else ()))


@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
def test_multi_query_group_of_71_heads_at_d128(layout):
    """G = 71 through the d = 128 bf16 build of the grouped kernel (one workgroup per CU: the largest tile images)."""
    _odd_group("bf16", layout, 128, 71, 1, (1, 5, 11))


def test_row_query_at_the_far_end_of_its_range():
    """G = 4096 heads on one kv head at Nq = 128: 2^19 rows, where a float reciprocal without row_query's remainder correction is
    first off by one (rho / G with 0.5 / G below the product's rounding).  Causal, so a query index that is one too small sees one
    key fewer.  One split.  out and lse are the fronts of larger NaN-filled buffers whose tails must come back untouched: a quotient
    that is one too small turns (query i, head 0) into (query i - 1, head G), which in [B][Nq][H][d] is the same q and out address but
    in lse [B][H][Nq] lies up to Nq - 1 entries past the end.  With 4096 entries of slack, a kernel that is wrong in this way (the
    row_query mutation of profiles/decode_edges.txt) still writes inside this test's own allocations."""
    torch = _torch()
    B, H, Hkv, Nq, Ncap, d = 1, 4096, 1, 128, 64, 32
    assert _splits(B, H, Hkv, Nq, Ncap, d, "f32") == 1
    rng = np.random.default_rng(650)
    q, k, v = _inputs_gqa(rng, "f32", B, H, Hkv, Nq, Ncap, d, [Ncap])
    tq, tk, tv = (_to_dev(t, "bnhd", d, "f32") for t in (q, k, v))
    slack = 4096
    obuf = torch.full((tq.numel() + slack,), float("nan"), dtype=torch.float32, device="cuda")
    lbuf = torch.full((B * H * Nq + slack,), float("nan"), dtype=torch.float32, device="cuda")
    out, lse = obuf[:tq.numel()].view(tq.shape), lbuf[:B * H * Nq].view(B, H, Nq)
    _raw("fa_mi355x_fwd_decode_gqa", (H, Hkv), tq, tk, tv, None, None, B, Nq, Ncap, d, "bnhd", True, "f32", out=out, lse=lse)
    assert bool(torch.isnan(obuf[tq.numel():]).all()) and bool(torch.isnan(lbuf[B * H * Nq:]).all())
    out, lse = _from_dev(out, "bnhd"), to_np(lse)
    _check_grouped(q, k, v, [Ncap], True, "f32", out, lse)
    _dead_rows_are_zero(out, lse)


# ------------------------------------------------------------------------------------------------------------ E. steep scores

def _sixteenths(rng, shape, lo, hi):
    """Multiples of 2^-4 in [lo, hi]: exact in bf16 (and their products with one such factor exact in fp32)."""
    return (rng.integers(int(lo * 16), int(hi * 16) + 1, shape) / 16.0).astype(np.float32)


def _steep_inputs(rng, kind, B, H, Nq, Ncap, d, lens, spike_at=None):
    """Scores known by construction: q is zero but for column col(h), value a_i = 8 - (i % 4) / 2; k's column col(h) holds the ramp
    or the spike over the key index, its other columns and v hold multiples of 2^-4 in [-1, 1].  Returns (q, k, v, softmax_scale);
    score(i, j) = scale * a_i * k[j, col] exactly."""
    q = np.zeros((B, H, Nq, d), np.float32)
    k = _sixteenths(rng, (B, H, Ncap, d), -1, 1)
    v = _sixteenths(rng, (B, H, Ncap, d), -1, 1)
    j = np.arange(Ncap)
    if kind == "up":
        col, scale = np.round((-8 + 16 * j / (Ncap - 1)) * 16) / 16, 60.0 / 64
    elif kind == "down":
        col, scale = np.round((8 - 16 * j / (Ncap - 1)) * 16) / 16, 60.0 / 64
    else:
        col, scale = -8 + _sixteenths(rng, (Ncap,), 0, 0.5), 40.0 / 64
        col[spike_at] = 8
    for h in range(H):
        c = 5 + 16 * h
        q[:, h, :, c] = 8 - (np.arange(Nq) % 4) / 2
        k[:, h, :, c] = col
    assert np.array_equal(oracle.bf16_round(q), q) and np.array_equal(oracle.bf16_round(k), k) and np.array_equal(oracle.bf16_round(v), v)
    for b, n in enumerate(lens):
        k[b, :, n:] = np.nan
        v[b, :, n:] = np.nan
    return q, k, v, scale


def _steep(dtype, kind, Ncap, spikes=(None,)):
    B, H, d = 2, 2, 64
    lens = [Ncap, Ncap - 40]
    rng = np.random.default_rng(700 + Ncap)
    for Nq in (1, 33):
        ns = _splits(B, H, H, Nq, Ncap, d, dtype)
        assert (ns == 1) if Ncap == 256 else (ns == 6)
        for spike_at in spikes:
            q, k, v, scale = _steep_inputs(rng, kind, B, H, Nq, Ncap, d, lens, spike_at)
            for causal in (True, False):
                out, lse = _decode(q, k, v, lens, causal, "bnhd", dtype, d, d, scale=scale)
                _check(q, k, v, lens, causal, dtype, out, lse, scale=scale)
                # the construction did what it is for: the row maxima span the range, a ramp's far end weighs nothing
                fin = np.isfinite(lse)
                assert fin.any() and np.max(np.abs(lse[fin])) > 25


@pytest.mark.parametrize("Ncap", [256, 1300])
@pytest.mark.parametrize("kind", ["up", "down"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_steep_score_ramps(dtype, kind, Ncap):
    """Scores from -60 to +60 (natural-log units after the scale) over the cache.  Ascending: every tile raises the running maximum,
    alpha underflows for the early tiles, the last wave and the last split own the result.  Descending: the first tile owns it and
    every later weight is tiny or 0.  One split (Ncap = 256) and six (1300).  The scores are exact in fp32 by construction (one
    product of multiples of 2^-4 per score), so TOL of tests/test_gpu_decode.py holds unchanged."""
    _steep(dtype, kind, Ncap)


@pytest.mark.parametrize("Ncap", [256, 1300])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_one_score_spike_in_each_wave_of_a_super_tile(dtype, Ncap):
    """One key at +40 among scores in [-40, -37.5], in wave 0, 1, 2, 3 of a super tile in turn (the second super tile of the cache /
    of its fifth chunk).  Under the causal mask the reference decides which rows see it: the second batch element is 40 keys shorter,
    so some of its 33 queries sit in front of the spike."""
    t0 = 128 if Ncap == 256 else 1152
    _steep(dtype, "spike", Ncap, spikes=[t0 + 32 * w + 5 for w in range(4)])


# ------------------------------------------------------------------------------------------------------ F. the caller's buffers

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_stale_nan_and_oversized_workspaces_never_reach_a_result(dtype):
    """Six splits with whole chunks empty: the combine must read only what this call's split kernel wrote.  A NaN-filled workspace,
    one of twice the size, and one left over from a larger call, with out and lse NaN on entry, each give the bits of the call on a
    fresh workspace."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    B, H, Nq, Ncap, d = 4, 2, 3, 1300, 64
    lens = [1300, 200, 0, 600]   # whole chunks of 256 keys empty in three of the four batch elements
    assert _splits(B, H, H, Nq, Ncap, d, dtype) == 6
    rng = np.random.default_rng(800)
    q, k, v = _inputs(rng, dtype, B, H, Nq, Ncap, d, lens)
    tq, tk, tv = (_to_dev(t, "bnhd", d, dtype) for t in (q, k, v))
    need = device_ops.decode_workspace(tq, tk).numel()
    nan = lambda n: torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    # what a different, larger call (twice the batch, no lengths) leaves behind in its workspace
    big = [torch.cat([t, t.flip(0)]).contiguous() for t in (tq, tk, tv)]
    stale = device_ops.decode_workspace(big[0], big[1])
    assert stale.numel() >= 2 * need
    device_ops.flash_attn_decode(big[0], big[1].nan_to_num(0.5), big[2].nan_to_num(-0.5), None, causal=False, workspace=stale)
    for causal in (True, False):
        fresh = _call(tq, tk, tv, lens, causal, "bnhd")
        _check(q, k, v, lens, causal, dtype, fresh[0], fresh[1])
        for ws in (nan(need), nan(2 * need), stale):
            o, l = nan(tq.numel()).view(tq.shape), nan(B * H * Nq).view(B, H, Nq)
            got = _call(tq, tk, tv, lens, causal, "bnhd", out=o, lse=l, workspace=ws)
            assert np.array_equal(got[0], fresh[0]) and np.array_equal(got[1], fresh[1])
            _check(q, k, v, lens, causal, dtype, got[0], got[1])
            _dead_rows_are_zero(got[0], got[1])


@pytest.mark.parametrize("Ncap", [200, 1300])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_null_lse_leaves_out_unchanged(dtype, Ncap):
    """The C ABI's lse = NULL on the device, in the split kernel's own epilogue (Ncap = 200: one split) and in the combine kernel
    (1300: six): out is bitwise the out of the call with lse."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    B, H, Nq, d = 4, 2, 3, 64
    lens = [Ncap, 200, 0, 2]
    assert (_splits(B, H, H, Nq, Ncap, d, dtype) == 1) == (Ncap == 200)
    rng = np.random.default_rng(810 + Ncap)
    q, k, v = _inputs(rng, dtype, B, H, Nq, Ncap, d, lens)
    tq, tk, tv = (_to_dev(t, "bnhd", d, dtype) for t in (q, k, v))
    tl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    ws = device_ops.decode_workspace(tq, tk)
    for causal in (True, False):
        with_lse = _raw("fa_mi355x_fwd_decode", (H,), tq, tk, tv, tl, ws, B, Nq, Ncap, d, "bnhd", causal, dtype)
        without = _raw("fa_mi355x_fwd_decode", (H,), tq, tk, tv, tl, ws, B, Nq, Ncap, d, "bnhd", causal, dtype, null_lse=True)
        assert without[1] is None and torch.equal(with_lse[0], without[0])
        _check(q, k, v, lens, causal, dtype, _from_dev(without[0], "bnhd"), to_np(with_lse[1]))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_caller_supplied_out_and_lse_through_the_unpad_path(dtype):
    """d = 80 in a 128-column cache: the library writes a padded result that flash_attn_decode copies into the caller's out.  The
    returned tensors are the caller's own and hold the reference's values."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    B, H, Nq, Ncap, d, dp = len(LENS), 2, 3, 520, 80, 128
    rng = np.random.default_rng(820)
    q, k, v = _inputs(rng, dtype, B, H, Nq, Ncap, d, LENS)
    for layout in ("bnhd", "bhnd"):
        tq, tk, tv = _to_dev(q, layout, d, dtype), _to_dev(k, layout, dp, dtype), _to_dev(v, layout, dp, dtype)
        out = torch.full(tq.shape, float("nan"), dtype=torch.float32, device="cuda")
        lse = torch.full((B, H, Nq), float("nan"), dtype=torch.float32, device="cuda")
        tl = torch.tensor(LENS, dtype=torch.int32, device="cuda")
        ro, rl = device_ops.flash_attn_decode(tq, tk, tv, tl, causal=True, layout=layout, out=out, lse=lse)
        torch.cuda.synchronize()
        assert ro is out and rl is lse
        _check(q, k, v, LENS, True, dtype, _from_dev(out, layout), to_np(lse))


# -------------------------------------------------------------------------------------- G. a batch element just under 2 GiB

def test_cache_batch_element_just_under_2_gib():
    """bf16, [B][N][H][d], 8 heads of d = 128, Ncap = 1048447 = the largest the library admits: row byte offsets up to 2^31 - 264192.
    The cache is one constant row (k = -1, v = 0.25) but for three windows of 300 random rows: the first rows, the rows around byte
    offset 2^30 and the last rows.  The fp64 reference adds the bulk in closed form (n_bulk exp(tau q.k_bulk)) to the windows' ordinary
    terms.  The windows carry between a quarter and three quarters of the softmax mass (asserted), so an offset that wraps and reads
    bulk rows for window rows moves out by far more than TOL."""
    torch = _torch()
    B, H, Nq, Ncap, d = 1, 8, 1, 1048447, 128
    assert (Ncap + 128) * H * d * 2 < 2 ** 31 <= (Ncap + 129) * H * d * 2
    assert _splits(B, H, H, Nq, Ncap, d, "bf16") == 128
    if torch.cuda.mem_get_info()[0] < 16 * 2 ** 30:
        pytest.skip("needs 16 GiB of free device memory for two caches of 2 GiB and their temporaries")
    rng = np.random.default_rng(900)
    K_BULK, V_BULK, W = -1.0, 0.25, 300
    starts = [0, 524288 - W // 2, Ncap - W]
    assert starts[1] * H * d * 2 < 2 ** 30 < (starts[1] + W) * H * d * 2
    q = oracle.bf16_round(rand_u(rng, (B, H, Nq, d)) * np.float32(0.25) + np.float32(0.75))          # U(0.5, 1)
    wk = oracle.bf16_round(rand_u(rng, (3, H, W, d)) * np.float32(0.5) - np.float32(0.25))           # U(-0.75, 0.25)
    wv = oracle.bf16_round(rand_u(rng, (3, H, W, d)))
    tq = _to_dev(q, "bnhd", d, "bf16")
    tk = torch.full((B, Ncap, H, d), K_BULK, dtype=torch.bfloat16, device="cuda")
    tv = torch.full((B, Ncap, H, d), V_BULK, dtype=torch.bfloat16, device="cuda")
    for s, a, b in zip(starts, wk, wv):
        tk[0, s:s + W] = torch.from_numpy(a.transpose(1, 0, 2).copy()).to("cuda", torch.bfloat16)
        tv[0, s:s + W] = torch.from_numpy(b.transpose(1, 0, 2).copy()).to("cuda", torch.bfloat16)

    def reference(n):
        tau = 1.0 / math.sqrt(d)
        out, lse, share = np.zeros((H, d)), np.zeros(H), np.zeros(H)
        for h in range(H):
            qh = q[0, h, 0].astype(np.float64)
            rows = [(wk[i, h, :max(0, min(W, n - s))], wv[i, h, :max(0, min(W, n - s))]) for i, s in enumerate(starts)]
            kw, vw = (np.concatenate([r[j] for r in rows]).astype(np.float64) for j in (0, 1))
            sw, sb, nb = tau * (kw @ qh), tau * K_BULK * qh.sum(), n - len(kw)
            m = max(sw.max(), sb)
            ew, eb = np.exp(sw - m), nb * math.exp(sb - m)
            out[h] = (ew @ vw + eb * V_BULK) / (ew.sum() + eb)
            lse[h] = m + math.log(ew.sum() + eb)
            share[h] = ew.sum() / (ew.sum() + eb)
        assert 0.25 < share.min() and share.max() < 0.75, share
        return out, lse

    try:
        for n, causal in ((Ncap, False), (Ncap, True), (524300, True)):
            if n < Ncap:   # the last window and half of the middle one are invalid now
                tk[0, n:] = float("nan")
                tv[0, n:] = float("nan")
            out, lse = _call(tq, tk, tv, [n], causal, "bnhd")
            ro, rl = reference(n)
            assert np.all(np.isfinite(out)) and np.all(np.isfinite(lse))
            err_o, err_l = maxabs(out[0, :, 0], ro), maxabs(lse[0, :, 0], rl)
            print(f"2 GiB cache, len {n}, causal {causal}: out {err_o:.3e}, lse {err_l:.3e}")
            assert err_o < TOL["bf16"] and err_l < TOL["bf16"], (n, causal, err_o, err_l)
    finally:
        del tk, tv
        torch.cuda.empty_cache()
