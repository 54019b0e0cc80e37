"""Key mask and dropout at the shapes, layouts and masks callers send: the FEAT 1 / 2 builds of fwd_kernel / bwd_dq_kernel, the
DKDV_CARE / DKDV_CARE_DROP / DKDV_DROP_F32 builds of bwd_dkdv_kernel and the launcher's routing of every masked or dropout call away
from the slot kernels, the tiled builds and the fp32 one-pass backward.  Every test compares with the fp64 oracle
(oracle.masked_attention_* / dropout_attention_*) on the same (bf16-rounded) U(-1, 1) inputs at the bounds of test_gpu_parity.py:
1e-4 (fp32) and 1e-3 (bf16), times the dropout scale."""
import numpy as np
import pytest

import oracle
from gpu_util import (LEFT_PAD, core_bwd, core_fwd, finite_drops_as_inf, masked_row_max, maxabs, oracle_heads, padding_and_hole_mask,
                      rand_u, to_np)

pytestmark = pytest.mark.gpu

TOL32 = 1e-4   # (test_gpu_parity.py)
TOLBF = 1e-3
TYPES = [("bf16", 32), ("bf16", 64), ("bf16", 128), ("f32", 32), ("f32", 64), ("f32", 128)]


@pytest.fixture(scope="module")
def dev():
    import torch
    from flash_attention_minitorch_amd import device_ops
    assert torch.cuda.is_available()
    return device_ops


def _inputs(rng, shape, dtype):
    """Four U(-1, 1) arrays (q, k, v, dO), bf16-rounded for the bf16 path, and their device tensors."""
    import torch
    arrs = [rand_u(rng, shape) for _ in range(4)]
    if dtype == "bf16":
        arrs = [oracle.bf16_round(a) for a in arrs]
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    return arrs, [torch.from_numpy(a).to("cuda", tdt) for a in arrs]


def _logsumexp(variant, l, m):
    """L of either side-output convention (FA-1: m + log l) as a NumPy array; -inf on dead rows."""
    from flash_attention_minitorch_amd import _lib
    if variant != _lib.FA_VARIANT_FA1:
        return to_np(l)
    with np.errstate(divide="ignore", invalid="ignore"):
        return to_np(m) + np.log(to_np(l))


def _assert_parity(tag, got, ref, tol, dead=None):
    """o, L, dq, dk, dv against the oracle: finite (but the L of dead rows) and within tol; returns the errors."""
    errs = {}
    for nm in ("o", "L", "dq", "dk", "dv"):
        a, b = np.asarray(got[nm]), np.asarray(ref[nm])
        if nm == "L" and dead is not None:
            assert np.array_equal(np.isneginf(a), dead), (tag, "dead rows")
            a, b = np.where(dead, 0, a), np.where(dead, 0, b)
        assert np.all(np.isfinite(a)), (tag, nm)
        errs[nm] = maxabs(a, b)
        print(f"{tag} {nm}: {errs[nm]:.3e} (bound {tol:.1e})")
    for nm, e in errs.items():
        assert e < tol, (tag, nm, e)
    return errs


# ---------------------------------------------------------------- 1. key-mask patterns x shapes
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("N", [128, 320, 1024])
@pytest.mark.parametrize("dtype,d", TYPES)
def test_key_mask_left_padding_and_block_edges(dev, dtype, d, N, causal):
    """Batch 0 is LEFT padded (keys [0, 70) at -inf: the first bf16 key tile and the first two fp32 tiles are wholly masked, so every
    row starts from fwd_kernel's made-up reference, `if (HM && m_ref == -INFINITY) m_ref = 0.f`, and continues on live tiles; under
    the causal rule rows 0..69 -- two whole waves and part of a third -- are dead: O = 0, L = -inf, FA-1 l = 0 and m = -inf, dq = 0).
    Batch 1 keeps key 0, has a whole -inf block in the interior and finite "minus infinity" entries (-1e4, the lowest float32) on a
    fifth of the other keys; on the CPU the oracle shows they act as -inf (< 1e-12), then the GPU owes the ordinary bound.
    N = 128 (one query block, no ragged tail: the key mask is the only source of -inf; 2 bf16 key tiles), 320 (three causally paired
    query blocks, block 1 paired with itself; 5 bf16 tiles: the `if (t < nt)` tail, the other parity of the smask double buffer),
    1024 (16 / 32 tiles; kept for every type: the fp64 oracle takes about a second there).  B * H = 8: map_block's XCD branch."""
    import torch
    from flash_attention_minitorch_amd import _lib
    B, H = 2, 4
    arrs, (tq, tk, tv, tdo) = _inputs(np.random.default_rng(1100 + d + N), (B, H, N, d), dtype)
    mask = padding_and_hole_mask(N)
    finite = np.isfinite(mask) & (mask < 0)
    assert finite[1].sum() >= 10 and not finite[0].any() and mask[1, 0] == 0 and (mask[1] == -1e4).any() and (mask[1] < -1e38).any()
    tmask = torch.from_numpy(mask).cuda()
    tol = TOLBF if dtype == "bf16" else TOL32
    ro, rL = oracle.masked_attention_fw(*arrs[:3], mask[:, None, :], causal)
    rdq, rdk, rdv = oracle.masked_attention_bw(*arrs, mask[:, None, :], causal)
    ref = {"o": ro, "L": rL, "dq": rdq, "dk": rdk, "dv": rdv}
    rm = masked_row_max(arrs[0], arrs[1], mask, causal)
    # the expectation is the reference's: on it, the finite entries are -inf (batch 1 holds them all)
    as_inf = finite_drops_as_inf(mask)[1:, None, :]
    one = [a[1:] for a in arrs]
    io, iL = oracle.masked_attention_fw(*one[:3], as_inf, causal)
    ig = oracle.masked_attention_bw(*one, as_inf, causal)
    assert maxabs(io, ro[1:]) < 1e-12 and maxabs(iL, rL[1:]) < 1e-12
    assert all(maxabs(a, b[1:]) < 1e-12 for a, b in zip(ig, (rdq, rdk, rdv)))
    dead = np.isneginf(rL)
    want_dead = np.zeros((B, H, N), dtype=bool)
    if causal:
        want_dead[0, :, :LEFT_PAD] = True
    assert np.array_equal(dead, want_dead)
    drop = np.isneginf(mask)
    for variant in (_lib.FA_VARIANT_FA1, _lib.FA_VARIANT_FA2):
        o, l, m = dev.flash_attn_fwd_masked(tq, tk, tv, tmask, causal, variant)
        dq, dk, dv = dev.flash_attn_bwd_masked(tq, tk, tv, o, tdo, l, m, tmask, causal, variant)
        got = {"o": to_np(o), "L": _logsumexp(variant, l, m), "dq": to_np(dq), "dk": to_np(dk), "dv": to_np(dv)}
        _assert_parity(f"mask {dtype} d={d} N={N} causal={causal} fa{variant}", got, ref, tol, dead)
        if variant == _lib.FA_VARIANT_FA1:
            gm, gl = to_np(m), to_np(l)
            assert np.array_equal(np.isneginf(gm), dead) and np.all(gl[dead] == 0)
            assert np.all(np.isfinite(gm[~dead])) and np.all(np.isfinite(gl)) and np.all(gl[~dead] > 0)
            assert maxabs(gm[~dead], rm[~dead]) < (1e-5 if dtype == "f32" else tol)
        # dead rows: exactly nothing
        assert np.all(got["o"][dead] == 0) and np.all(got["dq"][dead] == 0)
        for b in range(B):
            # keys at -inf: exactly zero gradient; the finite "minus infinity" ones: within the bound (exp2 of a hugely negative
            # number is zero by underflow only), finite
            assert np.all(got["dk"][b][:, drop[b]] == 0) and np.all(got["dv"][b][:, drop[b]] == 0)
            for nm in ("dk", "dv"):
                g = got[nm][b][:, finite[b]]
                assert np.all(np.isfinite(g)) and (g.size == 0 or float(np.max(np.abs(g))) < tol), nm


@pytest.mark.parametrize("dtype,d", [("bf16", 64), ("bf16", 128), ("f32", 32), ("f32", 64)])
def test_key_mask_first_tile_at_finite_minus_infinity(dev, dtype, d):
    """Left padding written with FINITE values: keys [0, 70) at -1e4 (batch 0; staged as mask / tau, about -8e4 raw) and at the lowest
    float32 (batch 1; mask / tau overflows to -inf).  Batch 0's first key tile then sets a reference near -8e4, the first live tile
    overflows exp2 against it and takes the MAX_DEFER_SUM redo, which moves the reference by 8e4 and rescales O and l by alpha = 0.
    Non-causal only: every row then has unbiased keys, which is what makes a finite bias act as -inf (under the causal rule rows
    0..69 would see biased keys alone, where the bias cancels and fp32 scores near 8e4 keep no digits).  The oracle shows the
    equivalence with the -inf mask on the CPU (< 1e-12); the GPU owes the ordinary bound."""
    import torch
    from flash_attention_minitorch_amd import _lib
    B, H, N = 2, 4, 320
    arrs, (tq, tk, tv, tdo) = _inputs(np.random.default_rng(1150 + d), (B, H, N, d), dtype)
    mask = np.zeros((B, N), dtype=np.float32)
    mask[0, :LEFT_PAD] = np.float32(-1e4)
    mask[1, :LEFT_PAD] = np.finfo(np.float32).min
    tmask = torch.from_numpy(mask).cuda()
    tol = TOLBF if dtype == "bf16" else TOL32
    ro, rL = oracle.masked_attention_fw(*arrs[:3], mask[:, None, :], False)
    rg = oracle.masked_attention_bw(*arrs, mask[:, None, :], False)
    ref = dict(zip(("o", "L", "dq", "dk", "dv"), (ro, rL) + tuple(rg)))
    as_inf = finite_drops_as_inf(mask)[:, None, :]
    assert np.isneginf(as_inf[:, 0, :LEFT_PAD]).all()
    io, iL = oracle.masked_attention_fw(*arrs[:3], as_inf, False)
    assert maxabs(io, ro) < 1e-12 and maxabs(iL, rL) < 1e-12
    assert all(maxabs(a, b) < 1e-12 for a, b in zip(oracle.masked_attention_bw(*arrs, as_inf, False), rg))
    rm = masked_row_max(arrs[0], arrs[1], as_inf[:, 0], False)
    for variant in (_lib.FA_VARIANT_FA1, _lib.FA_VARIANT_FA2):
        o, l, m = dev.flash_attn_fwd_masked(tq, tk, tv, tmask, False, variant)
        dq, dk, dv = dev.flash_attn_bwd_masked(tq, tk, tv, o, tdo, l, m, tmask, False, variant)
        got = {"o": to_np(o), "L": _logsumexp(variant, l, m), "dq": to_np(dq), "dk": to_np(dk), "dv": to_np(dv)}
        _assert_parity(f"finite padding {dtype} d={d} fa{variant}", got, ref, tol)
        if variant == _lib.FA_VARIANT_FA1:
            assert np.all(np.isfinite(to_np(l))) and maxabs(to_np(m), rm) < (1e-5 if dtype == "f32" else tol)
        for nm in ("dk", "dv"):
            g = got[nm][:, :, :LEFT_PAD]
            assert np.all(np.isfinite(g)) and float(np.max(np.abs(g))) < tol, nm


# ---------------------------------------------------------------- 2. fp32 d = 64 must leave the one-pass backward
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("N", [256, 512, 1024])
def test_fp32_d64_mask_and_dropout_do_not_take_the_one_pass_backward(dev, N, causal):
    """fp32, d = 64, N >= 256 is where the plain backward CAN be bwd_onepass_f32_kernel, which knows nothing of key masks or dropout:
    onepass_f32 must decline such calls (DKDV_F32_64 / DKDV_DROP_F32 and the FEAT builds of bwd_dq_kernel instead).  Whether it takes
    a plain call depends on the launch size: at B * H = 8 on 256 CUs it does not at N = 256 and 512 (8 and 16 workgroups, cut into at
    most 2 and 4 parts, fill less than 80 % of a round: the plain call runs two kernels there as well, so those two sizes only check
    the masked builds), and it does at N = 1024 (32 workgroups in 8 parts; the plan is asserted below): there a condition that forgot
    the mask or the dropout would run the one-pass kernel and ignore them.  A key mask that drops a third of the keys and, separately,
    dropout at rate 0.2, against the oracle; the masked dk must also differ from the unmasked call's by far more than the bound,
    which an ignored mask cannot do."""
    import torch
    from flash_attention_minitorch_amd import _lib
    B, H, d = 2, 4, 64
    if torch.cuda.get_device_properties(0).multi_processor_count == 256:
        plain = _lib.plan(B * H, N, d, causal, _lib.FA_VARIANT_FA2, _lib.FA_DTYPE_F32, dev.STAGE_ALL, None)
        if N == 1024:
            assert plain == ["bwd_prep_kernel", "bwd_onepass_f32_kernel"]
        else:
            assert "bwd_onepass_f32_kernel" not in plain
    rng = np.random.default_rng(1200 + N)
    arrs, (tq, tk, tv, tdo) = _inputs(rng, (B, H, N, d), "f32")
    mask = np.zeros((B, N), dtype=np.float32)
    for b in range(B):
        mask[b, rng.permutation(np.arange(1, N))[:N // 3]] = -np.inf   # (key 0 stays: no dead row under the causal rule)
    tmask = torch.from_numpy(mask).cuda()
    ro, rL = oracle.masked_attention_fw(*arrs[:3], mask[:, None, :], causal)
    rg = oracle.masked_attention_bw(*arrs, mask[:, None, :], causal)
    o, l, _ = dev.flash_attn_fwd_masked(tq, tk, tv, tmask, causal)
    dq, dk, dv = dev.flash_attn_bwd_masked(tq, tk, tv, o, tdo, l, None, tmask, causal)
    got = {"o": to_np(o), "L": to_np(l), "dq": to_np(dq), "dk": to_np(dk), "dv": to_np(dv)}
    _assert_parity(f"f32 d=64 N={N} causal={causal} mask", got, dict(zip(("o", "L", "dq", "dk", "dv"), (ro, rL) + tuple(rg))), TOL32)
    drop = np.isneginf(mask)
    for b in range(B):
        assert np.all(got["dk"][b][:, drop[b]] == 0) and np.all(got["dv"][b][:, drop[b]] == 0)
    o_p, l_p, _ = dev.flash_attn_fwd(tq, tk, tv, causal)
    dk_plain = dev.flash_attn_bwd(tq, tk, tv, o_p, tdo, l_p, None, causal)[1]
    assert maxabs(got["dk"], to_np(dk_plain)) > 100 * TOL32
    # the two-kernel path is deterministic (each dq element is summed by one wave in a fixed order); the one-pass kernel adds its
    # dq with fp32 atomics in whatever order the workgroups arrive, so it is not: a second call must repeat dq bit for bit
    dq2 = dev.flash_attn_bwd_masked(tq, tk, tv, o, tdo, l, None, tmask, causal)[0]
    assert torch.equal(dq, dq2)
    # dropout, no mask
    rate, seed = 0.2, 0xD0D0
    scale = 1.0 / (1.0 - rate)
    keep = oracle.dropout_keep_mask(B * H, N, rate, seed)
    ro, rL = oracle.dropout_attention_fw(*arrs[:3], keep, scale, None, causal)
    rg = oracle.dropout_attention_bw(*arrs, keep, scale, None, causal)
    o, l, _ = dev.flash_attn_fwd_dropout(tq, tk, tv, rate, seed, scale, None, causal)
    dq, dk, dv = dev.flash_attn_bwd_dropout(tq, tk, tv, o, tdo, l, None, rate, seed, scale, None, causal)
    got = {"o": to_np(o), "L": to_np(l), "dq": to_np(dq), "dk": to_np(dk), "dv": to_np(dv)}
    _assert_parity(f"f32 d=64 N={N} causal={causal} dropout", got, dict(zip(("o", "L", "dq", "dk", "dv"), (ro, rL) + tuple(rg))),
                   TOL32 * scale)
    assert torch.equal(dq, dev.flash_attn_bwd_dropout(tq, tk, tv, o, tdo, l, None, rate, seed, scale, None, causal)[0])


# ---------------------------------------------------------------- 3. dropout where it has never run
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("N", [128, 320])
@pytest.mark.parametrize("dtype,d", [("f32", 64), ("f32", 128), ("bf16", 32), ("bf16", 64)])
def test_dropout_types_and_block_edges(dev, dtype, d, N, causal):
    """Dropout (rate 0.2) at fp32 d = 64 (DKDV_DROP_F32 at D = 64 exists for these calls alone) and d = 128, bf16 d = 32 (under the
    causal rule the one path where the phased forward / dQ feature builds run in ranked block order) and d = 64; B * H = 8 (the XCD
    branch of map_block / map_block_ranked: bh enters the hash); one and three query blocks; with and without the left-padding mask
    (under the causal rule its first 70 rows are dead).  Forward, dQ and dK/dV regenerate ONE mask: all three match the oracle on the
    oracle's mask.  L is the log-sum-exp BEFORE dropout: it is the L of the call without dropout.  scale = 1 / (1 - rate) and, at one
    shape, minitorch's scale = 1."""
    import torch
    from flash_attention_minitorch_amd import _lib
    B, H = 2, 4
    rate, seed = 0.2, 0xC0FFEE + N
    arrs, (tq, tk, tv, tdo) = _inputs(np.random.default_rng(1300 + d + N), (B, H, N, d), dtype)
    keep = oracle.dropout_keep_mask(B * H, N, rate, seed)
    pad = np.zeros((B, N), dtype=np.float32)
    pad[0, :LEFT_PAD] = -np.inf
    scales = [1.0 / (1.0 - rate)] + ([1.0] if (N == 320 and d == 64) else [])
    for km in (None, pad):
        okm = None if km is None else km[:, None, :]
        tkm = None if km is None else torch.from_numpy(km).cuda()
        l_nodrop = dev.flash_attn_fwd_masked(tq, tk, tv, torch.zeros((B, N), device="cuda") if km is None else tkm, causal)[1]
        for scale in scales:
            tol = (TOLBF if dtype == "bf16" else TOL32) * scale
            ro, rL = oracle.dropout_attention_fw(*arrs[:3], keep, scale, okm, causal)
            rg = oracle.dropout_attention_bw(*arrs, keep, scale, okm, causal)
            ref = dict(zip(("o", "L", "dq", "dk", "dv"), (ro, rL) + tuple(rg)))
            dead = np.isneginf(rL)
            assert dead.any() == (causal and km is not None)
            for variant in (_lib.FA_VARIANT_FA1, _lib.FA_VARIANT_FA2):
                o, l, m = dev.flash_attn_fwd_dropout(tq, tk, tv, rate, seed, scale, tkm, causal, variant)
                dq, dk, dv = dev.flash_attn_bwd_dropout(tq, tk, tv, o, tdo, l, m, rate, seed, scale, tkm, causal, variant)
                got = {"o": to_np(o), "L": _logsumexp(variant, l, m), "dq": to_np(dq), "dk": to_np(dk), "dv": to_np(dv)}
                _assert_parity(f"dropout {dtype} d={d} N={N} causal={causal} mask={km is not None} scale={scale:.2f} fa{variant}",
                               got, ref, tol, dead)
                assert np.all(got["o"][dead] == 0) and np.all(got["dq"][dead] == 0)
                gl = to_np(l_nodrop)
                assert np.array_equal(np.isneginf(gl), dead)
                assert maxabs(np.where(dead, 0, got["L"]), np.where(dead, 0, gl)) < tol
                if km is not None:
                    assert np.all(got["dk"][0][:, :LEFT_PAD] == 0) and np.all(got["dv"][0][:, :LEFT_PAD] == 0)


# ---------------------------------------------------------------- 4. ranked dispatch with a short last chunk
def _partial_chunk_shape():
    """(This RESTATES the launcher's rank_chunk(wgs_per_cu, nb) = max(1, CUs * wgs_per_cu / (4 * nb)) and the blocks per head of the
    builds named below -- the library exposes neither.  If either changes in fa_api.hip, the test keeps passing but may stop reaching
    a short last chunk: change this helper with them.)
    (B, H, heads per XCD, chunk C) with B * H <= 128 a multiple of 8 whose heads per XCD exceed the ranked dispatch's chunk C
    without being a multiple of it -- so map_block_ranked's last chunk of every XCD is short -- or None.  N = 2048: the slot kernels
    take 8 blocks per head at one workgroup per CU, the phased dK/dV builds 16 at two, so C = CUs / 32 for all of them (rank_chunk,
    fa_api.hip)."""
    import torch
    C = max(1, torch.cuda.get_device_properties(0).multi_processor_count // 32)
    for per in [12] + list(range(2, 17)):
        if per > C and per % C != 0:
            return 4, 2 * per, per, C
    return None


@pytest.mark.parametrize("call", ["bf16_plain", "bf16_key_mask", "f32_plain", "bf16_dropout"])
def test_causal_ranked_dispatch_with_a_partial_last_chunk(dev, call):
    """map_block_ranked takes the heads of an XCD in chunks of C and its last chunk may be short (cper = min(C, per - chunk * C)); no
    other test has per > C with per % C != 0.  On 256 CUs: B * H = 96, N = 2048, d = 64, causal -> 12 heads per XCD against C = 8,
    chunk 1 has 4.  The oracle runs on the first and last head of a full and of a short chunk in the first and the last XCD
    (heads 0, 7, 8, 11, 12, 84, 95 there).
    Kernels (fa_mi355x_plan on 256 CUs): bf16 plain, U(-1, 1) operands so the guarded default folds the scale: fwd_slot_kernel
    (causal build, ranked, C = 16: one chunk), then bwd_dq_slot_kernel (causal build, ranked, C = 8, preprocesses its own rows) and
    bwd_dkdv_slot_kernel (causal build, C = 8); fp32 plain: fwd_kernel, then bwd_prep_kernel and bwd_onepass_f32_kernel (ranked,
    C = 8); key mask: DKDV_CARE ranked over 16 key blocks of 128 (C = 8); dropout: DKDV_CARE_DROP likewise."""
    import torch
    from flash_attention_minitorch_amd import _lib
    shape = _partial_chunk_shape()
    if shape is None:
        pytest.skip("no B * H <= 128 leaves a short last chunk on this device's CU count")
    B, H, per, C = shape
    BH, N, d = B * H, 2048, 64
    dtype = "f32" if call == "f32_plain" else "bf16"
    if torch.cuda.get_device_properties(0).multi_processor_count == 256:
        bf, f32 = _lib.FA_DTYPE_BF16, _lib.FA_DTYPE_F32
        assert _lib.plan(BH, N, d, True, 2, bf, 0, dev.OPTS_FOLDED_SCALE) == ["fwd_slot_kernel"]
        assert _lib.plan(BH, N, d, True, 2, bf, dev.STAGE_ALL, None) == ["bwd_dq_slot_kernel", "bwd_dkdv_slot_kernel"]
        assert _lib.plan(BH, N, d, True, 2, f32, dev.STAGE_ALL, None) == ["bwd_prep_kernel", "bwd_onepass_f32_kernel"]
    arrs, (tq, tk, tv, tdo) = _inputs(np.random.default_rng(1400), (B, H, N, d), dtype)
    heads = sorted({0, C - 1, C, per - 1, per, 7 * per, BH - 1})
    tol = TOLBF if dtype == "bf16" else TOL32
    flat = [a.reshape(BH, N, d) for a in arrs]
    if call in ("bf16_plain", "f32_plain"):
        o, l, _ = dev.flash_attn_fwd(tq, tk, tv, True)
        dq, dk, dv = dev.flash_attn_bwd(tq, tk, tv, o, tdo, l, None, True)
        ref = oracle_heads(*flat, True, heads)
    else:
        mask = tmask = None
        if call == "bf16_key_mask":
            rng = np.random.default_rng(1401)
            mask = np.where(rng.uniform(size=(B, N)) < 0.1, -np.inf, 0.0).astype(np.float32)
            mask[:, 0] = 0
            tmask = torch.from_numpy(mask).cuda()
            o, l, _ = dev.flash_attn_fwd_masked(tq, tk, tv, tmask, True)
            dq, dk, dv = dev.flash_attn_bwd_masked(tq, tk, tv, o, tdo, l, None, tmask, True)
        else:
            rate, seed = 0.2, 0xFACADE
            tol *= 1.0 / (1.0 - rate)
            o, l, _ = dev.flash_attn_fwd_dropout(tq, tk, tv, rate, seed, 1.0 / (1.0 - rate), None, True)
            dq, dk, dv = dev.flash_attn_bwd_dropout(tq, tk, tv, o, tdo, l, None, rate, seed, 1.0 / (1.0 - rate), None, True)
            keep = oracle.dropout_keep_mask(BH, N, rate, seed, heads=heads)
        ref = {n: [] for n in ("o", "L", "dq", "dk", "dv")}
        for i, hh in enumerate(heads):
            b, h = divmod(hh, H)
            one = [a[b:b + 1, h:h + 1] for a in arrs]
            if mask is not None:
                ro, rL = oracle.masked_attention_fw(*one[:3], mask[b:b + 1, None, :], True)
                rg = oracle.masked_attention_bw(*one, mask[b:b + 1, None, :], True)
            else:
                ro, rL = oracle.dropout_attention_fw(*one[:3], keep[i:i + 1], 1.0 / (1.0 - rate), None, True)
                rg = oracle.dropout_attention_bw(*one, keep[i:i + 1], 1.0 / (1.0 - rate), None, True)
            for n, a in zip(("o", "L", "dq", "dk", "dv"), (ro, rL) + tuple(rg)):
                ref[n].append(a[0, 0])
        ref = {n: np.stack(a) for n, a in ref.items()}
    idx = torch.tensor(heads, device="cuda")
    got = {"o": to_np(o.reshape(BH, N, d)[idx]), "L": to_np(l.reshape(BH, N)[idx])}
    for nm, g in (("dq", dq), ("dk", dk), ("dv", dv)):
        assert bool(torch.isfinite(g).all()), nm   # (every head, not only the sampled ones)
        got[nm] = to_np(g.reshape(BH, N, d)[idx])
    _assert_parity(f"ranked {call} BH={BH} C={C}", got, ref, tol)
    if call == "bf16_key_mask":
        for i, hh in enumerate(heads):
            dropped = np.isneginf(mask[hh // H])
            assert np.all(got["dk"][i][dropped] == 0) and np.all(got["dv"][i][dropped] == 0)


# ---------------------------------------------------------------- 5. [B][N][H][d] layout
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("N", [200, 256])
@pytest.mark.parametrize("dtype,d", [("bf16", 64), ("f32", 32)])
def test_bnhd_layout_with_mask_and_dropout(dev, dtype, d, N, causal):
    """fa_mi355x_{fwd,bwd}_masked / _dropout take `layout`, and head_base / mask_heads / drop_base all depend on the (b, h) split,
    but device_ops exposes these calls for (B, H, N, d) alone: [B][N][H][d] through the C ABI (gpu_util.core_fwd / core_bwd) with the
    left-padding / hole masks of test_key_mask_left_padding_and_block_edges, H = 3.  The selection does not read the layout, so the
    same kernels run as for the [B][H][N][d] call on permuted copies and the results are bit for bit the same; and against the
    oracle."""
    import torch
    from flash_attention_minitorch_amd import _lib
    B, H = 2, 3
    bnhd, bhnd = _lib.FA_LAYOUT_BNHD, _lib.FA_LAYOUT_BHND
    arrs, ts = _inputs(np.random.default_rng(1500 + d + N), (B, H, N, d), dtype)
    perm = lambda t: t.permute(0, 2, 1, 3).contiguous()
    tn = [perm(t) for t in ts]                                   # (B, N, H, d)
    mask = padding_and_hole_mask(N)
    tmask = torch.from_numpy(mask).cuda()
    rate, seed = 0.2, 0xBEEF
    scale = 1.0 / (1.0 - rate)
    keep = oracle.dropout_keep_mask(B * H, N, rate, seed)
    base = TOLBF if dtype == "bf16" else TOL32
    for tag, dropout, tol in (("mask", None, base), ("dropout", (rate, scale, seed), base * scale)):
        if dropout is None:
            ro, rL = oracle.masked_attention_fw(*arrs[:3], mask[:, None, :], causal)
            rg = oracle.masked_attention_bw(*arrs, mask[:, None, :], causal)
        else:
            ro, rL = oracle.dropout_attention_fw(*arrs[:3], keep, scale, mask[:, None, :], causal)
            rg = oracle.dropout_attention_bw(*arrs, keep, scale, mask[:, None, :], causal)
        ref = dict(zip(("o", "L", "dq", "dk", "dv"), (ro, rL) + tuple(rg)))
        dead = np.isneginf(rL)
        assert dead.any() == causal
        for variant in (_lib.FA_VARIANT_FA1, _lib.FA_VARIANT_FA2):
            o, l, m = core_fwd(bnhd, *tn[:3], tmask, dropout, causal, variant)
            dq, dk, dv = core_bwd(bnhd, *tn[:3], o, tn[3], l, m, tmask, dropout, causal, variant)
            o_r, l_r, m_r = core_fwd(bhnd, *ts[:3], tmask, dropout, causal, variant)
            g_r = core_bwd(bhnd, *ts[:3], o_r, ts[3], l_r, m_r, tmask, dropout, causal, variant)
            assert o.shape == (B, N, H, d) and l.shape == (B, H, N)
            assert torch.equal(perm(o), o_r) and torch.equal(l, l_r) and (m is None or torch.equal(m, m_r))
            for nm, a, b in zip(("dq", "dk", "dv"), (dq, dk, dv), g_r):
                assert torch.equal(perm(a), b), (tag, nm)
            got = {"o": to_np(perm(o)), "L": _logsumexp(variant, l, m), "dq": to_np(perm(dq)), "dk": to_np(perm(dk)), "dv": to_np(perm(dv))}
            _assert_parity(f"bnhd {tag} {dtype} d={d} N={N} causal={causal} fa{variant}", got, ref, tol, dead)
            assert np.all(got["o"][dead] == 0) and np.all(got["dq"][dead] == 0)
            drop = np.isneginf(mask)
            for b in range(B):
                assert np.all(got["dk"][b][:, drop[b]] == 0) and np.all(got["dv"][b][:, drop[b]] == 0)
