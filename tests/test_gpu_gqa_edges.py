"""Grouped-query (GQA / MQA) heads in the forward, dQ and dK/dV kernels: the paths and edges tests/test_gpu_gqa.py does not reach.
Several 256-row blocks per head in every kernel family, the default causal slot dispatch, both block orders of the causal slot
builds, the fp32 one-pass exclusion, the scale guard of tensors with different head counts, a caller's softmax scale, FA-1, groups of
7 and 32 heads, caller's buffers and the stage masks of fa_mi355x_bwd_gqa.

The two references are those of tests/test_gpu_gqa.py (whose helpers this file imports):
1. the fp64 oracle per query head on the expanded inputs, dK / dV summed over each group in fp64: the project's envelope, 1e-3 (bf16)
   and 1e-4 (fp32) max-abs on O, L, dQ and G times that on dK, dV.  Launches of many heads check whole groups only: the first, a
   middle and the last kv head of the flattened (B, Hkv).
2. the library itself on k and v repeated G times: out, l, dq bit for bit, dk and dv within G * 2^-23 * sum_g |term| of the fp64 group
   sum of the ungrouped call's per-head gradients.  Always all heads.
Every kernel plan asserted here is listed by plan_pins(), which tests/test_gqa_cpu.py holds against fa_mi355x_plan_gqa without a GPU."""
import math

import numpy as np
import pytest

import oracle
from gpu_util import maxabs, rand_u, to_np
from test_gpu_gqa import (ENVELOPE, GROUPINGS, _against_library, _bhnd, _check_group_sum, _check_oracle, _dev, _expand, _grouped,
                          _oracle, _plans, _same_kernel_opts, _torch)

pytestmark = pytest.mark.gpu

FA1, FA2 = 1, 2
LN2 = 0.6931471805599453
GROUPINGS = dict(GROUPINGS, B2H12kv3=(2, 12, 3),   # B * H = 24: three heads per XCD, G = 4, so groups straddle XCDs
                 B8H16kv4=(8, 16, 4))              # 128 heads: at N = 512 the default causal call takes the slot builds
BOTH, BNHD = ("bnhd", "bhnd"), ("bnhd",)
_DQ2 = "bwd_dq_kernel;bwd_dq_kernel;"
_PHASED = "bwd_dq_kernel;bwd_dkdv_kernel;group_sum_kernel"
_SLOT = "bwd_dq_slot_kernel;bwd_dkdv_slot_kernel;group_sum_kernel"
_SLOT_RAGGED = "bwd_prep_kernel;bwd_dkdv_slot_kernel;group_sum_kernel;bwd_dq_slot_kernel"
_CAUSAL64 = _DQ2 + "bwd_dkdv_kernel;group_sum_kernel"
_CAUSAL2 = _DQ2 + "bwd_dkdv_kernel;bwd_dkdv_kernel;group_sum_kernel"

# ---- 1. several 256-row blocks per head ----------------------------------------------------------------------------------------------
# name -> (dtype, d, N, causal, layouts, groupings (None: the three of GROUPINGS), forward plan, backward plan, {grouping: plans that
# differ}); the plans are those of a guarded call (option 8 = 3), as in tests/test_gpu_gqa.py
BLOCKS = {
    "bf16_d64_n768": ("bf16", 64, 768, False, BOTH, None, "fwd_slot_kernel;fwd_kernel", _SLOT, {}),
    "bf16_d64_n600": ("bf16", 64, 600, False, BNHD, None, "fwd_slot_kernel", _SLOT_RAGGED, {}),
    "bf16_d64_n768_causal": ("bf16", 64, 768, True, BOTH, None, "fwd_kernel", _CAUSAL64, {}),
    "bf16_d64_n600_causal": ("bf16", 64, 600, True, BNHD, None, "fwd_kernel", _CAUSAL64, {}),
    # batch * (N / 256) = 256 >= 128: the causal slot builds by default, ranked by default
    "bf16_d64_n512_causal_default_slot": ("bf16", 64, 512, True, BOTH, ("B8H16kv4",), "fwd_slot_kernel;fwd_kernel", _SLOT, {}),
    "bf16_d128_n768": ("bf16", 128, 768, False, BOTH, None, "fwd_slot_kernel;fwd_kernel", _PHASED, {}),
    "bf16_d128_n768_causal": ("bf16", 128, 768, True, BNHD, None, "fwd_kernel;fwd_kernel", _CAUSAL2, {}),
    "bf16_d128_n520": ("bf16", 128, 520, False, BNHD, None, "fwd_kernel", _PHASED, {}),
    "bf16_d128_n520_causal": ("bf16", 128, 520, True, BNHD, None, "fwd_kernel;fwd_kernel", _CAUSAL2, {}),
    "bf16_d32_n300": ("bf16", 32, 300, False, BNHD, None, "fwd_kernel", _PHASED, {}),
    "bf16_d32_n300_causal": ("bf16", 32, 300, True, BOTH, None, "fwd_kernel;fwd_kernel", _CAUSAL2, {}),
    # (24 heads x 6 blocks of 128 queries are beyond what the split-key forward takes)
    "f32_d64_n768": ("f32", 64, 768, False, BOTH, None, "fwd_splitk_f32_kernel", _PHASED, {"B2H12kv3": ("fwd_kernel", _PHASED)}),
    "f32_d64_n520_causal": ("f32", 64, 520, True, BOTH, None, "fwd_splitk_f32_kernel", _PHASED, {}),
    "f32_d32_n300_causal": ("f32", 32, 300, True, BNHD, None, "fwd_kernel", _PHASED, {}),
    "f32_d128_n300": ("f32", 128, 300, False, BNHD, None, "fwd_kernel", _PHASED, {}),
}
BLOCK_CASES = [(s, g, lay) for s, c in BLOCKS.items() for g in (c[5] or ("B2H8kv2", "B1H6kv1", "B2H12kv3")) for lay in c[4]]

# ---- 2. block order of the causal slot builds: (B, H, Hkv, N) -------------------------------------------------------------------------
ORDER_SHAPES = [(3, 8, 2, 512),     # BH = 24: map_block's XCD branch, an even block count
                (1, 5, 1, 768),     # BH = 5: the other branch, an odd block count
                (5, 8, 4, 256),     # BH = 40
                (3, 24, 8, 1024)]   # BH = 72: nine heads per XCD, G = 3
ORDER_OPTS = lambda order: (5, 3, 3, 0, 0, 0, 0, order)   # the causal slot builds of dK/dV, forward and dQ; 1 = paired, 2 = ranked
# ---- 3. where the ungrouped call takes the fp32 one-pass backward ----------------------------------------------------------------------
ONEPASS_SHAPES = [(1, 8, 2, 1024), (4, 64, 16, 256)]   # (the second takes it without a cut sweep)
ONEPASS_CASES = [(1, 8, 2, 1024, c, lay) for c in (False, True) for lay in BOTH] + [(4, 64, 16, 256, c, "bnhd") for c in (False, True)]
_TWO_KERNELS = "bwd_prep_kernel;bwd_dkdv_kernel;group_sum_kernel;bwd_dq_kernel"
ONEPASS_FWD = {(1, 8, 2, 1024): "fwd_splitk_f32_kernel", (4, 64, 16, 256): "fwd_kernel"}
# ---- 4. the scale guard: forward plans of option 8 = 1 (folded) and 2 (fp32 scaling) at grouping (2, 8, 2), N = 512 -------------------
GUARD_FWD_PLANS = {(64, False): ("fwd_slot_kernel", "fwd_kernel"), (64, True): ("fwd_kernel", "fwd_kernel"),
                   (128, False): ("fwd_slot_kernel", "fwd_kernel"), (128, True): ("fwd_kernel;fwd_kernel", "fwd_kernel;fwd_kernel")}
# ---- 5. FA-1 and a caller's scale at grouping (2, 8, 2): (dtype, d, N) -> {causal: plans} -------------------------------------------
FA1_SHAPES = {("bf16", 64, 256): {False: ("fwd_kernel", _SLOT), True: ("fwd_kernel", _CAUSAL64)},
              ("f32", 32, 100): {False: ("fwd_kernel", _PHASED), True: ("fwd_kernel", _PHASED)}}
# (the first of them is also the shape of the ln 2 autograd case, whose plans these are as well: the library ignores a guard there)
SCALED_SHAPES = {("bf16", 64, 600): {False: ("fwd_slot_kernel", _SLOT_RAGGED), True: ("fwd_kernel", _CAUSAL64)},
                 ("f32", 64, 520): {False: ("fwd_splitk_f32_kernel", _PHASED), True: ("fwd_splitk_f32_kernel", _PHASED)}}
# ---- 6. large and odd groups ---------------------------------------------------------------------------------------------------------
BIG_GROUPS = {"B1H7kv1": (1, 7, 1), "B1H32kv1": (1, 32, 1), "B2H14kv2": (2, 14, 2)}
BIG_PLANS = {256: ("fwd_slot_kernel;fwd_kernel", _SLOT), 200: ("fwd_slot_kernel", _SLOT_RAGGED)}
# ---- 7. stage masks at grouping (2, 8, 2), d = 64: (dtype, N, causal) -> the plans of the stage masks PREP, DKDV, DQ, for the calls
# the test makes: bf16 with a guard (option 8 = 3), fp32 without one (no kernel of an fp32 call folds the scale) ----------------------
STAGE_PLANS = {("bf16", 600, False): ("bwd_prep_kernel", "bwd_dkdv_slot_kernel;group_sum_kernel", "bwd_dq_slot_kernel"),
               ("bf16", 600, True): ("bwd_prep_kernel", "bwd_dkdv_kernel;group_sum_kernel", "bwd_dq_kernel;bwd_dq_kernel"),
               ("f32", 520, False): ("bwd_prep_kernel", "bwd_dkdv_kernel;group_sum_kernel", "bwd_dq_kernel"),
               ("f32", 520, True): ("bwd_prep_kernel", "bwd_dkdv_kernel;group_sum_kernel", "bwd_dq_kernel")}


def _stage_opts(dtype):
    return (0,) * 8 + (3,) if dtype == "bf16" else ()


def plan_pins():
    """Every kernel plan this file asserts: ((B, H, Hkv, N, d, causal, variant, dtype, stages, options), "kernel;kernel;...")."""
    pins = []

    def both(B, H, Hkv, N, d, causal, dtype, opts, fwd, bwd, variant=FA2):
        o = (tuple(opts or ()) + (0,) * 8)[:8] + (3,)
        pins.append(((B, H, Hkv, N, d, causal, variant, dtype, 0, o), fwd))
        pins.append(((B, H, Hkv, N, d, causal, variant, dtype, 7, o), bwd))
    for shape, grouping, _ in BLOCK_CASES:
        dtype, d, N, causal, _, _, fwd, bwd, other = BLOCKS[shape]
        both(*GROUPINGS[grouping], N, d, causal, dtype, None, *other.get(grouping, (fwd, bwd)))
    for B, H, Hkv, N in ORDER_SHAPES:
        for order in (1, 2):
            both(B, H, Hkv, N, 64, True, "bf16", ORDER_OPTS(order), "fwd_slot_kernel;fwd_kernel", _SLOT)
    for B, H, Hkv, N in ONEPASS_SHAPES:
        for causal in (False, True):
            both(B, H, Hkv, N, 64, causal, "f32", None, ONEPASS_FWD[B, H, Hkv, N], _TWO_KERNELS)
    for table, variant in ((FA1_SHAPES, FA1), (SCALED_SHAPES, FA2)):
        for (dtype, d, N), by_causal in table.items():
            for causal, (fwd, bwd) in by_causal.items():
                both(2, 8, 2, N, d, causal, dtype, None, fwd, bwd, variant)
    for B, H, Hkv in BIG_GROUPS.values():
        for N, (fwd, bwd) in BIG_PLANS.items():
            both(B, H, Hkv, N, 64, False, "bf16", None, fwd, bwd)
    for (d, causal), plans in GUARD_FWD_PLANS.items():
        for mode, plan in zip((1, 2), plans):
            pins.append(((2, 8, 2, 512, d, causal, FA2, "bf16", 0, (0,) * 8 + (mode,)), plan))
    for (dtype, N, causal), plans in STAGE_PLANS.items():
        for stage, plan in zip((1, 2, 4), plans):
            pins.append(((2, 8, 2, N, 64, causal, FA2, dtype, stage, _stage_opts(dtype)), plan))
    return pins


def _plan(B, H, Hkv, N, d, causal, variant, dtype, stages, opts):
    from flash_attention_minitorch_amd import _lib
    code = _lib.FA_DTYPE_BF16 if dtype == "bf16" else _lib.FA_DTYPE_F32
    return ";".join(_lib.plan_gqa(B, H, Hkv, N, d, causal, variant, code, stages, opts or None))


def _three_groups(B, Hkv):
    """The first, a middle and the last kv head of the flattened (B, Hkv)."""
    return sorted({0, (B * Hkv) // 2, B * Hkv - 1})


_CASES = {}


def _case(key, dtype, B, H, Hkv, N, d, causal, kv_heads=None, seed=0, q_factor=1.0):
    """numpy q, do (B, H, N, d) and k, v (B, Hkv, N, d), U(-1, 1) and bf16-rounded for bf16, and the fp64 oracle on ``kv_heads`` (None:
    all groups), computed once per ``key`` and shared by the layouts and tests of a case.  ``q_factor``: the oracle is called with
    q * q_factor and its dq is scaled back (a caller's softmax scale: q_factor = scale * sqrt(d))."""
    if key not in _CASES:
        rng = np.random.default_rng(52000 + seed)
        q, do = rand_u(rng, (B, H, N, d)), rand_u(rng, (B, H, N, d))
        k, v = rand_u(rng, (B, Hkv, N, d)), rand_u(rng, (B, Hkv, N, d))
        if dtype == "bf16":
            q, k, v, do = (oracle.bf16_round(t) for t in (q, k, v, do))
        ref = None
        if kv_heads is None or len(kv_heads):   # (an empty list: the inputs alone)
            ref = _oracle(q.astype(np.float64) * q_factor, k, v, do, causal, kv_heads)
            ref["dq"] = ref["dq"] * q_factor
        _CASES[key] = (q, k, v, do, ref)
    return _CASES[key]


def _run_both_references(tag, arrays, kv_heads, dtype, B, H, Hkv, causal, layout, opts, opts_ungrouped="same", **kw):
    """One grouped forward and backward on the device against the oracle (on ``kv_heads``) and the library on expanded k, v."""
    torch = _torch()
    q, k, v, do, ref = arrays
    tq, tk, tv, tdo = (_dev(a, layout, dtype) for a in (q, k, v, do))
    got = _grouped(tq, tk, tv, tdo, causal, layout, opts, **kw)
    torch.cuda.synchronize()
    assert got[0].shape == tq.shape and got[2].shape == tq.shape and got[3].shape == tk.shape and got[4].shape == tv.shape
    assert tuple(got[1].shape) == (B, H, q.shape[2])
    _check_oracle(got, ref, kv_heads, Hkv, layout, dtype, tag)
    if opts_ungrouped == "same":
        opts_ungrouped = _same_kernel_opts(B, H, q.shape[2], q.shape[3], causal, dtype, opts)
    _against_library(tq, tk, tv, tdo, got, H // Hkv, causal, layout, opts_ungrouped, **kw)
    return (tq, tk, tv, tdo), got


@pytest.mark.parametrize("shape,grouping,layout", BLOCK_CASES, ids=[f"{s}-{g}-{lay}" for s, g, lay in BLOCK_CASES])
def test_several_blocks_per_head(shape, grouping, layout):
    """More than one 256-row block per head in every kernel family: N > 256, so the workgroup id -> (batch*head, block) maps run with more
    than one block per head together with the kv head of bh / G; B * H = 24 with G = 4 puts a group's heads on different XCDs; and the
    (8, 16, 4) case is the only default call that reaches the causal slot builds of dQ and dK/dV (256 blocks, ranked)."""
    dtype, d, N, causal, _, _, fwd, bwd, other = BLOCKS[shape]
    B, H, Hkv = GROUPINGS[grouping]
    assert _plans(B, H, Hkv, N, d, causal, dtype, None) == other.get(grouping, (fwd, bwd))
    kv_heads = _three_groups(B, Hkv) if B * H > 24 else None
    arrays = _case(("blocks", shape, grouping), dtype, B, H, Hkv, N, d, causal, kv_heads, seed=len(shape) + 31 * len(grouping) + N)
    _run_both_references(f"blocks {shape} {grouping} {layout}", arrays, kv_heads, dtype, B, H, Hkv, causal, layout, None)


@pytest.mark.parametrize("order", [1, 2], ids=["paired", "ranked"])
@pytest.mark.parametrize("B,H,Hkv,N", ORDER_SHAPES)
def test_causal_slot_builds_block_order_with_groups(B, H, Hkv, N, order):
    """The grouped form of test_causal_slot_builds_block_order (tests/test_gpu_parity.py): the causal slot builds of the forward, dQ and dK/dV forced
    (options 5, 3, 3) with the paired and the ranked block order.  Every block of every head is visited exactly once and read its own
    group's K and V: all heads against the library on expanded k, v under the same options, three whole groups against the oracle."""
    opts = ORDER_OPTS(order)
    assert _plans(B, H, Hkv, N, 64, True, "bf16", opts) == ("fwd_slot_kernel;fwd_kernel", _SLOT)
    kv_heads = _three_groups(B, Hkv)
    arrays = _case(("order", B, H, Hkv, N), "bf16", B, H, Hkv, N, 64, True, kv_heads, seed=B * H + N)
    _run_both_references(f"order {(B, H, Hkv, N)} order={order}", arrays, kv_heads, "bf16", B, H, Hkv, True, "bnhd", opts, opts)


@pytest.mark.parametrize("B,H,Hkv,N,causal,layout", ONEPASS_CASES)
def test_where_the_ungrouped_call_takes_the_one_pass_backward(B, H, Hkv, N, causal, layout):
    """The fp32 one-pass exclusion of select_bwd: fp32, d = 64 at launch sizes where the ungrouped call runs bwd_onepass_f32_kernel (atomic adds: not repeatable).  The
    grouped call runs what option 4 = 4 selects, the library on expanded k, v is called with exactly that option, and three
    repeated grouped backward calls return the same bits, which is what the exclusion exists for."""
    torch = _torch()
    from flash_attention_minitorch_amd import _lib
    assert "bwd_onepass_f32_kernel" in _lib.plan(B * H, N, 64, causal, FA2, _lib.FA_DTYPE_F32, 7, None)
    plans = _plans(B, H, Hkv, N, 64, causal, "f32", None)
    assert plans == (ONEPASS_FWD[B, H, Hkv, N], _TWO_KERNELS) and "onepass" not in plans[1]
    assert _same_kernel_opts(B, H, N, 64, causal, "f32", None) == (0, 0, 0, 0, 4)
    kv_heads = _three_groups(B, Hkv) if B * H > 24 else None
    arrays = _case(("onepass", B, H, Hkv, N, causal), "f32", B, H, Hkv, N, 64, causal, kv_heads, seed=7 * B + N + causal)
    (tq, tk, tv, tdo), first = _run_both_references(f"onepass {(B, H, Hkv, N)} causal={causal} {layout}", arrays, kv_heads, "f32", B, H,
                                                    Hkv, causal, layout, None)
    for _ in range(2):
        again = _grouped(tq, tk, tv, tdo, causal, layout, None)
        torch.cuda.synchronize()
        for name, a, b in zip(("out", "l", "dq", "dk", "dv"), first, again):
            assert torch.equal(a, b), name


# ---- 4. the scale guard under grouping ------------------------------------------------------------------------------------------------

GUARD_FACTOR = 4.0   # (a power of two: exact in bf16)


def _guard_inputs(d, causal, which):
    """(q, k, v, do, oracle) of the three guard inputs at grouping (2, 8, 2), N = 512: "a" U(-1, 1) throughout, "b" the last kv head of
    the last batch element of k times GUARD_FACTOR, "c" the last query head of the last batch element of q times it."""
    key = ("guard", d, causal, which)
    if key not in _CASES:
        q, k, v, do, _ = _case(("guard-base", d), "bf16", 2, 8, 2, 512, d, False, kv_heads=[], seed=900 + d)
        q, k = q.copy(), k.copy()
        if which == "b":
            k[-1, -1] *= np.float32(GUARD_FACTOR)
        if which == "c":
            q[-1, -1] *= np.float32(GUARD_FACTOR)
        _CASES[key] = (q, k, v, do, _oracle(q, k, v, do, causal))
    return _CASES[key]


GUARD_MARGIN = 8.0   # a row of it has the squared norm 64 * d; no row of k can exceed 16 * d (input "b": every element below 4)


def _inside_large_values(t, margin):
    """``t`` as a slice of a larger tensor filled with GUARD_MARGIN, ``margin`` elements on either side.  Not NaN: the guard's reduction
    is fmaxf from 0, which drops a NaN operand, so a NaN margin would leave an over-reading pass with the right maxima."""
    torch = _torch()
    big = torch.full((t.numel() + 2 * margin,), GUARD_MARGIN, dtype=t.dtype, device="cuda")
    part = big[margin:margin + t.numel()].view(t.shape)
    part.copy_(t)
    return part


@pytest.mark.parametrize("layout", BOTH)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_scale_guard_of_a_grouped_call(d, causal, layout):
    """The scale guard of tensors with different head counts, after test_scale_guard_routes_by_operand_size_without_a_host_sync: q has
    B*N*H rows and k B*N*Hkv.  k lies inside a larger tensor filled with 8.0 (a q-sized margin on either side: rows of squared norm
    64 * d, beyond every row of k), so a pass that reads k with q's row count, in the separate pass or in the forward that fills the
    guard itself, returns a k maximum that differs from torch's and sends input "a" to the fp32-scaling kernels; and the large rows
    of input "b" are the LAST rows of k, which a pass that stops short misses.  Factor: 4 (d = 64 and d = 128 alike;
    device_ops.pick_opts on the host copy says "exact" for "b" and "c" at both, asserted below: U(-1, 1) sits at 0.6 - 0.7 of the
    budget, one operand times 4 at 2.4 - 2.8 of it).
    - the maxima of _scale_guard_gqa equal torch's within 1e-3 relative and those a produce_guard forward leaves within 1e-5 (the
      bounds of the ungrouped test);
    - the default guard = "auto" pair equals, bit for bit, the pair given the separate-pass guard, the pair whose forward produced the
      guard, and the explicit OPTS_FOLDED_SCALE / OPTS_EXACT_SCALE pair that pick_opts names;
    - "a" meets the envelope, "b" and "c" the fp32-scaling kernels' bound of that test, 5e-3 * max(1, max |ref|) (G times on dk, dv);
    - where the forward plans of option 8 = 1 and 2 differ, the folded and the exact outputs differ: the routing is not vacuous."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops as dev
    B, H, Hkv, N, G = 2, 8, 2, 512, 4
    plans = tuple(_plan(B, H, Hkv, N, d, causal, FA2, "bf16", 0, (0,) * 8 + (mode,)) for mode in (1, 2))
    assert plans == GUARD_FWD_PLANS[d, causal]
    for which in "abc":
        q, k, v, do, ref = _guard_inputs(d, causal, which)
        tq, tk_plain, tv, tdo = (_dev(a, layout, "bf16") for a in (q, k, v, do))
        tk = _inside_large_values(tk_plain, tq.numel())
        want = dev.pick_opts(tq.cpu(), tk_plain.cpu())
        assert want == (dev.OPTS_FOLDED_SCALE if which == "a" else dev.OPTS_EXACT_SCALE), (which, d)
        # the separate pass, and the forward that fills a guard in its own launch
        guard = dev._scale_guard_gqa(tq, tk)
        gq, gk = float(guard[:256].max()), float(guard[256:].max())
        tq2, tk2 = float(tq.float().pow(2).sum(-1).max()), float(tk.float().pow(2).sum(-1).max())
        assert abs(gq - tq2) < 1e-3 * gq and abs(gk - tk2) < 1e-3 * gk, (which, gq, tq2, gk, tk2)
        g2 = dev.new_guard(tq)
        o_, l_, _ = dev.flash_attn_fwd_gqa(tq, tk, tv, causal=causal, layout=layout, guard=g2, produce_guard=True)
        produced = (o_, l_) + tuple(dev.flash_attn_bwd_gqa(tq, tk, tv, o_, tdo, l_, causal=causal, layout=layout, guard=g2))
        assert abs(float(g2[:256].max()) - gq) < 1e-5 * gq and abs(float(g2[256:].max()) - gk) < 1e-5 * gk, which
        default = _grouped(tq, tk, tv, tdo, causal, layout, None)
        shared = _grouped(tq, tk, tv, tdo, causal, layout, None, guard=guard)
        explicit = _grouped(tq, tk, tv, tdo, causal, layout, want, guard=None)
        torch.cuda.synchronize()
        for name, a, b, c, e in zip(("out", "l", "dq", "dk", "dv"), default, shared, produced, explicit):
            assert torch.equal(a, b), (which, name, "separate-pass guard")
            assert torch.equal(a, c), (which, name, "produced guard")
            assert torch.equal(a, e), (which, name, "explicit option 8")
        bound = None if which == "a" else (lambda name, r: 5e-3 * max(1.0, float(np.max(np.abs(r)))))
        _check_oracle(default, ref, None, Hkv, layout, "bf16", f"guard d={d} causal={causal} {layout} input {which}", bound)
        _against_library(tq, tk_plain, tv, tdo, default, G, causal, layout, None)
        if plans[0] != plans[1]:
            folded = dev.flash_attn_fwd_gqa(tq, tk, tv, causal=causal, layout=layout, guard=None, opts=dev.OPTS_FOLDED_SCALE)[0]
            exact = dev.flash_attn_fwd_gqa(tq, tk, tv, causal=causal, layout=layout, guard=None, opts=dev.OPTS_EXACT_SCALE)[0]
            assert not torch.equal(folded, exact), which


# ---- 5. a caller's scale, and FA-1 ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", BOTH)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype,d,N", list(SCALED_SHAPES))
def test_a_callers_softmax_scale(dtype, d, N, causal, layout):
    """A caller's scale in the grouped kernels: softmax_scale = 0.2, neither 1/sqrt(d) nor ln 2, through forward and backward.  The oracle applies sqrt(1/d) itself: it is
    called with q * 0.2 * sqrt(d) and its dq is scaled back, as test_folded_softmax_scale_keeps_the_slot_kernels_exact_on_large_
    activations does.  0.2 * sqrt(64) = 1.6: the scores are 1.6 times those of the default scale, still those of U(-1, 1)-sized
    operands, so the envelope applies."""
    B, H, Hkv = 2, 8, 2
    assert _plans(B, H, Hkv, N, d, causal, dtype, None) == SCALED_SHAPES[dtype, d, N][causal]
    arrays = _case(("scaled", dtype, N, causal), dtype, B, H, Hkv, N, d, causal, seed=N + causal, q_factor=0.2 * math.sqrt(d))
    _run_both_references(f"scale0.2 {dtype} N={N} causal={causal} {layout}", arrays, None, dtype, B, H, Hkv, causal, layout, None,
                         softmax_scale=0.2)


@pytest.mark.parametrize("layout", BOTH)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype,d,N", list(FA1_SHAPES))
def test_fa1_with_groups(dtype, d, N, causal, layout):
    """variant = FA-1 through flash_attn_fwd_gqa / flash_attn_bwd_gqa: l = sum exp(s - m) and the row maximum m, both (B, H, N).
    m within 1e-5 of the fp64 row maximum (tests/test_gpu_parity.py's bound for FA-1's m), m + log l and everything else within the
    envelope, and all of it the bits of the ungrouped FA-1 call on expanded k, v."""
    torch = _torch()
    B, H, Hkv = 2, 8, 2
    assert _plans(B, H, Hkv, N, d, causal, dtype, None, FA1) == FA1_SHAPES[dtype, d, N][causal]
    q, k, v, do, ref = _case(("fa1", dtype, N, causal), dtype, B, H, Hkv, N, d, causal, seed=3 * N + causal)
    tq, tk, tv, tdo = (_dev(a, layout, dtype) for a in (q, k, v, do))
    got = _grouped(tq, tk, tv, tdo, causal, layout, None, variant=FA1)
    torch.cuda.synchronize()
    out, l, dq, dk, dv, m = got
    assert tuple(m.shape) == tuple(l.shape) == (B, H, N) and dk.shape == tk.shape
    err_m = maxabs(to_np(m).reshape(B * Hkv, H // Hkv, N), ref["m"])
    print(f"fa1 {dtype} N={N} causal={causal} {layout}: m {err_m:.3e} (< 1e-05)")
    assert err_m < 1e-5
    _check_oracle((out, m + torch.log(l), dq, dk, dv), ref, None, Hkv, layout, dtype, f"fa1 {dtype} N={N} causal={causal} {layout}")
    _against_library(tq, tk, tv, tdo, got, H // Hkv, causal, layout, _same_kernel_opts(B, H, N, d, causal, dtype, None), variant=FA1)


@pytest.mark.parametrize("layout", BOTH)
@pytest.mark.parametrize("causal", [False, True])
def test_autograd_with_the_folded_scale(causal, layout):
    """flash_attn_gqa(q', k, v, causal, softmax_scale = ln 2) under autograd, the call multi_head_attention(fold_scale=True)
    issues: q' = q * log2(e) / sqrt(d) rounded to bf16 once, as the folded query projection leaves it.  bf16, d = 64, N = 600 (ragged,
    three blocks per head: the first shape of test_a_callers_softmax_scale), grouping (2, 8, 2).  The oracle is called with q' * ln 2 * sqrt(d) and its dq is scaled back to q'.  Bound: that of
    test_autograd_returns_gradients_in_each_input_shape_and_dtype, the envelope plus one bf16 rounding of the returned gradient."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    B, H, Hkv, N, d, G = 2, 8, 2, 600, 64, 4
    assert _plans(B, H, Hkv, N, d, causal, "bf16", None) == SCALED_SHAPES["bf16", d, N][causal]
    key = ("autograd-ln2", causal)
    if key not in _CASES:
        q, k, v, do, _ = _case(("autograd-base",), "bf16", B, H, Hkv, N, d, False, kv_heads=[], seed=77)
        qf = oracle.bf16_round((q * np.float32(1.4426950408889634 / math.sqrt(d))).astype(np.float32))
        g = LN2 * math.sqrt(d)
        ref = _oracle(qf.astype(np.float64) * g, k, v, do, causal)
        ref["dq"] = ref["dq"] * g
        _CASES[key] = (qf, k, v, do, ref)
    qf, k, v, do, ref = _CASES[key]
    tq, tk, tv = (_dev(a, layout, "bf16").requires_grad_() for a in (qf, k, v))
    out = device_ops.flash_attn_gqa(tq, tk, tv, causal=causal, softmax_scale=LN2, layout=layout)
    out.backward(_dev(do, layout, "f32"))
    torch.cuda.synchronize()
    assert out.dtype is torch.float32 and out.shape == tq.shape
    err_o = maxabs(_bhnd(out, layout).reshape(B * Hkv, G, N, d), ref["o"])
    print(f"autograd ln2 causal={causal} {layout}: o {err_o:.3e} (< {ENVELOPE['bf16']:.1e})")
    assert err_o < ENVELOPE["bf16"]
    shapes = {"dq": (B * Hkv, G, N, d), "dk": (B * Hkv, N, d), "dv": (B * Hkv, N, d)}
    for name, t, scale in (("dq", tq, 1), ("dk", tk, G), ("dv", tv, G)):
        assert t.grad.shape == t.shape and t.grad.dtype is torch.bfloat16, name
        err = np.abs(_bhnd(t.grad, layout).astype(np.float64).reshape(shapes[name]) - ref[name])
        bound = scale * ENVELOPE["bf16"] + 2.0 ** -8 * np.abs(ref[name])
        print(f"autograd ln2 causal={causal} {layout} {name}: max-abs {err.max():.3e}, worst err - bound {float((err - bound).max()):.3e}")
        assert np.all(err < bound), (name, float((err - bound).max()))


# ---- 6. large and odd groups ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", BOTH)
@pytest.mark.parametrize("N", [256, 200])
@pytest.mark.parametrize("grouping", list(BIG_GROUPS))
def test_large_and_odd_groups(grouping, N, layout):
    """Large and odd groups: G = 7 and G = 32 (multi-query) and (2, 14, 2) in group_sum_kernel's four-deep unrolled loop, bf16, d = 64.  The G-times
    envelope on dK / dV is wide here (3.2e-2 at G = 32): the group-sum bound against the library is the sharp reference; both are
    printed."""
    B, H, Hkv = BIG_GROUPS[grouping]
    assert _plans(B, H, Hkv, N, 64, False, "bf16", None) == BIG_PLANS[N]
    arrays = _case(("big", grouping, N), "bf16", B, H, Hkv, N, 64, False, seed=H + N)
    _run_both_references(f"groups {grouping} N={N} {layout}", arrays, None, "bf16", B, H, Hkv, False, layout, None)


# ---- 7. caller's buffers and stage masks ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", BOTH)
@pytest.mark.parametrize("dtype,n_big,n_small", [("bf16", 600, 200), ("f32", 520, 256)])
def test_two_shapes_through_one_workspace_and_callers_buffers(dtype, n_big, n_small, layout):
    """A caller's workspace, gradient and output buffers on the device: d = 64, a small call (1, 6, 1, n_small), a large one (2, 8, 2, n_big) and the small one again through ONE workspace sized for
    the large call (bwd_workspace_gqa), 256-byte aligned and filled with NaN before each call, with NaN-filled ``grads`` and a
    NaN-filled ``out`` for the forward: every result is finite and has the bits of the call that allocates its own buffers.  The last
    call finds the scratch behind its row constants inside what the larger call used."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops as dev
    nan = lambda shape: torch.full(tuple(shape), float("nan"), dtype=torch.float32, device="cuda")
    calls = {}
    for name, (B, H, Hkv), N in (("small", (1, 6, 1), n_small), ("big", (2, 8, 2), n_big)):
        q, k, v, do, _ = _case(("buffers", dtype, name), dtype, B, H, Hkv, N, 64, False, kv_heads=[], seed=N)
        t = tuple(_dev(a, layout, dtype) for a in (q, k, v, do))
        calls[name] = (t, _grouped(*t, False, layout, None))
    big = calls["big"][0]
    ws = dev.bwd_workspace_gqa(big[0], big[1], layout)
    assert ws.data_ptr() % 256 == 0
    for name in ("small", "big", "small"):
        (tq, tk, tv, tdo), want = calls[name]
        ws.fill_(float("nan"))
        o_buf, grads = nan(tq.shape), (nan(tq.shape), nan(tk.shape), nan(tv.shape))
        out, l, _ = dev.flash_attn_fwd_gqa(tq, tk, tv, layout=layout, out=o_buf)
        got = dev.flash_attn_bwd_gqa(tq, tk, tv, out, tdo, l, layout=layout, workspace=ws, grads=grads)
        torch.cuda.synchronize()
        assert out is o_buf and all(a is b for a, b in zip(got, grads))
        for nm, a, b in zip(("out", "l", "dq", "dk", "dv"), (out, l) + tuple(got), want):
            assert bool(torch.isfinite(a).all()), (name, nm)
            assert torch.equal(a, b), (name, nm)


def _bwd_stage(grouped, t, out, l, grads, ws, Hkv, causal, layout, stage, guard):
    """One stage mask of fa_mi355x_bwd_gqa (``grouped``) or fa_mi355x_bwd_guarded through the C ABI."""
    from flash_attention_minitorch_amd import _lib, device_ops as dev
    tq, tk, tv, tdo = t
    (B, N, H, d) = tq.shape if layout == "bnhd" else (tq.shape[0], tq.shape[2], tq.shape[1], tq.shape[3])
    p = dev._ptr
    ptrs = (p(tq), p(tk), p(tv), p(out), p(tdo), p(grads[0]), p(grads[1]), p(grads[2]), p(l), None, p(ws))
    tail = (N, d, dev._DECODE_LAYOUTS[layout], 0.0, int(causal), FA2, dev._dtype_code(tq), stage, None, 0, p(guard), dev._stream_ptr())
    if grouped:
        _lib.check(_lib.core().fa_mi355x_bwd_gqa(*ptrs, B, H, Hkv, *tail))
    else:
        _lib.check(_lib.core().fa_mi355x_bwd_guarded(*ptrs, B, H, *tail))


@pytest.mark.parametrize("layout", BOTH)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype,N", [("bf16", 600), ("f32", 520)])
def test_stage_masks_of_the_grouped_backward(dtype, N, causal, layout):
    """The stage masks of fa_mi355x_bwd_gqa: one backward of grouping (2, 8, 2), d = 64, as three calls of fa_mi355x_bwd_gqa on one NaN-filled workspace:
    FA_BWD_STAGE_PREP, then _DKDV, then _DQ.  validate() swaps the caller's dk / dv for the scratch in every one of them, but only a
    call with the dK/dV stage runs the group sum that writes them: the preprocess leaves all three NaN-filled gradients untouched, the
    dK/dV call leaves dq untouched, and the dQ call, given fresh NaN-filled dk and dv, leaves those untouched (the ungrouped entry
    point behaves the same, asserted below).  dq is bit for bit that of the same three calls of fa_mi355x_bwd_guarded on expanded k, v,
    dk and dv meet the group-sum bound, and everything meets the envelope against the oracle."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops as dev
    B, H, Hkv, d, G = 2, 8, 2, 64, 4
    assert tuple(_plan(B, H, Hkv, N, d, causal, FA2, dtype, st, _stage_opts(dtype)) for st in (1, 2, 4)) == STAGE_PLANS[dtype, N, causal]
    q, k, v, do, ref = _case(("stages", dtype, causal), dtype, B, H, Hkv, N, d, causal, seed=11 * N + causal)
    t = tuple(_dev(a, layout, dtype) for a in (q, k, v, do))
    te = (t[0], _expand(t[1], G, layout), _expand(t[2], G, layout), t[3])
    nan = lambda like: torch.full(tuple(like.shape), float("nan"), dtype=torch.float32, device="cuda")
    all_nan = lambda x: bool(torch.isnan(x).all())
    results = {}
    for grouped, ts in ((True, t), (False, te)):
        tq, tk, tv, _ = ts
        if grouped:
            out, l, _ = dev.flash_attn_fwd_gqa(tq, tk, tv, causal=causal, layout=layout)
            ws = dev.bwd_workspace_gqa(tq, tk, layout)
            guard = dev._scale_guard_gqa(tq, tk) if dtype == "bf16" else None
        else:
            out, l, _ = (dev.flash_attn_fwd_bnhd if layout == "bnhd" else dev.flash_attn_fwd)(tq, tk, tv, causal)
            ws = dev.bwd_workspace(tq if layout == "bhnd" else tq.permute(0, 2, 1, 3))
            guard = dev.scale_guard(tq, tk) if dtype == "bf16" else None
        ws.fill_(float("nan"))
        grads = (nan(tq), nan(tk), nan(tv))
        _bwd_stage(grouped, ts, out, l, grads, ws, Hkv, causal, layout, dev.STAGE_PREP, guard)
        torch.cuda.synchronize()
        assert all(all_nan(g) for g in grads), "the preprocess wrote a gradient"
        _bwd_stage(grouped, ts, out, l, grads, ws, Hkv, causal, layout, dev.STAGE_DKDV, guard)
        torch.cuda.synchronize()
        assert all_nan(grads[0]), "the dK/dV stage wrote dq"
        assert bool(torch.isfinite(grads[1]).all()) and bool(torch.isfinite(grads[2]).all())
        fresh = (grads[0], nan(tk), nan(tv))
        _bwd_stage(grouped, ts, out, l, fresh, ws, Hkv, causal, layout, dev.STAGE_DQ, guard)
        torch.cuda.synchronize()
        assert all_nan(fresh[1]) and all_nan(fresh[2]), "the dQ stage wrote dk or dv"
        assert bool(torch.isfinite(grads[0]).all())
        results[grouped] = (out, l) + grads
    got, lib = results[True], results[False]
    for name, a, b in zip(("out", "l", "dq"), got, lib):
        assert torch.equal(a, b), f"{name} differs from the ungrouped stages on expanded k, v"
    _check_group_sum(got[3], lib[3], G, layout, "dk")
    _check_group_sum(got[4], lib[4], G, layout, "dv")
    _check_oracle(got, ref, None, Hkv, layout, dtype, f"stages {dtype} N={N} causal={causal} {layout}")
