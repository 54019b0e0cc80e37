"""The kernel families beside bf16 d = 64 -- bf16 d = 128, bf16 d = 32, fp32 d = 32, fp32 d = 128 -- at the sizes where their own
kernels can go wrong: block, stage and tail boundaries (group 1), the ranked block order over many heads with a partial last chunk
(group 2, bf16 / fp32 d = 64 included) and the default dispatch of bf16 d = 128 around its launch-size thresholds (group 3).

Reference: the fp64 dense oracle on the same inputs (U(-1, 1), bf16-rounded first for bf16).  Tolerances are the project's own (max-abs):
TOL32 = 1e-4 for fp32, TOLBF = 1e-3 for bf16, on o, L (FA-1: m + log l, and m), dq, dk, dv; every value finite.  Every output buffer
holds NaN on entry: a block that no workgroup visits leaves NaN rows, not the right answer of the call before.

Every case asserts, through _lib.plan, the kernels its call launches.  The expected names restate select_fwd / select_dq / select_dkdv
(csrc/fa_api.hip) for the four families:
  forward   bf16 d = 128, FA-2, N >= 64: the slot kernel when N % 64 == 0 without the causal mask, or N % 256 == 0 under it and
            (batch * N / 256 >= 256 or option 1 = 3); a guarded call (the default) then launches it AND its fp32-scaling twin, the
            phased kernel; option 8 = 2 the phased kernel alone.  Everything else: the phased kernel.
            The phased bf16 kernel under the causal mask (N >= 64) is followed by its split-operand build on query block 0.
  dQ        one bwd_dq_kernel (bf16 d = 128 without the mask: the 8-wave build; else the 4-wave phased one); bf16 causal N >= 64: the
            split-operand follow-up on query block 0 behind it.  The launch preprocesses its own rows (no bwd_prep_kernel, dQ first)
            unless option 4 = 1 or the whole launch is the split-operand build (bf16, N < 64).
  dK/dV     one bwd_dkdv_kernel; bf16 causal N >= 64: the thin main launch (queries 0..63 skipped) + the split-operand follow-up.
(The plan lists kernel names, not template arguments: which BUILD of a name runs follows from the same rules and is stated per case.)"""
import numpy as np
import pytest

import oracle
from gpu_util import maxabs, oracle_heads, rand_u, to_np
from test_gpu_parity import TOL32, TOLBF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    from flash_attention_minitorch_amd import device_ops
    assert torch.cuda.is_available()
    return device_ops


FA1, FA2 = 1, 2
FAMILIES = [("bf16", 128), ("bf16", 32), ("f32", 32), ("f32", 128)]
OPT_PREP = (0, 0, 0, 0, 1)   # option 4 = 1: the separate preprocess kernel
NAMES = ("o", "L", "dq", "dk", "dv")


def _tol(dtype):
    return TOLBF if dtype == "bf16" else TOL32


def _opt(opts, i):
    return int(opts[i]) if opts is not None and len(opts) > i else 0


def _with(opts, i, value):
    o = list(opts or ()) + [0] * 10
    o[i] = value
    return tuple(o[:max(i + 1, len(opts or ()))])


# ---------------------------------------------------------------- the plan each call must have (see the header)
def expect_fwd(dtype, d, BH, N, causal, variant=FA2, opts=None):
    bf = dtype == "bf16"
    phased = ["fwd_kernel"] * (2 if bf and causal and N >= 64 else 1)
    if not (bf and d == 128):
        return phased
    o1, nqb = _opt(opts, 1), (N + 255) // 256
    cslot = causal and N % 256 == 0 and (o1 == 3 or (o1 == 0 and BH * nqb >= 256))
    slot = variant == FA2 and o1 != 2 and N >= 64 and (cslot or (not causal and N % 64 == 0))
    mode = _opt(opts, 8)
    if not slot or mode == 2:
        return phased
    return ["fwd_slot_kernel"] + (phased if mode != 1 else [])


def expect_bwd(dtype, N, causal, opts=None):
    pair = 2 if dtype == "bf16" and causal and N >= 64 else 1
    dq, dkdv = ["bwd_dq_kernel"] * pair, ["bwd_dkdv_kernel"] * pair
    fused = _opt(opts, 4) == 0 and not (dtype == "bf16" and N < 64)
    return dq + dkdv if fused else ["bwd_prep_kernel"] + dkdv + dq


def planned(dev, dtype, d, BH, N, causal, variant, stages, opts):
    """The plan of the call device_ops issues with these options: bf16 d = 64 / 128 calls with option 8 = 0 are GUARDED calls."""
    from flash_attention_minitorch_amd import _lib
    if dtype == "bf16" and d in (64, 128) and _opt(opts, 8) == 0:
        opts = _with(opts, 8, 3)
    return _lib.plan(BH, N, d, causal, variant, _lib.FA_DTYPE_BF16 if dtype == "bf16" else _lib.FA_DTYPE_F32, stages, opts)


def assert_plan(dev, dtype, d, BH, N, causal, variant=FA2, opts=None, fwd=None, bwd=None):
    want_f = expect_fwd(dtype, d, BH, N, causal, variant, opts) if fwd is None else fwd
    want_b = expect_bwd(dtype, N, causal, opts) if bwd is None else bwd
    got_f = planned(dev, dtype, d, BH, N, causal, variant, 0, opts)
    got_b = planned(dev, dtype, d, BH, N, causal, variant, dev.STAGE_ALL, opts)
    assert got_f == want_f, (dtype, d, BH, N, causal, variant, opts, got_f)
    assert got_b == want_b, (dtype, d, BH, N, causal, variant, opts, got_b)


# ---------------------------------------------------------------- inputs, calls on NaN-filled outputs, checks
def make_inputs(dtype, shape, seed):
    import torch
    rng = np.random.default_rng(seed)
    arrs = [rand_u(rng, shape) for _ in range(4)]
    if dtype == "bf16":
        arrs = [oracle.bf16_round(a) for a in arrs]
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    return arrs, [torch.from_numpy(a).to("cuda", tdt) for a in arrs]


def _nan(shape):
    import torch
    return torch.full(tuple(shape), float("nan"), dtype=torch.float32, device="cuda")


def run_fwd(dev, t, causal, variant=FA2, opts=None):
    q = t[0]
    m = _nan(q.shape[:-1]) if variant == FA1 else None
    return dev.flash_attn_fwd(q, t[1], t[2], causal=causal, variant=variant, out=_nan(q.shape), l=_nan(q.shape[:-1]), m=m, opts=opts)


def run_bwd(dev, t, f, causal, variant=FA2, opts=None):
    q = t[0]
    return dev.flash_attn_bwd(q, t[1], t[2], f[0], t[3], f[1], f[2], causal=causal, variant=variant,
                              grads=tuple(_nan(q.shape) for _ in range(3)), opts=opts)


def run(dev, t, causal, variant=FA2, opts=None):
    f = run_fwd(dev, t, causal, variant, opts)
    return {"f": f, "g": run_bwd(dev, t, f, causal, variant, opts)}


def tensors(res, variant=FA2):
    """name -> tensor of one run; L is FA-2's l or FA-1's m + log l."""
    import torch
    o, l, m = res["f"]
    out = {"o": o, "L": l if variant == FA2 else m + torch.log(l)}
    if variant == FA1:
        out["m"] = m
    if "g" in res:
        out.update(zip(("dq", "dk", "dv"), res["g"]))
    return out


def check_oracle(label, res, ref, tol, heads=None, variant=FA2):
    """Every output finite on every head; the heads `heads` (all by default) within tol of the oracle.  Prints each figure first."""
    import torch
    bad = []
    for nm, got in tensors(res, variant).items():
        if not bool(torch.isfinite(got).all()):
            bad.append((nm, "not finite"))
            continue
        sel = got if heads is None else got[torch.tensor(list(heads), device=got.device)]
        err = maxabs(to_np(sel), ref[nm])
        print(f"ERR {label} {nm} {err:.3e} tol {tol:.0e}")
        if not err < tol:
            bad.append((nm, err))
    assert not bad, (label, bad)


def diff(a, b):
    return float((a - b).abs().max())


def check_close(label, ra, rb, tol, names=None, variant=FA2):
    ta, tb = tensors(ra, variant), tensors(rb, variant)
    bad = []
    for nm in names or ta.keys():
        e = diff(ta[nm], tb[nm])
        print(f"DIFF {label} {nm} {e:.3e} tol {tol:.0e}")
        if not e < tol:   # (NaN fails too)
            bad.append((nm, e))
    assert not bad, (label, bad)


def check_equal(label, ra, rb, names, variant=FA2):
    import torch
    ta, tb = tensors(ra, variant), tensors(rb, variant)
    bad = [nm for nm in names if not torch.equal(ta[nm], tb[nm])]
    assert not bad, (label, "not bit for bit", bad)


# ================================================================ group 1: block, stage and tail boundaries, batch*head = 2
G1_CASES = [(dt, d, N) for dt, d in FAMILIES
            for N in ((255, 256, 257, 512, 513, 768, 1000, 1280, 2048) if dt == "bf16" else (257, 384, 513, 1000, 1280))]


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype,d,N", G1_CASES)
def test_block_stage_and_tail_boundaries(dev, dtype, d, N, causal):
    """Forward + backward at batch*head = 2, every head against the oracle.
    bf16 (256-key dK/dV workgroups, 256-query dQ / slot-forward workgroups at d = 128, 64 / 128-query stages): one to eight key blocks,
    ragged tails, the causal diagonal inside a stage.  d = 128 runs the default (guarded) call and OPTS_EXACT_SCALE, whose forward is
    the phased kernel and whose causal backward keeps the split-operand follow-up launches (the d = 128 backward scales in fp32 either
    way: the same kernels).  fp32 (128-key blocks, paired under the mask): an odd and an even number of blocks, a ragged last one.
    N = 513, 1000: FA-1 side outputs too.  N = 1000, 1280: the separate preprocess kernel (option 4 = 1) against the default: the
    arithmetic is NOT identical (bwd_prep_kernel sums a row's dO * O in 8-element pieces per lane and a butterfly over d / 8 lanes,
    the dQ launch's own preprocess in two interleaved halves and one exchange: delta differs in its last bits), so within the tolerance.
    Forward builds against each other: without the mask and N % 64 == 0 against option 1 = 2 (phased); under it and N % 256 == 0
    against option 1 = 3 (the causal slot forward).  Both sides are within tol of the oracle on every head (checked here), so within
    2 tol of each other by that alone; asserted at tol.  bf16 d = 32 has the phased forward only: the same launch, bit for bit."""
    BH, tol = 2, _tol(dtype)
    arrs, t = make_inputs(dtype, (BH, N, d), 5000 + 7 * N + d)
    ref = oracle_heads(*arrs, causal, range(BH))
    tag = f"g1 {dtype} d{d} N{N} c{int(causal)}"
    calls = [("default", None)] + ([("exact", dev.OPTS_EXACT_SCALE)] if (dtype, d) == ("bf16", 128) else [])
    res = {}
    for name, opts in calls:
        assert_plan(dev, dtype, d, BH, N, causal, FA2, opts)
        res[name] = run(dev, t, causal, FA2, opts)
        check_oracle(f"{tag} {name}", res[name], ref, tol)
    if "exact" in res:
        assert planned(dev, dtype, d, BH, N, causal, FA2, 0, dev.OPTS_EXACT_SCALE) == ["fwd_kernel"] * (2 if causal else 1)
    if N in (513, 1000):
        assert_plan(dev, dtype, d, BH, N, causal, FA1, None)
        check_oracle(f"{tag} fa1", run(dev, t, causal, FA1), ref, tol, variant=FA1)
    if N in (1000, 1280):
        assert_plan(dev, dtype, d, BH, N, causal, FA2, OPT_PREP)
        sep = {"f": res["default"]["f"], "g": run_bwd(dev, t, res["default"]["f"], causal, FA2, OPT_PREP)}
        check_oracle(f"{tag} prep", sep, ref, tol)
        check_close(f"{tag} prep-vs-default", sep, res["default"], tol, ("dq", "dk", "dv"))
    if dtype == "bf16":
        other = (0, 2) if (not causal and N % 64 == 0) else (0, 3) if (causal and N % 256 == 0) else None
        if other is not None:
            want = expect_fwd(dtype, d, BH, N, causal, FA2, other)
            assert planned(dev, dtype, d, BH, N, causal, FA2, 0, other) == want
            if d == 128:   # (0, 2): phased against the default's slot kernel; (0, 3): the causal slot kernel against the default's phased one
                assert want[0] == ("fwd_kernel" if other == (0, 2) else "fwd_slot_kernel")
            fo = {"f": run_fwd(dev, t, causal, FA2, other)}
            check_oracle(f"{tag} fwd{other[1]}", fo, ref, tol)
            if d == 128:
                check_close(f"{tag} fwd{other[1]}-vs-default", fo, {"f": res["default"]["f"]}, tol)
            else:
                check_equal(f"{tag} fwd{other[1]}", fo, {"f": res["default"]["f"]}, ("o", "L"))


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("N", [63, 64, 65, 96, 127, 128])
@pytest.mark.parametrize("d", [128, 32])
def test_rows_with_few_keys(dev, d, N, causal):
    """bf16 rows with fewer than 64 admissible keys feed P / dS to the second product as two bf16 fragments.  Without the mask N = 63 is
    the whole-launch split-operand build of all three kernels (separate preprocess kernel), N >= 64 the main builds (d = 128: the
    8-wave dQ build, the slot forward at N = 64, 128).  Under it the thin dK/dV main launch skips queries 0..63 and the split-operand
    launch behind it adds their contribution alone (N = 64: every query; N = 65: all but one), the forward and dQ redo query block 0."""
    BH = 2
    arrs, t = make_inputs("bf16", (BH, N, d), 6000 + 3 * N + d)
    ref = oracle_heads(*arrs, causal, range(BH))
    assert_plan(dev, "bf16", d, BH, N, causal)
    if N < 64:
        assert planned(dev, "bf16", d, BH, N, causal, FA2, dev.STAGE_ALL, None) == ["bwd_prep_kernel", "bwd_dkdv_kernel", "bwd_dq_kernel"]
    check_oracle(f"g1few bf16 d{d} N{N} c{int(causal)}", run(dev, t, causal), ref, TOLBF)


@pytest.mark.parametrize("dtype,d", FAMILIES)
def test_bnhd_layout_matches_permuted_copy(dev, dtype, d):
    """[B][N][H][d] in place (B = 2, H = 3, N = 1000, causal) against the [B][H][N][d] call on the permuted copy: the kernels take
    the row and head strides as arguments and do the same arithmetic in the same order (none of these families adds with atomics),
    so bit for bit; two heads against the oracle."""
    import torch
    B, H, N = 2, 3, 1000
    arrs, t = make_inputs(dtype, (B, N, H, d), 6500 + d)
    perm = lambda x: x.permute(0, 2, 1, 3).contiguous()
    assert_plan(dev, dtype, d, B * H, N, True)
    o, l, m = dev.flash_attn_fwd_bnhd(*t[:3], True)
    g = dev.flash_attn_bwd_bnhd(*t[:3], o, t[3], l, m, True)
    p = [perm(x) for x in t]
    o_r, l_r, m_r = dev.flash_attn_fwd(*p[:3], True)
    g_r = dev.flash_attn_bwd(*p[:3], o_r, p[3], l_r, m_r, True)
    assert torch.equal(perm(o), o_r) and torch.equal(l, l_r)
    for nm, a, b in zip(("dq", "dk", "dv"), g, g_r):
        assert torch.equal(perm(a), b), nm
    heads = [0, B * H - 1]
    flat = [a.transpose(0, 2, 1, 3).reshape(B * H, N, d) for a in arrs]
    ref = oracle_heads(*flat, True, heads)
    res = {"f": (perm(o).view(B * H, N, d), l.view(B * H, N), None), "g": tuple(perm(x).view(B * H, N, d) for x in g)}
    check_oracle(f"g1bnhd {dtype} d{d}", res, ref, _tol(dtype), heads)


# ================================================================ group 2: block order over many heads, causal, option 7 = 0, 1, 2
def _cus():
    import torch
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def rank_chunk(wgs_per_cu, nb):
    """csrc/fa_api.hip: heads per XCD whose blocks a ranked launch dispatches together."""
    return max(1, _cus() * wgs_per_cu // (4 * nb))


def order_shape(kind):
    """(batch*head, N) of the four block-order cases, from the device's CU count (256 CUs: the figures in brackets).
    rank_chunk(1, N / 256) == rank_chunk(2, N / 128) for every N here (the same quotient), C below."""
    if kind == "six_plus_two":     # (64, 2560): 8 heads per XCD in chunks of C = 6: a last chunk of two heads
        return 8 * (rank_chunk(1, 10) + 2), 2560
    if kind == "twelve_plus_one":  # (104, 1280): 13 heads per XCD in chunks of C = 12: a last chunk of ONE head
        return 8 * (rank_chunk(1, 5) + 1), 1280
    if kind == "not_by_eight":     # the map's other branch: block b of every head, head by head
        return 5, 768
    assert kind == "one_short_chunk"   # 3 heads per XCD, fewer than one chunk (32)
    return 24, 512


ALL_SHAPES = ("six_plus_two", "twelve_plus_one", "not_by_eight", "one_short_chunk")

# Per launch: dtype, d, the options in front of option 7, and the ranked kernels of the launch as (workgroups per CU, rows per block)
# of their rank_chunk: each must leave a partial last chunk at the first two shapes.
#   bf16 d = 128   slot causal forward (the default at the first two shapes, forced by option 1 = 3 at all four) and the unpaired dK/dV
#                  launch DKDV_PLAIN: rank_chunk(1, N / 256); phased forward (the last two shapes) and phased dQ, ranked under
#                  option 7 = 2 only: rank_chunk(2, N / 128).  (The dK/dV follow-up launch is never ranked.)
#   bf16 d = 32    phased forward and dQ, ranked by default: rank_chunk(2, N / 128).  dK/dV is DKDV_PAIRED: no ranked map.
#   fp32 d = 32, 128   phased forward and dQ under option 7 = 2: rank_chunk(2, N / 128).  dK/dV is paired.
#   bf16 d = 64, options (5, 3, 3): dQ slot causal and dK/dV slot causal (always ranked): rank_chunk(1, N / 256).  The forward slot
#                  kernel takes rank_chunk(2, N / 256), twice that: 12 and 25 against 8 and 13 heads per XCD, NO partial chunk there.
#   fp32 d = 64    the one-pass backward (ranked whatever option 7 says): rank_chunk(1, N / 256); phased forward under option 7 = 2:
#                  rank_chunk(2, N / 128).  Option 4 = 4: DKDV_F32_64 (ranked unless option 7 = 1) and the phased dQ (7 = 2):
#                  rank_chunk(2, N / 128).
LAUNCHES = {
    "bf16-d128": ("bf16", 128, (), [(1, 256), (2, 128)]),
    "bf16-d32": ("bf16", 32, (), [(2, 128)]),
    "f32-d32": ("f32", 32, (), [(2, 128)]),
    "f32-d128": ("f32", 128, (), [(2, 128)]),
    "bf16-d64-slot": ("bf16", 64, (5, 3, 3), [(1, 256)]),
    "f32-d64-onepass": ("f32", 64, (), [(1, 256), (2, 128)]),
    "f32-d64-two-kernels": ("f32", 64, (0, 0, 0, 0, 4), [(2, 128)]),
}
G2_CASES = [(name, kind) for name in LAUNCHES
            for kind in (ALL_SHAPES if name in ("bf16-d128", "bf16-d32", "f32-d32") else ALL_SHAPES[:2])]


def _g2_plan_and_bitwise(launch, dtype, d, BH, N):
    """(forward plan, backward plan, {output: the explicit order whose launch the default (option 7 = 0) IS}, outputs that are bit for
    bit the same under all three orders).  The backward of every order reads the forward of order 0, so its inputs are the same.
    Bit for bit under every order: dk, dv of every launch but the one-pass kernel's (only the workgroup-to-block map differs, or
    nothing at all), and o, L, dq of the PHASED forward and dQ kernels: their paired launch runs the one loop body of the ranked launch
    twice per workgroup, every per-block variable declared inside it (fwd_kernel, bwd_dq_kernel: `for (int pass ...`).  The slot
    kernels' paired and ranked builds are held to the tolerance."""
    nqb = N // 256
    everything = ("o", "L", "dq", "dk", "dv")
    if launch == "bf16-d64-slot":
        # causal_ranked: ranked while the launch is below 8 rounds of the chip; the dK/dV causal slot kernel is ranked always
        same = {"o": 2 if BH * nqb < 16 * _cus() else 1, "dq": 2 if BH * nqb < 8 * _cus() else 1}
        return ["fwd_slot_kernel", "fwd_kernel"], ["bwd_dq_slot_kernel", "bwd_dkdv_slot_kernel"], same, ("dk", "dv")
    if launch == "f32-d64-onepass":   # dq (and dk, dv of a cut sweep) are sums of atomics: no bitwise claim on the gradients
        return ["fwd_kernel"], ["bwd_prep_kernel", "bwd_onepass_f32_kernel"], {"o": 1}, ("o", "L")
    if launch == "f32-d64-two-kernels":   # DKDV_F32_64 ranked or head by head: "bitwise the same" (select_dkdv)
        return ["fwd_kernel"], ["bwd_prep_kernel", "bwd_dkdv_kernel", "bwd_dq_kernel"], {"o": 1, "dq": 1}, everything
    fwd, bwd = expect_fwd(dtype, d, BH, N, True), expect_bwd(dtype, N, True)
    if launch == "bf16-d128":   # DKDV_PLAIN ranked (0, 2) or head by head (1): one block per workgroup either way
        slot = fwd[0] == "fwd_slot_kernel"
        return fwd, bwd, {"o": (2 if BH * nqb < 8 * _cus() else 1) if slot else 1, "dq": 1}, ("dq", "dk", "dv") if slot else everything
    # phased forward / dQ: ranked by default at bf16 d = 32 alone; DKDV_PAIRED has no ranked map: the same launch three times
    return fwd, bwd, {"o": 2 if launch == "bf16-d32" else 1, "dq": 2 if launch == "bf16-d32" else 1}, everything


@pytest.mark.parametrize("launch,kind", G2_CASES)
def test_block_order_over_many_heads(dev, launch, kind):
    """Causal launches whose ranked map (map_block_ranked, csrc/fa_atoms.h) meets a partial last chunk per XCD (6 + 2 and 12 + 1 heads on
    256 CUs), batch*head not a multiple of 8, and fewer heads per XCD than one chunk; option 7 = 0, 1 and 2.  A wrong head or block
    in the map computes one block twice and another never: NaN rows here.  EVERY head: the three orders within the tolerance of each
    other; bit for bit where the default is the launch of an explicit order and wherever only the workgroup-to-block map differs
    (dk, dv: the unpaired launches of bf16 d = 128 and fp32 d = 64, the paired and always-ranked ones of the rest; o, L, dq of the
    phased kernels: _g2_plan_and_bitwise).  Three heads against the oracle, under every order: the first, one from the partial last
    chunk of XCD 3, the last."""
    dtype, d, base, chunks = LAUNCHES[launch]
    BH, N = order_shape(kind)
    per, tol = BH // 8, _tol(dtype)
    cs = [rank_chunk(w, N // rows) for w, rows in chunks]
    if kind in ("six_plus_two", "twelve_plus_one"):
        for C in cs:
            assert BH % 8 == 0 and per > C and per % C == (2 if kind == "six_plus_two" else 1), (BH, per, C)
        mid = 3 * per + (per // cs[0]) * cs[0]   # first head of XCD 3's partial chunk
    elif kind == "not_by_eight":
        assert BH % 8 != 0
        mid = BH // 2
    else:
        for C in cs:
            assert BH % 8 == 0 and per < C, (BH, per, C)
        mid = BH // 2
    heads = [0, mid, BH - 1]
    fwd_plan, bwd_plan, same, bitwise = _g2_plan_and_bitwise(launch, dtype, d, BH, N)
    arrs, t = make_inputs(dtype, (BH, N, d), 7000 + BH + N + d)
    ref = oracle_heads(*arrs, True, heads)
    res = {}
    for order in (0, 1, 2):
        opts = _with(base, 7, order)
        assert_plan(dev, dtype, d, BH, N, True, FA2, opts, fwd_plan, bwd_plan)
        f = run_fwd(dev, t, True, FA2, opts)
        res[order] = {"f": f, "g": run_bwd(dev, t, res[0]["f"] if order else f, True, FA2, opts)}
    tag = f"g2 {launch} BH{BH} N{N}"
    for order in (0, 1, 2):
        check_oracle(f"{tag} order{order}", res[order], ref, tol, heads)
    for order in (1, 2):
        check_close(f"{tag} order{order}-vs-0", res[order], res[0], tol)
    check_equal(f"{tag} default is order {same['o']}", res[0], res[same["o"]], ("o", "L"))
    if "dq" in same:
        check_equal(f"{tag} default is order {same['dq']}", res[0], res[same["dq"]], ("dq",))
    for order in (1, 2):
        check_equal(f"{tag} order {order} vs 0", res[order], res[0], bitwise)
    if launch == "bf16-d128":   # the causal slot forward forced onto every shape, paired (1) and ranked (2)
        slot = {}
        for order in (1, 2):
            opts = (0, 3, 0, 0, 0, 0, 0, order)
            assert planned(dev, dtype, d, BH, N, True, FA2, 0, opts) == ["fwd_slot_kernel", "fwd_kernel", "fwd_kernel"]
            slot[order] = {"f": run_fwd(dev, t, True, FA2, opts)}
            check_oracle(f"{tag} slotfwd order{order}", slot[order], ref, tol, heads)
        check_close(f"{tag} slotfwd 1-vs-2", slot[1], slot[2], tol)
        check_close(f"{tag} slotfwd-vs-default", slot[2], {"f": res[0]["f"]}, tol)


# ================================================================ group 3: default dispatch of bf16 d = 128 around batch * ceil(N / 256) = 256
@pytest.mark.parametrize("BH,N,causal", [(127, 512, True), (128, 512, True), (32, 2048, True), (127, 512, False), (128, 512, False)])
def test_d128_default_dispatch_around_launch_size_threshold(dev, BH, N, causal):
    """Under the causal mask the forward takes the causal slot build from batch * ceil(N / 256) = 256 on (254: the phased kernel and
    its split-operand follow-up; 256, by many heads or by many blocks: the slot kernel); without the mask the slot kernel on both
    sides.  Every head against the phased kernels (OPTS_PHASED) within TOLBF, the first and the last head against the oracle."""
    from flash_attention_minitorch_amd import _lib
    d = 128
    fold = _lib.plan(BH, N, d, causal, FA2, _lib.FA_DTYPE_BF16, 0, dev.OPTS_FOLDED_SCALE)
    slot = not causal or BH * ((N + 255) // 256) >= 256
    assert fold == (["fwd_slot_kernel"] if slot else ["fwd_kernel", "fwd_kernel"]), fold
    assert_plan(dev, "bf16", d, BH, N, causal)
    assert_plan(dev, "bf16", d, BH, N, causal, FA2, dev.OPTS_PHASED, ["fwd_kernel"] * (2 if causal else 1))
    arrs, t = make_inputs("bf16", (BH, N, d), 8000 + BH + N)
    tag = f"g3 BH{BH} N{N} c{int(causal)}"
    default, phased = run(dev, t, causal), run(dev, t, causal, FA2, dev.OPTS_PHASED)
    heads = [0, BH - 1]
    ref = oracle_heads(*arrs, causal, heads)
    check_oracle(f"{tag} default", default, ref, TOLBF, heads)
    check_oracle(f"{tag} phased", phased, ref, TOLBF, heads)
    check_close(f"{tag} default-vs-phased", default, phased, TOLBF)
