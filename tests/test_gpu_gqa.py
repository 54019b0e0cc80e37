"""Grouped-query (GQA / MQA) heads in the forward, dQ and dK/dV kernels on the GPU (fa_mi355x_fwd_gqa / _bwd_gqa through
device_ops.flash_attn_*_gqa), at the smallest shapes that reach each kernel family, against two references:

1. the fp64 oracle per query head on the expanded inputs (dK, dV summed over each group in fp64).  Bounds: the project's envelope
   (README.md), 1e-3 max-abs for bf16 and 1e-4 for fp32 on O, L and dQ; G times that on dK and dV, a group's gradient being the sum of
   G per-head gradients that are each within the envelope.
2. the library itself on k and v repeated G times along the head axis (the ungrouped entry points): out, l and dq bit for bit (a query
   head runs the same arithmetic on the same numbers, only fetched from another address), dk and dv against the fp64 sum over the
   group of the ungrouped call's per-head dk, dv within G * 2^-23 * sum_g |term| elementwise, the rounding of an ordered fp32 sum of
   G terms.
Inputs are U(-1, 1) (rand_u), bf16-rounded for bf16."""
import math

import numpy as np
import pytest

import oracle
from gpu_util import maxabs, rand_u, to_np

pytestmark = pytest.mark.gpu

GROUPINGS = {"B2H8kv2": (2, 8, 2),    # B * H a multiple of 8: map_block's XCD branch
             "B1H6kv1": (1, 6, 1)}    # multi-query, odd G, the other map_block branch
FORCE_CAUSAL_SLOT = (5, 3, 3)         # options [0] = 5, [1] = 3, [2] = 3: the causal slot builds of dK/dV, forward and dQ
# name -> (dtype, d, N, causal, options, layouts, forward plan, backward plan): the plans are those of a guarded call (option 8 = 3), which
# is what the default guard = "auto" makes; they tell the kernel families apart, not the builds within one
SHAPES = {
    "bf16_d64_n256": ("bf16", 64, 256, False, None, ("bnhd", "bhnd"), "fwd_slot_kernel;fwd_kernel",
                      "bwd_dq_slot_kernel;bwd_dkdv_slot_kernel;group_sum_kernel"),
    "bf16_d64_n200_ragged": ("bf16", 64, 200, False, None, ("bnhd",), "fwd_slot_kernel",
                             "bwd_prep_kernel;bwd_dkdv_slot_kernel;group_sum_kernel;bwd_dq_slot_kernel"),
    "bf16_d64_n256_causal": ("bf16", 64, 256, True, None, ("bnhd", "bhnd"), "fwd_kernel",
                             "bwd_dq_kernel;bwd_dq_kernel;bwd_dkdv_kernel;group_sum_kernel"),
    "bf16_d64_n256_causal_slot": ("bf16", 64, 256, True, FORCE_CAUSAL_SLOT, ("bnhd",), "fwd_slot_kernel;fwd_kernel",
                                  "bwd_dq_slot_kernel;bwd_dkdv_slot_kernel;group_sum_kernel"),
    "bf16_d128_n256": ("bf16", 128, 256, False, None, ("bnhd", "bhnd"), "fwd_slot_kernel;fwd_kernel",
                       "bwd_dq_kernel;bwd_dkdv_kernel;group_sum_kernel"),
    "bf16_d128_n256_causal": ("bf16", 128, 256, True, None, ("bnhd",), "fwd_kernel;fwd_kernel",
                              "bwd_dq_kernel;bwd_dq_kernel;bwd_dkdv_kernel;bwd_dkdv_kernel;group_sum_kernel"),
    "bf16_d32_n96_causal": ("bf16", 32, 96, True, None, ("bnhd", "bhnd"), "fwd_kernel;fwd_kernel",
                            "bwd_dq_kernel;bwd_dq_kernel;bwd_dkdv_kernel;bwd_dkdv_kernel;group_sum_kernel"),
    "bf16_d64_n40_few_keys": ("bf16", 64, 40, False, None, ("bnhd",), "fwd_kernel",
                              "bwd_prep_kernel;bwd_dkdv_kernel;group_sum_kernel;bwd_dq_kernel"),
    "f32_d64_n256": ("f32", 64, 256, False, None, ("bnhd", "bhnd"), "fwd_splitk_f32_kernel", "bwd_dq_kernel;bwd_dkdv_kernel;group_sum_kernel"),
    "f32_d64_n256_causal": ("f32", 64, 256, True, None, ("bnhd", "bhnd"), "fwd_splitk_f32_kernel",
                            "bwd_dq_kernel;bwd_dkdv_kernel;group_sum_kernel"),
    "f32_d32_n100": ("f32", 32, 100, False, None, ("bnhd",), "fwd_kernel", "bwd_dq_kernel;bwd_dkdv_kernel;group_sum_kernel"),
}
CASES = [(s, g, lay) for s in SHAPES for g in GROUPINGS for lay in SHAPES[s][5]]
ENVELOPE = {"bf16": 1e-3, "f32": 1e-4}


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _plans(B, H, Hkv, N, d, causal, dtype, opts, variant=2):
    from flash_attention_minitorch_amd import _lib
    o = (tuple(opts or ()) + (0,) * 8)[:8] + (3,)
    code = _lib.FA_DTYPE_BF16 if dtype == "bf16" else _lib.FA_DTYPE_F32
    return tuple(";".join(_lib.plan_gqa(B, H, Hkv, N, d, causal, variant, code, st, o)) for st in (0, 7))


def _same_kernel_opts(B, H, N, d, causal, dtype, opts):
    """The options of the ungrouped call that names the grouped call's kernels: where it would take the fp32 one-pass backward, a
    grouped call runs what option 4 = 4 selects."""
    from flash_attention_minitorch_amd import _lib
    code = _lib.FA_DTYPE_BF16 if dtype == "bf16" else _lib.FA_DTYPE_F32
    if "bwd_onepass_f32_kernel" in _lib.plan(B * H, N, d, causal, _lib.FA_VARIANT_FA2, code, 7, opts):
        return (tuple(opts or ()) + (0,) * 5)[:4] + (4,)
    return opts


def _oracle(q, k, v, do, causal, kv_heads=None):
    """The fp64 oracle of a grouped call, numpy q, do (B, H, N, d) and k, v (B, Hkv, N, d), on the whole groups ``kv_heads`` (indices
    into the flattened (B, Hkv); None: all of them, in order).  Per group, in that order: o, dq (n, G, N, d) and L, m (n, G, N) per
    query head, dk, dv (n, N, d) summed over the group's G heads in fp64."""
    B, H, N, d = q.shape
    Hkv = k.shape[1]
    G = H // Hkv
    qg, dog = q.reshape(B * Hkv, G, N, d), do.reshape(B * Hkv, G, N, d)
    kf, vf = k.reshape(B * Hkv, 1, N, d), v.reshape(B * Hkv, 1, N, d)
    per = {n: [] for n in ("o", "L", "m", "dq", "dk", "dv")}
    for i in (range(B * Hkv) if kv_heads is None else kv_heads):
        o, L, m, _ = oracle.dense_attention_fw(qg[i], kf[i], vf[i], causal)
        dq, dk, dv = oracle.dense_attention_bw(qg[i], kf[i], vf[i], dog[i], causal)
        for n, a in zip(("o", "L", "m", "dq", "dk", "dv"), (o, L, m, dq, dk.sum(axis=0), dv.sum(axis=0))):
            per[n].append(np.asarray(a, dtype=np.float64))
    return {n: np.stack(a) for n, a in per.items()}


_INPUTS = {}


def _inputs(shape, grouping):
    """numpy q, do (B, H, N, d), k, v (B, Hkv, N, d) of a case and, computed once and shared by its layouts and tests, the fp64 oracle
    per query head: o, L, dq (B, H, ..) and dk, dv summed over each group (B, Hkv, N, d)."""
    key = (shape, grouping)
    if key not in _INPUTS:
        dtype, d, N, causal = SHAPES[shape][:4]
        B, H, Hkv = GROUPINGS[grouping]
        G = H // Hkv
        rng = np.random.default_rng(1000 + 17 * list(SHAPES).index(shape) + list(GROUPINGS).index(grouping))
        q, do = rand_u(rng, (B, H, N, d)), rand_u(rng, (B, H, N, d))
        k, v = rand_u(rng, (B, Hkv, N, d)), rand_u(rng, (B, Hkv, N, d))
        if dtype == "bf16":
            q, k, v, do = (oracle.bf16_round(t) for t in (q, k, v, do))
        per = _oracle(q, k, v, do, causal)
        ref = {n: per[n].reshape((B, H) + per[n].shape[2:]) for n in ("o", "L", "dq")}
        ref.update({n: per[n].reshape(B, Hkv, N, d) for n in ("dk", "dv")})
        _INPUTS[key] = (q, k, v, do, ref)
    return _INPUTS[key]


def _dev(a, layout, dtype):
    """A (B, heads, N, d) numpy array as a contiguous device tensor in ``layout``."""
    torch = _torch()
    t = torch.from_numpy(a).to("cuda", torch.bfloat16 if dtype == "bf16" else torch.float32)
    return t.permute(0, 2, 1, 3).contiguous() if layout == "bnhd" else t.contiguous()


def _bhnd(t, layout):
    return to_np(t.permute(0, 2, 1, 3) if layout == "bnhd" else t)


def _expand(t, G, layout):
    return t.repeat_interleave(G, dim=2 if layout == "bnhd" else 1).contiguous()


def _grouped(tq, tk, tv, tdo, causal, layout, opts, variant=2, softmax_scale=None, guard="auto"):
    """(out, l, dq, dk, dv) of the grouped forward and backward; with variant = FA-1 also m, behind them.  ``guard``: "auto", None, or a
    tensor that both calls read."""
    from flash_attention_minitorch_amd import device_ops
    out, l, m = device_ops.flash_attn_fwd_gqa(tq, tk, tv, causal=causal, variant=variant, softmax_scale=softmax_scale, layout=layout,
                                              guard=guard, opts=opts)
    dq, dk, dv = device_ops.flash_attn_bwd_gqa(tq, tk, tv, out, tdo, l, m, causal=causal, variant=variant, softmax_scale=softmax_scale,
                                               layout=layout, guard=guard, opts=opts)
    return (out, l, dq, dk, dv) + (() if m is None else (m,))


def _ungrouped(tq, tk, tv, tdo, causal, layout, opts, variant=2, softmax_scale=None, guard="auto"):
    """The existing by-heads entry points (fa_mi355x_fwd_guarded / _bwd_guarded) on tensors of one shape; results as _grouped."""
    from flash_attention_minitorch_amd import device_ops
    if layout == "bnhd":
        out, l, m = device_ops.flash_attn_fwd_bnhd(tq, tk, tv, causal, variant, softmax_scale, guard=guard, opts=opts)
        g = device_ops.flash_attn_bwd_bnhd(tq, tk, tv, out, tdo, l, m, causal=causal, variant=variant, softmax_scale=softmax_scale,
                                           guard=guard, opts=opts)
    elif softmax_scale is None:
        out, l, m = device_ops.flash_attn_fwd(tq, tk, tv, causal, variant, opts=opts, guard=guard)
        g = device_ops.flash_attn_bwd(tq, tk, tv, out, tdo, l, m, causal=causal, variant=variant, opts=opts, guard=guard)
    else:   # (the public (B, H, N, d) calls take no scale: the call path they share with the (B, N, H, d) ones does)
        out, l, m = device_ops._fwd(device_ops._BHND, tq, tk, tv, causal, variant, softmax_scale, opts, guard=guard)
        g = device_ops._bwd(device_ops._BHND, tq, tk, tv, out, tdo, l, m, causal, variant, softmax_scale, opts, guard=guard)
    return (out, l) + tuple(g) + (() if m is None else (m,))


def _check_group_sum(got, per_head, G, layout, what):
    """``got`` (kv-shaped) against the fp64 sum over each group of ``per_head`` (q-shaped, the ungrouped call's gradient):
    |got - sum| <= G * 2^-23 * sum_g |term| elementwise, the rounding of an ordered fp32 sum of G terms."""
    if layout == "bnhd":
        B, N, H, d = per_head.shape
        terms = per_head.double().view(B, N, H // G, G, d)
        total, mag = terms.sum(3), terms.abs().sum(3)
    else:
        B, H, N, d = per_head.shape
        terms = per_head.double().view(B, H // G, G, N, d)
        total, mag = terms.sum(2), terms.abs().sum(2)
    err, bound = (got.double() - total).abs(), G * 2.0 ** -23 * mag
    worst = float((err - bound).max())
    print(f"  {what}: max |got - fp64 group sum| {float(err.max()):.3e}, largest bound {float(bound.max()):.3e}")
    assert got.shape == total.shape and worst <= 0.0, (what, worst)


def _against_library(tq, tk, tv, tdo, got, G, causal, layout, opts_ungrouped, variant=2, softmax_scale=None, guard="auto"):
    torch = _torch()
    ref = _ungrouped(tq, _expand(tk, G, layout), _expand(tv, G, layout), tdo, causal, layout, opts_ungrouped, variant, softmax_scale,
                     guard)
    torch.cuda.synchronize()
    assert len(got) == len(ref)
    for name, a, b in zip(("out", "l", "dq"), (got[0], got[1], got[2]), (ref[0], ref[1], ref[2])):
        assert torch.equal(a, b), f"{name} differs from the ungrouped call on expanded k, v"
    if len(got) > 5:   # FA-1: the row maxima
        assert got[5].shape == ref[5].shape and torch.equal(got[5], ref[5]), "m differs from the ungrouped call on expanded k, v"
    _check_group_sum(got[3], ref[3], G, layout, "dk")
    _check_group_sum(got[4], ref[4], G, layout, "dv")


def _check_oracle(got, ref, kv_heads, Hkv, layout, dtype, tag, bound=None):
    """(out, l, dq, dk, dv) of a grouped call against _oracle's ``ref`` on the whole groups ``kv_heads`` (None: all): max-abs error below
    the envelope on o, L and dq and G times it on dk and dv, or ``bound(name, reference)`` in its place.  Returns the errors."""
    B = got[1].shape[0]
    G = got[1].shape[1] // Hkv
    N, d = got[1].shape[2], got[0].shape[-1]
    sel = list(range(B * Hkv) if kv_heads is None else kv_heads)
    have = {"o": _bhnd(got[0], layout).reshape(B * Hkv, G, N, d)[sel], "L": to_np(got[1]).reshape(B * Hkv, G, N)[sel],
            "dq": _bhnd(got[2], layout).reshape(B * Hkv, G, N, d)[sel], "dk": _bhnd(got[3], layout).reshape(B * Hkv, N, d)[sel],
            "dv": _bhnd(got[4], layout).reshape(B * Hkv, N, d)[sel]}
    errs = {n: maxabs(a, ref[n]) for n, a in have.items()}
    env = ENVELOPE[dtype]
    lim = {n: (bound(n, ref[n]) if bound else env) * (G if n in ("dk", "dv") else 1) for n in have}
    print(f"{tag} ({len(sel)} groups of {G}): " + ", ".join(f"{n} {e:.3e} (< {lim[n]:.1e})" for n, e in errs.items()))
    for n, a in have.items():
        assert np.all(np.isfinite(a)), (tag, n)
        assert errs[n] < lim[n], (tag, n, errs[n], lim[n])
    return errs


@pytest.mark.parametrize("shape,grouping,layout", CASES, ids=[f"{s}-{g}-{lay}" for s, g, lay in CASES])
def test_grouped_forward_and_backward(shape, grouping, layout):
    torch = _torch()
    dtype, d, N, causal, opts, _, plan_fwd, plan_bwd = SHAPES[shape]
    B, H, Hkv = GROUPINGS[grouping]
    G = H // Hkv
    assert _plans(B, H, Hkv, N, d, causal, dtype, opts) == (plan_fwd, plan_bwd)
    q, k, v, do, ref = _inputs(shape, grouping)
    tq, tk, tv, tdo = (_dev(a, layout, dtype) for a in (q, k, v, do))
    got = _grouped(tq, tk, tv, tdo, causal, layout, opts)
    torch.cuda.synchronize()
    assert got[0].shape == tq.shape and got[2].shape == tq.shape and got[3].shape == tk.shape and got[4].shape == tv.shape
    assert tuple(got[1].shape) == (B, H, N)
    # reference 1: the fp64 oracle
    env = ENVELOPE[dtype]
    errs = {"o": maxabs(_bhnd(got[0], layout), ref["o"]), "L": maxabs(to_np(got[1]), ref["L"]), "dq": maxabs(_bhnd(got[2], layout), ref["dq"]),
            "dk": maxabs(_bhnd(got[3], layout), ref["dk"]), "dv": maxabs(_bhnd(got[4], layout), ref["dv"])}
    print(f"{shape} {grouping} {layout}: " + ", ".join(f"{n} {e:.3e}" for n, e in errs.items()) + f" (envelope {env:.0e}, dk / dv x {G})")
    for n, e in errs.items():
        assert e < (G * env if n in ("dk", "dv") else env), (n, e)
    # reference 2: the library on expanded k, v
    _against_library(tq, tk, tv, tdo, got, G, causal, layout, _same_kernel_opts(B, H, N, d, causal, dtype, opts))


def test_the_shape_of_the_tiled_builds():
    """bf16, d = 64, N = 256, non-causal, B = 8, H = 64, Hkv = 16: an ungrouped call of this size runs the tiled dQ and dK/dV builds
    (head_tiles: 2 consecutive heads per workgroup).  Their head-to-head hand-over keeps K and V where q lives, so a grouped call
    takes the one-head-per-workgroup builds instead ("Grouped-query heads", exclusions): compared against the library on
    expanded k, v with option 5 = 1, which names those builds.  Against the library only."""
    torch = _torch()
    B, H, Hkv, N, d = 8, 64, 16, 256, 64
    assert _plans(B, H, Hkv, N, d, False, "bf16", None) == SHAPES["bf16_d64_n256"][6:]
    g = torch.Generator(device="cuda").manual_seed(5)
    tq, tdo = (torch.rand((B, N, H, d), generator=g, device="cuda").mul_(2).sub_(1).to(torch.bfloat16) for _ in range(2))
    tk, tv = (torch.rand((B, N, Hkv, d), generator=g, device="cuda").mul_(2).sub_(1).to(torch.bfloat16) for _ in range(2))
    got = _grouped(tq, tk, tv, tdo, False, "bnhd", None)
    _against_library(tq, tk, tv, tdo, got, H // Hkv, False, "bnhd", (0, 0, 0, 0, 0, 1))


@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("shape", ["bf16_d64_n256", "f32_d64_n256_causal"])
def test_k_with_all_heads_is_the_ungrouped_call_bit_for_bit(shape, layout):
    """Hkv == H: the _gqa entry points are fa_mi355x_fwd_guarded / _bwd_guarded, all five outputs bit for bit."""
    torch = _torch()
    dtype, d, N, causal, opts = SHAPES[shape][:5]
    B, H, _ = GROUPINGS["B2H8kv2"]
    q, _, _, do, _ = _inputs(shape, "B2H8kv2")
    rng = np.random.default_rng(77)
    k, v = rand_u(rng, q.shape), rand_u(rng, q.shape)
    tq, tk, tv, tdo = (_dev(a, layout, dtype) for a in (q, k, v, do))
    got = _grouped(tq, tk, tv, tdo, causal, layout, opts)
    ref = _ungrouped(tq, tk, tv, tdo, causal, layout, opts)
    torch.cuda.synchronize()
    for name, a, b in zip(("out", "l", "dq", "dk", "dv"), got, ref):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("shape", ["bf16_d64_n256", "bf16_d64_n256_causal", "f32_d64_n256"])
def test_a_repeated_grouped_backward_returns_the_same_bits(shape):
    torch = _torch()
    dtype, d, N, causal, opts = SHAPES[shape][:5]
    q, k, v, do, _ = _inputs(shape, "B1H6kv1")
    tq, tk, tv, tdo = (_dev(a, "bnhd", dtype) for a in (q, k, v, do))
    first = _grouped(tq, tk, tv, tdo, causal, "bnhd", opts)
    for _ in range(2):
        again = _grouped(tq, tk, tv, tdo, causal, "bnhd", opts)
        torch.cuda.synchronize()
        for a, b in zip(first, again):
            assert torch.equal(a, b)


@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("shape", ["bf16_d64_n256", "bf16_d64_n200_ragged", "bf16_d64_n256_causal", "bf16_d128_n256", "f32_d64_n256"])
def test_nothing_outside_k_and_v_is_read(shape, layout):
    """k and v are slices of larger tensors filled with NaN (a q-sized margin on either side): a K / V base, row stride or buffer
    size still formed from H reads the margin.  The results are finite and the bits of the call on plain tensors."""
    torch = _torch()
    dtype, d, N, causal, opts = SHAPES[shape][:5]
    q, k, v, do, _ = _inputs(shape, "B2H8kv2")
    tq, tk, tv, tdo = (_dev(a, layout, dtype) for a in (q, k, v, do))
    plain = _grouped(tq, tk, tv, tdo, causal, layout, opts)

    def inside_nan(t):
        big = torch.full((t.numel() + 2 * tq.numel(),), float("nan"), dtype=t.dtype, device="cuda")
        part = big[tq.numel():tq.numel() + t.numel()].view(t.shape)
        part.copy_(t)
        return part
    got = _grouped(tq, inside_nan(tk), inside_nan(tv), tdo, causal, layout, opts)
    torch.cuda.synchronize()
    for name, a, b in zip(("out", "l", "dq", "dk", "dv"), got, plain):
        assert bool(torch.isfinite(a).all()), name
        assert torch.equal(a, b), name


@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
def test_autograd_returns_gradients_in_each_input_shape_and_dtype(layout):
    """flash_attn_gqa under autograd at the first shape: values against the fp64 oracle.  The gradients are cast to bf16, one rounding
    of at most 2^-8 relative, on top of the envelope (bf16 keeps 8 significant bits, so neighbours in [1, 2) are 2^-7 apart and a value
    just above 1 moves by up to half of that, 2^-8 of itself)."""
    torch = _torch()
    from flash_attention_minitorch_amd import device_ops
    shape, grouping = "bf16_d64_n256", "B2H8kv2"
    dtype, d, N, causal = SHAPES[shape][:4]
    B, H, Hkv = GROUPINGS[grouping]
    G = H // Hkv
    q, k, v, do, ref = _inputs(shape, grouping)
    tq, tk, tv = (_dev(a, layout, dtype).requires_grad_() for a in (q, k, v))
    out = device_ops.flash_attn_gqa(tq, tk, tv, causal=causal, layout=layout)
    out.backward(_dev(do, layout, "f32"))
    torch.cuda.synchronize()
    assert out.dtype is torch.float32 and out.shape == tq.shape
    assert maxabs(_bhnd(out, layout), ref["o"]) < ENVELOPE[dtype]
    for name, t, scale in (("dq", tq, 1), ("dk", tk, G), ("dv", tv, G)):
        assert t.grad.shape == t.shape and t.grad.dtype is torch.bfloat16, name
        err = np.abs(_bhnd(t.grad, layout).astype(np.float64) - ref[name])
        bound = scale * ENVELOPE[dtype] + 2.0 ** -8 * np.abs(ref[name])
        print(f"autograd {layout} {name}: max-abs {err.max():.3e}")
        assert np.all(err < bound), (name, float((err - bound).max()))


@pytest.mark.parametrize("d", [64, 48])
def test_grouped_prefill_keeps_the_bits_of_the_expanded_path(d):
    """attention_stack_prefill of a grouped-query stack: the returned activations and the cache contents are bit for bit what the
    expanded path gives (flash_attn_fwd_bnhd on _expand_kv of the cache-shaped k and v), native d and a padded one."""
    torch = _torch()
    from flash_attention_minitorch_amd import _lib, device_ops, modules_transformer as mt
    rng = np.random.default_rng(31)
    B, H, Hkv, P, L = 2, 8, 2, 200, 2
    E = H * d
    x = torch.from_numpy(rand_u(rng, (B, P, E))).to("cuda", torch.bfloat16)
    w = lambda cols: torch.from_numpy(rand_u(rng, (E, cols)) / np.float32(math.sqrt(E))).to("cuda", torch.bfloat16)
    layers = [(w(E), w(Hkv * d), w(Hkv * d), w(E)) for _ in range(L)]
    cache = mt.KVCache(L, B, 256, H, d, torch.bfloat16, "cuda", n_kv_head=Hkv)
    got = mt.attention_stack_prefill(x, layers, H, cache)
    want_cache = mt.KVCache(L, B, 256, H, d, torch.bfloat16, "cuda", n_kv_head=Hkv)
    y = x
    for li, (wq, wk, wv, wo) in enumerate(layers):
        q, k, v = mt._project(y, wq, wk, wv, H)
        kp, vp = want_cache._pad(k), want_cache._pad(v)
        want_cache.k[li][:, :P] = kp
        want_cache.v[li][:, :P] = vp
        ke, ve = mt._expand_kv(kp, H), mt._expand_kv(vp, H)
        if want_cache.dp == d:
            o, _, _ = device_ops.flash_attn_fwd_bnhd(q, ke, ve, True, _lib.FA_VARIANT_FA2)
        else:
            o, _, _ = device_ops.flash_attn_fwd_bnhd(want_cache._pad(q), ke, ve, True, _lib.FA_VARIANT_FA2, softmax_scale=d ** -0.5)
            o = o[..., :d]
        y = y + (o.reshape(B * P, E).to(y.dtype) @ wo).view(B, P, E)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got).all()) and torch.equal(got, y)
    for li in range(L):
        assert torch.equal(cache.k[li], want_cache.k[li]) and torch.equal(cache.v[li], want_cache.v[li])
    assert int(cache.lengths.min()) == int(cache.lengths.max()) == P
