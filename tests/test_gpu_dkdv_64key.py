"""The four-wave build of the non-causal d = 64 dK/dV slot kernel (fa_bwd_dkdv64.h: 64 keys per wave, K / V fragments and the dK, dV
accumulators in AGPRs, one LDS read per two MFMAs) against the eight-wave build it replaces by default: the same per-key arithmetic and
the same order of the sum over queries, so dk and dv must be BITWISE equal, for both scalings (the scale guard sends U(-1, 1) operands
to the folded-scale sweep and x6 operands to the fp32-scaling one), and within the suite's bf16 bound of the fp64 oracle.  Option 0 = 7
runs the build wherever it is valid, 6 keeps the eight-wave builds.  Shapes: the smallest launch with a workgroup for every CU
(BH * N / 256 = 256), a partial last head group, and at single-workgroup granularity N = 256 (one key block, one stage pair) and 512
with 1, 3 and 5 heads (one head, a partial group, more than one group): where the ring hand-off, the head hand-off and the
wave -> key map can go wrong.  Every launch runs twice and must repeat bit for bit (a ring race shows there)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import oracle  # noqa: E402
from gpu_util import maxabs, oracle_heads, rand_u, to_np  # noqa: E402

NEW, OLD = (7,), (6,)
D = 64
# (BH, N, heads checked against the oracle)
SHAPES = [(64, 1024, (0, 37, 63)), (6, 512, range(6)),
          (1, 256, (0,)), (3, 256, range(3)), (5, 256, range(5)), (1, 512, (0,)), (3, 512, range(3)), (5, 512, range(5))]


@pytest.fixture(scope="module")
def dev():
    import torch
    from flash_attention_minitorch_amd import device_ops
    assert torch.cuda.is_available()
    return device_ops


def _builds(BH, N, causal, opts):
    from flash_attention_minitorch_amd import _lib, device_ops
    return _lib.plan_builds(BH, N, D, causal, _lib.FA_VARIANT_FA2, _lib.FA_DTYPE_BF16, device_ops.STAGE_ALL, opts)


@pytest.mark.parametrize("amp", [1.0, 6.0], ids=["u1-folded", "x6-fp32scale"])
@pytest.mark.parametrize("BH,N,heads", SHAPES, ids=[f"bh{s[0]}-n{s[1]}" for s in SHAPES])
def test_bitwise_equal_to_the_eight_wave_build(dev, BH, N, heads, amp):
    import torch
    rng = np.random.default_rng(6400 + 7 * BH + N)
    arrs = [oracle.bf16_round(amp * rand_u(rng, (BH, N, D))) for _ in range(3)] + [oracle.bf16_round(rand_u(rng, (BH, N, D)))]
    t = [torch.from_numpy(a).to("cuda", torch.bfloat16) for a in arrs]
    assert "DKDV_SLOT64_TILED" in _builds(BH, N, False, NEW) and "DKDV_SLOT64_TILED" not in _builds(BH, N, False, OLD)
    assert (dev.pick_opts(t[0], t[1]) == dev.OPTS_EXACT_SCALE) == (amp > 1.0)   # the guard's side for these operands
    o, L, _ = dev.flash_attn_fwd(*t[:3], False)

    def run(opts):
        _, dk, dv = dev.flash_attn_bwd(*t[:3], o, t[3], L, None, False, opts=opts)   # (guarded: the launch picks its sweep itself)
        return to_np(dk), to_np(dv)

    new1, new2, old = run(NEW), run(NEW), run(OLD)
    for nm, a, b, c in zip(("dk", "dv"), new1, new2, old):
        assert np.array_equal(a, b), (nm, "differs between two launches", maxabs(a, b))
        assert np.array_equal(a, c), (nm, "differs from the eight-wave build", maxabs(a, c))
    heads = list(heads)
    ref = oracle_heads(*arrs, False, heads)
    # U(-1, 1): the suite's bf16 bound, 1e-3 absolute.  x6 operands (scores of order 100, P and dS of order 1 on few keys, whose 2^-9
    # bf16 rounding is averaged over N <= 1024 keys only): the suite's bound for exactly these operands, 5e-3 of the largest
    # reference magnitude (test_gpu_parity.py, test_pick_opts_keeps_the_north_star_domain_on_the_fast_kernels); the eight-wave build
    # has the same error to the bit (measured at BH = 64, N = 1024: dk 3.9e-3 of the scale).
    for nm, got in zip(("dk", "dv"), new1):
        scale = max(1.0, float(np.max(np.abs(ref[nm]))))
        err = maxabs(got[heads], ref[nm])
        print(f"BH={BH} N={N} x{amp:g} {nm}: max-abs {err:.3e}, scale {scale:.3g}")
        assert err < (1e-3 if amp == 1.0 else 5e-3 * scale), (nm, err, scale)


def test_plan_names_the_build():
    from flash_attention_minitorch_amd import _lib, device_ops
    fold = device_ops.OPTS_FOLDED_SCALE
    # the metric shape: the four-wave build by default, the eight-wave build on request; the family name is the same
    assert _builds(64, 4096, False, fold) == ["DQ_SLOT_TILED", "DKDV_SLOT64_TILED"]
    assert _builds(64, 4096, False, None) == ["DQ_SLOT_TILED", "DKDV_SLOT64_TILED"]
    assert _builds(64, 4096, False, (6,)) == ["DQ_SLOT_TILED", "DKDV_SLOT"]
    assert _lib.plan(64, 4096, D, False, 2, _lib.FA_DTYPE_BF16, device_ops.STAGE_ALL, fold) == ["bwd_dq_slot_kernel", "bwd_dkdv_slot_kernel"]
    # every other case keeps its kernel: causal, ragged N, a launch too small for several heads per workgroup, one head per workgroup
    assert _builds(64, 4096, True, fold) == ["DQ_SLOT_CAUSAL", "DKDV_SLOT_CAUSAL"]
    assert _builds(64, 4000, False, fold) == ["BWD_PREP", "DKDV_SLOT", "DQ_SLOT_MASKED"]
    assert _builds(8, 1024, False, fold) == ["DQ_SLOT_WHOLE", "DKDV_SLOT"]
    assert _builds(64, 4096, False, (0, 0, 0, 0, 0, 1)) == ["DQ_SLOT_WHOLE", "DKDV_SLOT"]
    assert _builds(64, 4000, False, (7,)) == ["BWD_PREP", "DKDV_SLOT", "DQ_SLOT_MASKED"]   # (forcing needs a valid shape: N a multiple of 256)
    assert "DKDV_SLOT64_TILED" not in _builds(64, 4096, True, (7,))
