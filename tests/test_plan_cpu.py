"""The kernel selection, pinned on the CPU: fa_mi355x_plan needs no GPU (without a device the launch-size rules assume 256 CUs, which
is what an MI355X reports), so every (return code, plan string) of a grid over dtype, d, N, batch, causal, variant, stage mask and the
per-call options is compared with a fixture that was generated from the build BEFORE the selection became a value
(tests/golden/make_plan_golden.py holds the grid and the generator; tests/golden/plan_grid.npz the 290,304 recorded answers)."""
import ctypes
import importlib.util
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _grid_module():
    spec = importlib.util.spec_from_file_location("make_plan_golden", os.path.join(ROOT, "tests", "golden", "make_plan_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from flash_attention_minitorch_amd import _lib
    return _lib


def test_plan_grid_matches_the_recorded_selection(built):
    grid = _grid_module()
    # the grid as the issue states it: a shortened one cannot pass
    assert (len(grid.DTYPES), len(grid.DS), len(grid.NS), len(grid.BATCHES), len(grid.CAUSAL), len(grid.VARIANTS), len(grid.STAGES),
            len(grid.OPTIONS)) == (2, 3, 12, 8, 2, 2, 7, 18)
    want = grid.load_fixture()
    assert len(want) == grid.N_CASES == 290304
    assert len({p for _, p in want}) == 42 and {rc for rc, _ in want} == {0}   # what the parent build answered
    lib = ctypes.CDLL(built.lib_path(built.CORE_NAME))   # a handle of its own: core()'s argtypes stay as they are
    got = grid.walk(lib)
    assert len(got) == grid.N_CASES
    bad = [(case, g, w) for case, g, w in zip(grid.cases(), got, want) if g != w]
    assert not bad, f"{len(bad)} of {len(got)} plans differ; first (dtype, d, N, batch, causal, variant, stages, options): {bad[:5]}"
    # every one of the parent's 42 distinct plans still occurs
    assert {p for _, p in got} == {p for _, p in want}
