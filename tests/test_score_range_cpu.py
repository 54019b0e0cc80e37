"""The deferred-reference softmax of the training-side forwards (window capped and uncapped, varlen, bidir, prefix) under the NumPy
model of tests/score_range.py, no GPU: the inputs of the existing GPU tests never reach the redo branch (a lane's partial row sum
stays far below *_DEFER_SUM = 64), the cases of tests/test_gpu_score_range.py do, in every library and dtype, with waves in which every
row outgrows its reference and waves in which only some do; ramp_down never does; low_lse / high_lse have |L| > 100 on every row."""
import functools

import numpy as np
import pytest

import oracle
import score_range as sr
from score_range import BN, CASES, LIBS, Case, Problem, model_counts, reference_steps


@functools.lru_cache(maxsize=None)
def _counts(case):
    return model_counts(sr.problem(case))


def test_the_constants_the_model_runs_on_are_the_headers():
    k = sr.tile_constants()
    assert k["bn"] == {"bf16": 64, "f32": 32} and k["defer"] == {"window": 64.0, "bidir": 64.0} and k["qblock"] == [128, 128]
    # acc_row(i, h) of fa_atoms.h: the keys of lane half h within a 32-key sub-tile
    acc_row = lambda i, h: (i & 3) + 8 * (i >> 2) + 4 * h
    for h in (0, 1):
        assert sorted(acc_row(i, h) for i in range(16)) == [j for j in range(32) if (j >> 2) & 1 == h]


def test_the_model_by_hand():
    """One wave of 32 rows on four fp32 tiles (bn = 32), every pair admitted.  Tile 0: first.  Tile 1 at the reference: 16 keys of
    P = 1 per lane, deferred, lane sum 16.  Tile 2: one key of rows 0..4 at ln 60 above the reference: 60 + 15 = 75 >= 64 in that
    lane, redone with 5 rows over, and those rows' reference moves.  Tile 3: every key ln 3.9 above the OLD reference: 16 x 3.9 = 62.4
    for the rows that kept it (deferred), P < 1 for the five that moved."""
    s = np.zeros((32, 128))
    s[:5, 64 + 9] = np.log(60.0)
    s[:, 96:] = np.log(3.9)
    st = reference_steps(np.ones((32, 128), bool), s, 32, 1.0)
    assert [x.kind for x in st] == ["first", "deferred", "redone", "deferred"]
    assert st[1].lane_sum == 16.0 and st[2].rows_over == 5 and st.partial == 1 and st.whole == 0
    assert abs(st.max_lane_sum - 62.4) < 1e-9
    s[:, 96:] = np.log(4.1)   # 65.6: redone, by the 27 rows that stood on the old reference
    st = reference_steps(np.ones((32, 128), bool), s, 32, 1.0)
    assert [x.kind for x in st][3] == "redone" and st[3].rows_over == 27
    # the two lane halves sum apart: 20 keys of P = 3.9 in one tile, 16 in half 0 (62.4) and 4 in half 1 (15.6 + 12): deferred
    s = np.zeros((32, 64))
    s[:, 32 + np.array([0, 1, 2, 3, 8, 9, 10, 11, 16, 17, 18, 19, 24, 25, 26, 27, 4, 5, 6, 7])] = np.log(3.9)
    assert [x.kind for x in reference_steps(np.ones((32, 64), bool), s, 32, 1.0)] == ["first", "deferred"]
    # a bf16 tile is two sub-tiles on the same lanes: the same 16 keys twice is 124.8
    s = np.zeros((32, 128))
    s[:, 64 + np.array([0, 1, 2, 3, 8, 9, 10, 11, 16, 17, 18, 19, 24, 25, 26, 27])] = np.log(3.9)
    s[:, 96 + np.array([0, 1, 2, 3, 8, 9, 10, 11, 16, 17, 18, 19, 24, 25, 26, 27])] = np.log(3.9)
    st = reference_steps(np.ones((32, 128), bool), s, 64, 1.0)
    assert [x.kind for x in st] == ["first", "redone"] and st.whole == 1
    # rows that gain their reference late: a window of 8 on 64 rows walks tile 0 then tile 1 for wave 1; in tile 0 only rows 32..38
    # admit a key, so tile 1 is "first" too (some row has no reference yet), and a wave that admits nothing of a tile skips it
    adm = sr.window_admit(64, 8, 0, 32)
    st = reference_steps(adm, np.zeros((64, 64)), 32, 1.0, sr.win_walk(64, 8, 0, 32))
    assert [(x.wave, x.tile, x.kind) for x in st] == [(0, 0, "first"), (0, 1, "skipped"), (1, 0, "first"), (1, 1, "first")]


def test_the_window_walk_is_winwalk():
    walk = sr.win_walk(515, 100, 5, 64)
    assert walk(0) == [0, 1] and walk(1) == [0, 1, 2, 3] and walk(2) == [0, 2, 3, 4, 5] and walk(4) == [0, 6, 7, 8]
    assert sr.win_walk(300, 300, 0, 32)(2) == list(range(10)) and sr.win_walk(300, 40, 33, 32)(2) == [0, 1, 6, 7, 8, 9]
    assert sr.prefix_walk(64, 192, 64)(0) == [0, 1, 2] and sr.prefix_walk(200, 70, 64)(0) == [] and sr.prefix_walk(200, 70, 64)(1) == [0, 1]


# ---- today's inputs never reach the redo branch -----------------------------------------------------------------------------------

def _packed_problem(lib, dtype, d, q, k, segments, W=0, S=0, cap=0.0):
    return Problem(Case(lib, "u", dtype, d, None), q, k, None, None, segments, q.shape[0], k.shape[0], None, None, W, S, cap)


def _existing():
    """(id, problems): the _inputs of the existing GPU tests under their seeds, one case or more per library."""
    import test_gpu_bidir as tb
    import test_gpu_prefix as tp
    import test_gpu_softcap_train as tc
    import test_gpu_varlen as tv
    import test_gpu_window_train as tw
    out = []
    for case in (tw.CASES[7], tw.CASES[13], tw.CASES[11]):   # N = 515: bf16 d = 64 with sinks, fp32 d = 32 and d = 128
        N, W, S, d, dtype, _, Hq, Hkv, B = case
        W = W or N - 1
        q, k, _, _ = tw._inputs(np.random.default_rng(N * 1000 + W + S), dtype, B, Hq, Hkv, N, d)
        out.append(("window-" + str(case), [_packed_problem("window", dtype, d, q[b].transpose(1, 0, 2), k[b].transpose(1, 0, 2), [(0, N, 0, N)], W, S)
                                            for b in range(B)]))
    N, W, S, d, dtype, _, Hq, Hkv, B = case = tc.CASES[8]    # N = 515 without a window, bf16 d = 64, under the cap of that file
    q, k, _, _ = tw._inputs(np.random.default_rng(N * 1000 + N + S + d), dtype, B, Hq, Hkv, N, d)
    for cap in (tc.CAP, 0.0):   # (and what the cap hides: the same inputs uncapped)
        out.append((f"capped-{cap}-" + str(case), [_packed_problem("capped", dtype, d, q[b].transpose(1, 0, 2), k[b].transpose(1, 0, 2), [(0, N, 0, N)], N, S, cap)
                                                   for b in range(B)]))
    for case in (tv.CASES[8], tv.CASES[10]):                 # set B: 513, 31, 255, 256 rows, bf16 d = 128 and fp32 d = 32, no window
        name, W, S, Hq, Hkv, dtype, d = case
        cu, T = tv._cu(name)
        q, k, _, _ = tv._inputs(np.random.default_rng(T * 1000 + W + S + d), dtype, T, Hq, Hkv, d)
        out.append(("varlen-" + str(case), [_packed_problem("varlen", dtype, d, q, k, [(s, n, s, n) for s, n in tv.seq_rows(cu, T)], W, S)]))
    for mod, lib in ((tb, "bidir"), (tp, "prefix")):
        for case in (mod.CASES[14], mod.CASES[15]):          # set U: 300 queries on 700 keys, bf16 d = 64 and fp32 d = 128
            name, Hq, Hkv, dtype, d = case
            cu_q, Tq, cu_k, Tk = mod._cus(name)
            q, k, _, _ = tb._inputs(np.random.default_rng(Tq * 1000 + Tk + d), dtype, Tq, Tk, Hq, Hkv, d)
            segs = [(a, b, c, e) for (a, b), (c, e) in zip(tb.seq_rows(cu_q, Tq), tb.seq_rows(cu_k, Tk))]
            out.append((f"{lib}-" + str(case), [_packed_problem(lib, dtype, d, q, k, segs)]))
    return out


def test_the_inputs_of_the_existing_gpu_tests_never_reach_the_redo_branch():
    seen = set()
    for name, problems in _existing():
        tot = [model_counts(p) for p in problems]
        redone, lane, steps = sum(t["redone"] for t in tot), max(t["max_lane_sum"] for t in tot), sum(t["deferred"] for t in tot)
        print(f"{name}: {steps} deferred steps, {redone} redone, largest lane sum {lane:.1f}")
        assert redone == 0 and steps > 0 and lane < 64.0, (name, redone, lane)
        seen.add(name.split("-")[0])
    assert seen == set(LIBS)


def test_causal_u11_at_n_515_under_the_default_scale_and_0_2():
    """The issue's own figures: N = 515, d in {32, 64, 128}, both scales: no redone tile, the largest lane sum far below 64."""
    rng = np.random.default_rng(0)
    for dtype in ("bf16", "f32"):
        for d in (32, 64, 128):
            q, k = (sr.rand_u(rng, (515, 1, d)) for _ in range(2))
            if dtype == "bf16":
                q, k = oracle.bf16_round(q), oracle.bf16_round(k)
            sc = q[:, 0].astype(np.float64) @ k[:, 0].astype(np.float64).T
            for tau in (1.0 / np.sqrt(d), 0.2):
                st = reference_steps(sr.window_admit(515, 515, 0, BN[dtype]), sc, BN[dtype], tau, sr.win_walk(515, 515, 0, BN[dtype]))
                assert st.redone == 0 and st.max_lane_sum < 40.0, (dtype, d, tau, st.redone, st.max_lane_sum)
                assert st.count("deferred") > 50 and st.count("first") == 17   # (17 waves, each with one first tile)


# ---- the new cases do ----------------------------------------------------------------------------------------------------------------

ALL = [c for lib in LIBS for c in CASES[lib]]


@pytest.mark.parametrize("case", [c for c in ALL if c.family in sr.REDO_FAMILIES], ids=sr.case_id)
def test_every_case_that_claims_the_redo_has_a_redone_tile(case):
    tot = _counts(case)
    print(sr.case_id(case), tot)
    assert tot["redone"] >= 1, tot


def test_every_library_and_dtype_is_redone_with_whole_waves_and_with_partial_ones_on_a_spiked_diagonal():
    for lib in LIBS:
        for dtype in ("bf16", "f32"):
            mine = [c for c in CASES[lib] if c.dtype == dtype and c.family in sr.REDO_FAMILIES]
            assert mine and all(_counts(c)["redone"] >= 1 for c in mine), (lib, dtype)
            assert sum(_counts(c)["whole"] for c in mine) >= 1, (lib, dtype)        # every row of a wave outgrew its reference
            if lib != "bidir":   # (no diagonal there: a spike is admitted by every row)
                assert sum(_counts(c)["partial"] for c in mine if c.family == "spikes") >= 1, (lib, dtype)
        print(lib, "redone steps of the new cases:", sum(_counts(c)["redone"] for c in CASES[lib]), "of", sum(_counts(c)["steps"] for c in CASES[lib]))


def test_the_spiked_diagonal_splits_its_wave():
    """The window spikes cases: the wave that holds the diagonal spike redoes that key tile with 19 of its 32 rows over (the rows at or
    below the spike), once per head."""
    for case in (c for c in CASES["window"] if c.family == "spikes"):
        p = sr.problem(case)
        N, bn = case.geom[0], BN[case.dtype]
        i_d = 32 * ((N - 1) // 32) - 32 + 13
        assert i_d in sr.spike_keys(N, N, bn, 0, p.S)
        hits = 0
        for admit, sc, tau, walk, _ in sr.head_scores(p):
            st = reference_steps(admit, sc, bn, tau, walk)
            hits += sum(1 for x in st if x.kind == "redone" and x.wave == i_d // 32 and x.tile == i_d // bn and x.rows_over == 19)
        assert hits == sr.H, (case, hits)


def test_spike_keys_sit_on_the_edges():
    assert sr.spike_keys(200, 200, 64, 0, 3) == [1, 63, 64, 173, 199] and sr.spike_keys(300, 300, 32, 0, 0) == [31, 32, 269, 299]
    assert sr.spike_keys(129, 77, 64, None, 0) == [63, 64, 76] and sr.spike_keys(5, 63, 64, None, 0) == [62]
    assert sr.spike_keys(257, 300, 64, 43, 0) == [63, 64, 237 + 43, 299] and sr.spike_keys(200, 70, 32, -130, 0) == [31, 32, 173 - 130, 69]
    for N, bn in ((200, 64), (300, 64), (200, 32), (300, 32)):   # the diagonal spike, in a wave past row 64, is the only spike of its
        keys = sr.spike_keys(N, N, bn, 0, 3)                       # key tile that the wave's rows admit
        i_d = 32 * ((N - 1) // 32) - 32 + 13
        assert i_d >= 64 and [j for j in keys if j // bn == i_d // bn and j <= i_d // 32 * 32 + 31] == [i_d]


@pytest.mark.parametrize("case", [c for c in ALL if c.family == "ramp_down"], ids=sr.case_id)
def test_ramp_down_never_moves_its_reference(case):
    tot = _counts(case)
    assert tot["redone"] == 0 and tot["deferred"] > 0 and tot["max_lane_sum"] <= BN[case.dtype] / 2 + 1e-9, tot   # (every P <= 1)


@pytest.mark.parametrize("case", [c for c in ALL if c.family in ("low_lse", "high_lse")], ids=sr.case_id)
def test_the_lse_families_leave_the_range_in_which_exp_of_minus_l_is_a_float(case):
    L = sr.row_lse(sr.problem(case))
    print(sr.case_id(case), float(L.min()), float(L.max()))
    assert L.size and (np.max(L) < -100.0 if case.family == "low_lse" else np.min(L) > 100.0)


def test_the_families_are_what_they_say():
    for c in ALL:
        p = sr.problem(c)
        for a in (p.q, p.k, p.v, p.do):
            assert a.dtype == np.float32 and np.all(np.isfinite(a))
            assert c.dtype != "bf16" or np.array_equal(oracle.bf16_round(a), a)
        assert np.max(np.abs(p.v)) <= 1 and np.max(np.abs(p.do)) <= 1
        if c.family.startswith("ramp") or c.family == "spikes":
            assert np.max(np.abs(p.q)) <= 1
        if c.family.startswith("ramp"):
            assert np.max(np.abs(p.k)) <= 1
        if c.family == "x6":
            assert 5 < np.max(np.abs(p.q)) <= 6 and 5 < np.max(np.abs(p.k)) <= 6


def test_the_case_lists_cover_every_dtype_d_pair_family_and_geometry_in_every_library():
    pairs = {(t, d) for t in ("bf16", "f32") for d in (32, 64, 128)}
    for lib in LIBS:
        assert {(c.dtype, c.d) for c in CASES[lib]} == pairs, lib
        assert {(c.dtype, c.d) for c in CASES[lib] if c.family in sr.REDO_FAMILIES} == pairs, lib
        assert {c.family for c in CASES[lib]} == set(sr.FAMILIES) - ({"low_lse", "high_lse"} if lib == "capped" else set()), lib
        assert all(c.lib == lib for c in CASES[lib]) and len(set(CASES[lib])) == len(CASES[lib])
    for lib in ("window", "capped"):
        assert {c.geom[0] for c in CASES[lib]} == {200, 300} and {c.geom[1:] for c in CASES[lib]} == {(0, 0), (40, 3), (100, 33)}
    assert {c.geom for c in CASES["varlen"]} == {(0, 0), (40, 3)}
    assert [k - q for q, k in sr.PREFIX_PAIRS] == [0, 43, 128, -130]
    import test_gpu_prefix as tp
    assert all(pr in list(zip(*tp.SETS["X"][:2])) for pr in sr.PREFIX_PAIRS)
    assert len(ALL) <= 50
