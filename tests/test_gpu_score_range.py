"""The training-side libraries (window uncapped and under softcap = 50, varlen, bidir, prefix) on the GPU at scores beyond U(-1, 1):
the families and cases of tests/score_range.py, on which the forward's deferred reference is outgrown and the tile redone (counted,
without a GPU, by tests/test_score_range_cpu.py) and the backward meets row logsumexps beyond +-100.  out, lse, dq, dk and dv against
the fp64 references the other GPU tests of these libraries use; the packed libraries' laws, repeatability, and the window forward
against the core library, on the same inputs.

Bounds (README "Accuracy envelope"; TOL of tests/test_gpu_decode.py):
  ramp_down      inputs in [-1, 1]: the plain envelope, max-abs TOL[dtype], unless the reference alone (score_range.p_rounding_estimate)
                 shows the first keys holding so much of every row's P that four standard deviations of its bf16 rounding, gathered by
                 one key's dV over all rows of its group, pass 1e-3: then that key's dV is a sum of hundreds of terms of one size, the
                 tensor's scale is no longer 1, and the case takes the large-magnitude bound of its dtype.  At these d the family as
                 defined (|elements| <= 1, scores falling by 1.5 sqrt(d) over the sequence) does so in every case: the test below
                 prints the estimates
  every other    finite, and below 5e-3 * max(1, max |reference tensor|) for bf16, fp32_envelope * max(1, max |reference tensor|) for fp32
  fp32_envelope  TOL["f32"], except where the fp32 rounding of the scores themselves is larger (fp32_score_rounding_envelope below):
                 the low_lse / high_lse cases alone, and by more than a hair only at d = 128, where |S'| reaches 717
Measured maxima: profiles/score_range_accuracy.txt."""
import functools

import numpy as np
import pytest

import score_range as sr
import test_gpu_bidir as tb
import test_gpu_prefix as tp
import test_gpu_varlen as tv
import test_gpu_window_train as tw
from gpu_util import maxabs
from score_range import CASES, Case, case_id
from test_gpu_decode import TOL
from test_softcap_train_cpu import softcap_train_reference
from test_window_train_cpu import window_train_reference

pytestmark = pytest.mark.gpu

NAMES = tw.NAMES
LAYOUT = "bnhd"   # the window cases: (1, N, heads, d), the packed rows as they are


def _windowed(p):
    return p.case.lib in ("window", "capped")


def _bhnd(a):
    return np.ascontiguousarray(a.transpose(1, 0, 2))[None]


@functools.lru_cache(maxsize=None)
def _problem_and_reference(case):
    """The case's inputs and its fp64 reference (out, lse, dq, dk, dv), computed once.  Window cases: (1, heads, N, d) / (1, H, N)
    arrays; packed cases: (T, heads, d) / (H, Tq)."""
    p = sr.problem(case)
    if _windowed(p):
        N = p.Tq
        args = [_bhnd(a) for a in (p.q, p.k, p.v, p.do)] + [p.W or N, p.S]
        want = softcap_train_reference(*args, None, p.cap) if p.cap else window_train_reference(*args)
    elif case.lib == "varlen":
        want = tv._reference(p.q, p.k, p.v, p.do, p.cu_q, p.Tq, p.W, p.S)
    else:
        want = (tb if case.lib == "bidir" else tp)._reference(p.q, p.k, p.v, p.do, p.cu_q, p.Tq, p.cu_k, p.Tk)
    for w in want:
        w.setflags(write=False)
    return p, want


def _device(p):
    dt = p.case.dtype
    if _windowed(p):
        return [tw._dev(_bhnd(a), LAYOUT, dt) for a in (p.q, p.k, p.v, p.do)]
    return [tb._dev(a, dt) for a in (p.q, p.k, p.v, p.do)]


def _call(p, ts):
    """Forward and backward through device_ops on device tensors: (out, lse, dq, dk, dv) device tensors."""
    from flash_attention_minitorch_amd import device_ops
    lib = p.case.lib
    if _windowed(p):
        W, kw = p.W or p.Tq, dict(softcap=p.cap) if p.cap else {}
        o, lse = device_ops.flash_attn_fwd_window(ts[0], ts[1], ts[2], W, p.S, None, LAYOUT, **kw)
        return (o, lse) + tuple(device_ops.flash_attn_bwd_window(ts[0], ts[1], ts[2], o, ts[3], lse, W, p.S, None, LAYOUT, **kw))
    if lib == "varlen":
        return tv._run(*ts, tb._i32(p.cu_q), p.W, p.S)
    return (tb if lib == "bidir" else tp)._run(*ts, tb._i32(p.cu_q), tb._i32(p.cu_k))


def _host(p, outs):
    return [tw._host(t, LAYOUT) for t in outs] if _windowed(p) else [t.double().cpu().numpy() for t in outs]


def fp32_score_rounding_envelope(p):
    """In the manner of test_gpu_parity.operand_rounding_envelope, for fp32.  A score S' = c q.k (log2 units) is accumulated over d
    products in fp32; every partial sum is rounded to 24 bits, 2^-24 relative to a partial sum that is at most |S'| when the products
    are of one sign (low_lse, high_lse: keys and queries of one sign each).  d such roundings move S' by up to d * 2^-24 * |S'|, and by
    sqrt(d) * 2^-24 * |S'| as a random walk; P = exp2(S' - L') moves by ln 2 times that, relative, and so does every tensor P enters.
    The bound is the random-walk figure, ln 2 * sqrt(d) * 2^-24 * max |S'| over the admitted pairs, where that exceeds TOL["f32"].
    Checked without a GPU: the scores of prefix-high_lse-f32-d128 (max |S'| = 717) accumulated one product at a time in fp32, with
    the softmax and P.V in fp64, put out 1.45e-4 from the fp64 reference; the kernel measures 1.50e-4, the bound is 3.35e-4
    (profiles/score_range_accuracy.txt).  The cap builds accumulate the raw score in front of the cap: the raw scores count."""
    d = p.case.d
    smax = max((float(np.max(np.abs(np.where(admit[:sc.shape[0], :sc.shape[1]], sc, 0.0)))) * tau for admit, sc, tau, _, _ in
                sr.head_scores(p._replace(cap=0.0))), default=0.0) * 1.4426950408889634
    return max(TOL["f32"], float(np.log(2.0) * np.sqrt(d) * 2.0 ** -24 * smax))


def dominated_by_one_key(p):
    """ramp_down, on the reference alone (the module's docstring)."""
    return max(sr.p_rounding_estimate(p)) >= TOL["bf16"]


def bounds(p, want):
    """Per tensor, from the reference alone (the module's docstring)."""
    dtype = p.case.dtype
    if p.case.family == "ramp_down" and not dominated_by_one_key(p):
        return {n: TOL[dtype] for n in NAMES}
    rel = 5e-3 if dtype == "bf16" else fp32_score_rounding_envelope(p)
    return {n: rel * max(1.0, float(np.max(np.abs(w)))) for n, w in zip(NAMES, want)}


def _compare(p, got, want, what):
    errs = {n: maxabs(g, w) for n, g, w in zip(NAMES, got, want)}
    bnd = bounds(p, want)
    print(f"score_range_accuracy {what}: " + " ".join(f"{n} {errs[n]:.3e} (bound {bnd[n]:.2e})" for n in NAMES))
    assert all(np.all(np.isfinite(g)) for g in got), what
    assert all(errs[n] < bnd[n] for n in NAMES), (what, errs, bnd)


@pytest.mark.parametrize("case", [c for lib in sr.LIBS for c in CASES[lib]], ids=case_id)
def test_forward_and_backward_match_the_fp64_reference(case):
    p, want = _problem_and_reference(case)
    got = _host(p, _call(p, _device(p)))
    _compare(p, got, want, case_id(case))
    if not _windowed(p):   # rows that carry no result: exactly zero
        if case.lib == "varlen":
            lq = lk = tv._owned(p.cu_q, p.Tq)
        else:
            lq, lk = (tb if case.lib == "bidir" else tp)._live(p.cu_q, p.Tq, p.cu_k, p.Tk)
        for n, g, qside in zip(NAMES, got, tb.QSIDE):
            assert np.all(tb._rows(n, g)[~(lq if qside else lk)] == 0), (case, n)


def test_the_bounds_are_the_projects_except_where_the_reference_says_why():
    """ramp_down: the estimate decides, and it is an estimate of something: where it sends a case to the large-magnitude bound, one
    key's dV is far larger than any input.  fp32: TOL["f32"] x scale in every family but low_lse / high_lse, and at most 3.4 of them there."""
    for c in (c for lib in sr.LIBS for c in CASES[lib]):
        p, want = _problem_and_reference(c)
        bnd = bounds(p, want)
        if c.family == "ramp_down":
            est, plain = sr.p_rounding_estimate(p), set(bnd.values()) == {TOL[c.dtype]}
            print(case_id(c), "estimate (out, dv)", tuple(f"{e:.2e}" for e in est), "plain envelope" if plain else "large-magnitude bound",
                  f"max |dv| {float(np.max(np.abs(want[4]))):.1f}")
            assert plain == (max(est) < 1e-3) and (plain or float(np.max(np.abs(want[4]))) > 3.0)
        elif c.dtype == "f32":
            env = fp32_score_rounding_envelope(p)
            assert env == TOL["f32"] or c.family in ("low_lse", "high_lse"), (case_id(c), env)   # (717 x sqrt(128): the largest)
            assert env < 4e-4 and bnd["out"] == env * max(1.0, float(np.max(np.abs(want[0]))))
        else:
            assert bnd["out"] == 5e-3 * max(1.0, float(np.max(np.abs(want[0]))))


# ---- the laws of the packed libraries ----------------------------------------------------------------------------------------------

def _x6(lib, dtype):
    return next(c for c in CASES[lib] if c.family == "x6" and c.dtype == dtype)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_every_packed_sequence_has_the_bits_of_the_window_library_on_that_sequence_alone(dtype):
    from flash_attention_minitorch_amd import device_ops
    p, _ = _problem_and_reference(_x6("varlen", dtype))
    ts = _device(p)
    got = _call(p, ts)
    for sq, n, _, _ in p.segments:
        one = [t[sq:sq + n][None].contiguous() for t in ts]
        o, lse = device_ops.flash_attn_fwd_window(one[0], one[1], one[2], p.W or tv.NO_WINDOW, p.S)
        dq, dk, dv = device_ops.flash_attn_bwd_window(one[0], one[1], one[2], o, one[3], lse, p.W or tv.NO_WINDOW, p.S)
        for nm, g, a in zip(NAMES, got, (o[0], lse[0], dq[0], dk[0], dv[0])):
            mine = g[:, sq:sq + n] if nm == "lse" else g[sq:sq + n]
            assert tb._bits_equal(mine, a), (case_id(p.case), nm, (sq, n), float((mine - a).abs().max()))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("lib", ["bidir", "prefix"])
def test_every_sequence_has_the_bits_of_the_same_call_on_that_sequence_alone(lib, dtype):
    p, _ = _problem_and_reference(_x6(lib, dtype))
    ts = _device(p)
    got = _call(p, ts)
    run = (tb if lib == "bidir" else tp)._run
    for sq, nq, sk, nk in p.segments:
        one = [t[s:s + n].contiguous() for t, s, n in ((ts[0], sq, nq), (ts[1], sk, nk), (ts[2], sk, nk), (ts[3], sq, nq))]
        alone = run(*one, tb._i32([0, nq]), tb._i32([0, nk]))
        for nm, g, a, qside in zip(NAMES, got, alone, tb.QSIDE):
            s, n = (sq, nq) if qside else (sk, nk)
            mine = g[:, s:s + n] if nm == "lse" else g[s:s + n]
            assert tb._bits_equal(mine, a), (case_id(p.case), nm, (sq, nq, sk, nk), float((mine - a).abs().max()))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("lib", sr.LIBS)
def test_two_calls_on_spikes_return_the_same_bits(lib, dtype):
    p, _ = _problem_and_reference(next(c for c in CASES[lib] if c.family == "spikes" and c.dtype == dtype))
    ts = _device(p)
    first, second = _call(p, ts), _call(p, ts)
    assert all(tb._bits_equal(a, b) for a, b in zip(first, second))


# ---- inside the old domain: two sets of kernels, one reference ---------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_the_unwindowed_forward_on_x6_agrees_with_the_core_library(dtype):
    """W = N, S = 0 through the window library against device_ops.flash_attn_gqa (the core library under its default guard): each is
    held to the same reference by the large-magnitude bound, so they agree within twice that bound, and each is checked here too."""
    from flash_attention_minitorch_amd import device_ops
    case = Case("window", "x6", dtype, 64, (300, 0, 0))
    p, want = _problem_and_reference(case)
    N = p.Tq
    tq, tk, tv_, _ = _device(p)
    o, _ = device_ops.flash_attn_fwd_window(tq, tk, tv_, N, 0, None, LAYOUT)
    core = device_ops.flash_attn_gqa(tq, tk, tv_, causal=True, layout=LAYOUT)
    o, core = tw._host(o, LAYOUT), tw._host(core, LAYOUT)
    bnd = bounds(p, want)["out"]
    errs = (maxabs(o, core), maxabs(o, want[0]), maxabs(core, want[0]))
    print(f"score_range_accuracy window-vs-core-x6-{dtype}-d64-N300: window vs core {errs[0]:.3e} (bound {2 * bnd:.2e}) "
          f"window vs fp64 {errs[1]:.3e} core vs fp64 {errs[2]:.3e} (bound {bnd:.2e})")
    assert np.all(np.isfinite(o)) and np.all(np.isfinite(core))
    assert errs[0] < 2 * bnd and errs[1] < bnd and errs[2] < bnd, (errs, bnd)
