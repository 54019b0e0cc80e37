"""Scores beyond U(-1, 1) for the training-side libraries (window capped and uncapped, varlen, bidir, prefix): the input families, a
NumPy model of the forward's deferred-reference softmax that says which (wave, key tile) steps take the redo branch, and the case
lists that tests/test_score_range_cpu.py (the model, no GPU) and tests/test_gpu_score_range.py (the kernels) share.  A plain helper
module like tests/gpu_util.py: no tests of its own.

Everything here is laid out PACKED, (rows, heads, d) with the sequence on axis 0, whichever library a case is for; the window cases
(B = 1) are transposed to (1, heads, N, d) where they are run."""
import os
import re
import zlib
from collections import namedtuple

import numpy as np

import oracle
from gpu_util import rand_u

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flash_attention_minitorch_amd", "csrc")
H, HKV = 4, 2   # every case: four query heads on two key heads


def tile_constants():
    """What the model needs from the headers: the forward's key tile per dtype (SideTiles::BN of fa_side_host.h, which the four
    .hip files take their BN from), the bound on a lane's partial row sum (WIN_DEFER_SUM of fa_window.h, BIDIR_DEFER_SUM of
    fa_bidir.h, which fa_prefix.h uses too) and the query block (BIDIR_QBLOCK, VARLEN_QBLOCK; the window kernels' literal 128)."""
    read = lambda name: open(os.path.join(CSRC, name)).read()
    bn = re.search(r"struct SideTiles \{.*?static constexpr int BN = BF \? (\d+) : (\d+),", read("fa_side_host.h"), re.S)
    win = re.search(r"constexpr float WIN_DEFER_SUM = ([\d.]+)f;", read("fa_window.h"))
    bid = re.search(r"constexpr float BIDIR_DEFER_SUM = ([\d.]+)f;", read("fa_bidir.h"))
    qb = [int(re.search(rf"constexpr int {n} = (\d+);", read(f)).group(1)) for n, f in (("BIDIR_QBLOCK", "fa_bidir.h"), ("VARLEN_QBLOCK", "fa_varlen.h"))]
    assert "BIDIR_DEFER_SUM" in read("fa_prefix.h") and "WIN_DEFER_SUM" in read("fa_window_body.h")
    return {"bn": {"bf16": int(bn.group(1)), "f32": int(bn.group(2))}, "defer": {"window": float(win.group(1)), "bidir": float(bid.group(1))},
            "qblock": qb}


_K = tile_constants()
BN = _K["bn"]
DEFER_SUM = _K["defer"]["window"]
QBLOCK = _K["qblock"][0]


# ---- the input families ----------------------------------------------------------------------------------------------------------

FAMILIES = ("x6", "ramp_up", "ramp_down", "spikes", "low_lse", "high_lse")
REDO_FAMILIES = ("x6", "ramp_up", "spikes")   # the ones a case may claim the redo branch with


def spike_keys(nq, nk, bn, delta, sink):
    """Key positions (within a sequence of nk keys and nq queries, query i on the diagonal i + delta; delta None: no diagonal) that
    the `spikes` family replaces: a sink key; the last key of key tile 0 and the first of tile 1; a key on the diagonal of row 13 of
    the last wave but one, so that 13 rows of that wave do not admit it and 19 do, in a key tile of its own; the last real key."""
    keys = [1] if sink and sink >= 2 and nk > 1 else []
    if nk > bn:
        keys += [bn - 1, bn]
    if delta is not None:
        i_d = 32 * ((nq - 1) // 32) - 32 + 13
        if i_d >= 64 and 0 <= i_d + delta < nk:
            keys.append(i_d + delta)
    keys.append(nk - 1)
    return sorted(set(keys))


def family(name, rng, dtype, q_shape, k_shape, segments=None, delta=0, sink=0):
    """q, do of q_shape = (Tq, H, d) and k, v of k_shape = (Tk, Hkv, d), float32, rounded to the dtype.  v and do are U(-1, 1) in
    every family.  ``segments``: [(sq, nq, sk, nk)], the rows of each sequence in the two buffers (default: one sequence over
    everything); ``delta``: 0 (query i sits at key i), "prefix" (at key i + nk - nq) or None (no diagonal); ``sink``: the call's S.
    Key indices count within a sequence; query head h goes with key head h // G.
      x6         q, k = 6 x U(-1, 1): the project's large-magnitude input
      ramp_up    k_j = u * ramp(j), q_i = a_i * u: u a random sign vector per key head, ramp linear from -1 to 1 over the sequence's
                 keys, a_i in U(0.5, 1).  Scores rise with the key index, every |element| <= 1
      ramp_down  the same with the ramp reversed: the first keys (the sinks) hold every row's maximum
      spikes     U(-1, 1) keys except the spike_keys, which are 8 * u * (rank + 1) / count (later spikes are larger: each is a jump
                 of about ten or more over everything before it); q_i = 0.9 u + 0.1 U(-1, 1)
      low_lse / high_lse   tests/test_gpu_parity.py::test_ragged_tail_with_very_negative_logsumexp: k = U(-1, 1) + 1.5, all of one
                 sign, q = -/+ 16 * |U(-1, 1) + 1.5|"""
    assert name in FAMILIES, name
    (Tq, Hq, d), (Tk, Hk, _) = q_shape, k_shape
    G = Hq // Hk
    q, k, v, do = rand_u(rng, q_shape), rand_u(rng, k_shape), rand_u(rng, k_shape), rand_u(rng, q_shape)
    segments = [(0, Tq, 0, Tk)] if segments is None else segments
    u = np.where(rng.random((Hk, d)) < 0.5, np.float32(-1), np.float32(1))
    uq = np.repeat(u, G, axis=0)   # (H, d)
    if name == "x6":
        q, k = q * np.float32(6), k * np.float32(6)
    elif name in ("low_lse", "high_lse"):
        k = k + np.float32(1.5)
        q = np.float32(-16 if name == "low_lse" else 16) * np.abs(q + np.float32(1.5))
    elif name in ("ramp_up", "ramp_down"):
        a = (np.float32(0.75) + np.float32(0.25) * rand_u(rng, (Tq, Hq)))[:, :, None]
        q = a * uq[None]
        for sq, nq, sk, nk in segments:
            ramp = np.linspace(-1.0, 1.0, nk).astype(np.float32) if nk > 1 else np.zeros(nk, np.float32)
            k[sk:sk + nk] = (ramp if name == "ramp_up" else ramp[::-1])[:, None, None] * u[None]
    else:
        q = np.float32(0.9) * uq[None] + np.float32(0.1) * q
        for sq, nq, sk, nk in segments:
            if nq == 0 or nk == 0:
                continue
            dl = nk - nq if delta == "prefix" else delta
            keys = spike_keys(nq, nk, BN[dtype], dl, sink)
            for rank, j in enumerate(keys):
                k[sk + j] = np.float32(8.0 * (rank + 1) / len(keys)) * u
    rnd = oracle.bf16_round if dtype == "bf16" else (lambda a: a.astype(np.float32))
    return rnd(q), rnd(k), rnd(v), rnd(do)


# ---- the admit matrices, padded as the kernels see them --------------------------------------------------------------------------

def _up(n, m):
    return (n + m - 1) // m * m


def window_admit(N, W, S, bn):
    """test_window_train_cpu.admitted(N, W, S) continued over the rows of the last wave (32-row waves) and the keys of the last tile:
    the kernels apply win_admits to those rows and keys too (they read as zeros)."""
    i, j = np.arange(_up(N, 32))[:, None], np.arange(_up(N, bn))[None, :]
    return (j <= i) & ((j > i - W) | (j < S))


def bidir_admit(nq, nk, bn):
    """All-true with a key tail: every row, padding rows included, admits the keys below nk."""
    return np.broadcast_to(np.arange(_up(nk, bn))[None, :] < nk, (_up(nq, 32), _up(nk, bn))).copy()


def prefix_admit(nq, nk, bn):
    """j <= i + n_k - n_q, continued over the padding rows and keys like window_admit."""
    i, j = np.arange(_up(nq, 32))[:, None], np.arange(_up(max(nk, 1), bn))[None, :]
    return j <= i + nk - nq


def win_walk(N, W, S, bn):
    """WinWalk of fa_window.h for the 128-row query block qb: the tiles that hold a sink key and lie wholly below the window's range,
    then the tiles from the first row's window edge up to the last row's position."""
    def tiles(qb):
        q_lo, q_hi = qb * QBLOCK, min(N, qb * QBLOCK + QBLOCK) - 1
        lo_t = max(q_lo - W + 1, 0) // bn
        ns = min((S + bn - 1) // bn, lo_t)
        return list(range(ns)) + list(range(lo_t, q_hi // bn + 1))
    return tiles


def prefix_walk(nq, nk, bn):
    """The walk of prefix_fwd_kernel: the key tiles below the diagonal of the block's last row."""
    def tiles(qb):
        kend = max(0, min(nq, qb * QBLOCK + QBLOCK) + nk - nq)
        return list(range((kend + bn - 1) // bn))
    return tiles


# ---- the model -------------------------------------------------------------------------------------------------------------------

Step = namedtuple("Step", "wave tile kind rows_over rows_real lane_sum")


class Steps(list):
    """The (wave, tile) steps of one head, in the kernel's order."""

    def count(self, kind):
        return sum(1 for s in self if s.kind == kind)

    @property
    def redone(self):
        return self.count("redone")

    @property
    def whole(self):   # redone steps in which every real row of the wave outgrew its reference
        return sum(1 for s in self if s.kind == "redone" and s.rows_over == s.rows_real)

    @property
    def partial(self):   # ... in which only some did
        return sum(1 for s in self if s.kind == "redone" and 0 < s.rows_over < s.rows_real)

    @property
    def max_lane_sum(self):
        return max([s.lane_sum for s in self if s.kind == "deferred"], default=0.0)


def reference_steps(admit, scores, bn, tau, walk=None, defer_sum=None):
    """Which steps of the forward's deferred-reference softmax are skipped, take the classic step because some row has no reference
    yet ("first"), stand on the old reference ("deferred") or are redone, for one head.

    ``scores``: (n_q, n_k) fp64 q.k (``tau`` scales them; the capped build: the capped logits with tau = 1).  ``admit``: bool, at
    least as large, (a multiple of 32, a multiple of bn): the mask continued over the padding rows of the last wave and the padding
    keys of the last tile, whose scores are zeros as the kernels read them (window_admit, bidir_admit, prefix_admit).  ``walk``:
    query block -> its key tiles in the kernel's order (win_walk, prefix_walk; default: all, ascending).

    Mirrors, in fp64 and natural-log units where the kernels use fp32 and exp2:
      fa_window_body.h  win_fwd_kernel, the `tile` lambda: `active` and `q0 < N` (skipped), `classic = __any(m_ref == -INFINITY)`
                        (first), `rowsum = exps()` against nmc and `__any(!(rowsum < WIN_DEFER_SUM))` (redone), then
                        `m_new = fmaxf(m_ref, tile_max())` for every row of the wave
      fa_bidir.h        bidir_fwd_kernel, the same lines with `classic = t == 0` (every row admits key 0, so the two rules agree)
      fa_prefix.h       prefix_fwd_kernel, the same lines under `kbase <= q0 + 31 + DELTA`
      fa_atoms.h        acc_row(i, h): lane half h of row r owns keys (i & 3) + 8 * (i >> 2) + 4 * h of every 32-key sub-tile, and
                        its partial row sum runs over all BN / 32 sub-tiles of the tile
    Steps carry the number of rows that outgrew their reference and the largest lane sum of a deferred step."""
    defer_sum = DEFER_SUM if defer_sum is None else defer_sum
    admit = np.asarray(admit, bool)
    R, C = admit.shape
    nq, nk = scores.shape
    assert R % 32 == 0 and C % bn == 0 and R >= nq and C >= nk and R - nq < 32, (admit.shape, scores.shape, bn)
    s = np.zeros((R, C))
    s[:nq, :nk] = np.asarray(scores, np.float64) * tau
    s = np.where(admit, s, -np.inf)
    half = (np.arange(bn) % 32 >> 2) & 1
    out = Steps()
    with np.errstate(over="ignore", invalid="ignore"):
        for w in range(R // 32):
            rows = slice(32 * w, 32 * w + 32)
            real = min(nq - 32 * w, 32)
            tiles = walk(w // (QBLOCK // 32)) if walk else range(C // bn)
            m_ref = np.full(32, -np.inf)
            for t in tiles:
                blk = s[rows, t * bn:(t + 1) * bn]
                if blk.shape[1] == 0 or not np.isfinite(blk).any():
                    out.append(Step(w, t, "skipped", 0, real, 0.0))
                    continue
                over, lane = 0, 0.0
                if np.isinf(m_ref).any():
                    kind = "first"
                else:
                    p = np.exp(blk - m_ref[:, None])
                    sums = np.stack([p[:, half == 0].sum(1), p[:, half == 1].sum(1)])
                    big = ~(sums < defer_sum)
                    kind = "redone" if big.any() else "deferred"
                    over, lane = int(big.any(0)[:real].sum()), float(sums.max())
                    assert kind == "deferred" or over > 0   # (a padding row has P <= 1: it never outgrows)
                if kind != "deferred":
                    m_ref = np.maximum(m_ref, blk.max(1))
                out.append(Step(w, t, kind, over, real, lane))
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------------------

Case = namedtuple("Case", "lib family dtype d geom")
Problem = namedtuple("Problem", "case q k v do segments Tq Tk cu_q cu_k W S cap")

SOFTCAP = 50.0
VARLEN_LENS, VARLEN_PAD = [129, 1, 33, 200, 64], (3, 7)
BIDIR_PAIRS, BIDIR_PAD = [(129, 77), (33, 200), (200, 33), (5, 63)], ((2, 5), (4, 3))
PREFIX_PAIRS, PREFIX_PAD = [(129, 129), (257, 300), (64, 192), (200, 70)], ((5, 19), (3, 0))   # n_k - n_q = 0, 43, 128, -130 (set "X")

# window, capped: geom = (N, W, S), W = 0 standing for N.  varlen: geom = (W, S), 0 for none.  bidir, prefix: no geometry beyond the
# pairs above.  A covering selection, not the product: every (dtype, d) pair in every library, every family in every library, the
# three (W, S) shapes of the window library on both N.  (The capped build has no low_lse / high_lse case: under softcap = 50 no row's L
# leaves [-50, 50 + ln N], and exp(50) is an ordinary float.)
CASES = {
    "window": [
        Case("window", "x6", "bf16", 64, (300, 0, 0)), Case("window", "x6", "f32", 128, (200, 40, 3)),
        Case("window", "ramp_up", "bf16", 128, (200, 100, 33)), Case("window", "ramp_up", "f32", 32, (300, 0, 0)),
        Case("window", "spikes", "bf16", 32, (300, 100, 33)), Case("window", "spikes", "f32", 64, (200, 0, 0)),
        Case("window", "spikes", "bf16", 64, (200, 40, 3)),
        Case("window", "ramp_down", "bf16", 64, (300, 100, 33)), Case("window", "ramp_down", "f32", 128, (200, 40, 3)),
        Case("window", "low_lse", "bf16", 128, (200, 40, 3)), Case("window", "low_lse", "f32", 32, (300, 0, 0)),
        Case("window", "high_lse", "bf16", 32, (200, 0, 0)), Case("window", "high_lse", "f32", 64, (300, 100, 33)),
    ],
    "capped": [
        Case("capped", "x6", "bf16", 128, (200, 100, 33)), Case("capped", "x6", "f32", 128, (200, 0, 0)),
        Case("capped", "ramp_up", "f32", 64, (300, 0, 0)), Case("capped", "ramp_up", "bf16", 32, (300, 100, 33)),
        Case("capped", "spikes", "bf16", 64, (300, 0, 0)), Case("capped", "spikes", "f32", 32, (200, 40, 3)),
        Case("capped", "ramp_down", "bf16", 128, (200, 40, 3)), Case("capped", "ramp_down", "f32", 64, (200, 100, 33)),
    ],
    "varlen": [
        Case("varlen", "x6", "bf16", 64, (0, 0)), Case("varlen", "x6", "f32", 64, (40, 3)),
        Case("varlen", "ramp_up", "f32", 128, (0, 0)), Case("varlen", "ramp_up", "bf16", 32, (0, 0)),
        Case("varlen", "spikes", "bf16", 128, (40, 3)), Case("varlen", "spikes", "f32", 32, (0, 0)),
        Case("varlen", "ramp_down", "bf16", 64, (0, 0)), Case("varlen", "low_lse", "f32", 64, (0, 0)),
        Case("varlen", "high_lse", "bf16", 128, (40, 3)),
    ],
    "bidir": [
        Case("bidir", "x6", "bf16", 32, None), Case("bidir", "x6", "f32", 128, None),
        Case("bidir", "ramp_up", "bf16", 64, None), Case("bidir", "ramp_up", "f32", 32, None),
        Case("bidir", "spikes", "bf16", 128, None), Case("bidir", "spikes", "f32", 64, None),
        Case("bidir", "ramp_down", "bf16", 64, None), Case("bidir", "low_lse", "bf16", 128, None),
        Case("bidir", "high_lse", "f32", 32, None),
    ],
    "prefix": [
        Case("prefix", "x6", "bf16", 128, None), Case("prefix", "x6", "f32", 32, None),
        Case("prefix", "ramp_up", "bf16", 32, None), Case("prefix", "ramp_up", "f32", 64, None),
        Case("prefix", "spikes", "bf16", 64, None), Case("prefix", "spikes", "f32", 128, None),
        Case("prefix", "ramp_down", "f32", 64, None), Case("prefix", "low_lse", "bf16", 64, None),
        Case("prefix", "high_lse", "f32", 128, None),
    ],
}
LIBS = tuple(CASES)


def case_id(c):
    return "{}-{}-{}-d{}{}".format(c.lib, c.family, c.dtype, c.d, "" if c.geom is None else "-" + "-".join(str(g) for g in c.geom))


def _pack(lengths, lead, tail):
    cu = lead + np.concatenate([[0], np.cumsum(lengths)])
    return cu.astype(np.int32), int(cu[-1]) + tail


def problem(case):
    """The inputs of a case (seeded by the case alone) and its geometry: packed q, do (Tq, H, d) and k, v (Tk, Hkv, d); segments
    [(sq, nq, sk, nk)]; the two cu_seqlens; W and S as the call takes them (0: none); the cap (0: none)."""
    lib, name, dtype, d, geom = case
    rng = np.random.default_rng(zlib.crc32(case_id(case).encode()))
    W = S = 0
    if lib in ("window", "capped"):
        N, W, S = geom
        cu_q, Tq = _pack([N], 0, 0)
        cu_k, Tk = cu_q, Tq
    elif lib == "varlen":
        W, S = geom
        cu_q, Tq = _pack(VARLEN_LENS, *VARLEN_PAD)
        cu_k, Tk = cu_q, Tq
    else:
        pairs, (qpad, kpad) = (BIDIR_PAIRS, BIDIR_PAD) if lib == "bidir" else (PREFIX_PAIRS, PREFIX_PAD)
        cu_q, Tq = _pack([p[0] for p in pairs], *qpad)
        cu_k, Tk = _pack([p[1] for p in pairs], *kpad)
    segments = [(int(cu_q[b]), int(cu_q[b + 1] - cu_q[b]), int(cu_k[b]), int(cu_k[b + 1] - cu_k[b])) for b in range(len(cu_q) - 1)]
    delta = {"bidir": None, "prefix": "prefix"}.get(lib, 0)
    q, k, v, do = family(name, rng, dtype, (Tq, H, d), (Tk, HKV, d), segments, delta, S)
    return Problem(case, q, k, v, do, segments, Tq, Tk, cu_q, cu_k, W, S, SOFTCAP if lib == "capped" else 0.0)


def head_scores(p):
    """For every (sequence, query head) of a problem: (admit, scores, tau, walk, (seg, h)) as reference_steps takes them, and the
    scaled fp64 logits under the real mask (-inf elsewhere) for whoever wants L or P."""
    lib, _, dtype, d, _ = p.case
    Hq = p.q.shape[1]
    bn, tau, G = BN[dtype], 1.0 / np.sqrt(d), Hq // p.k.shape[1]
    for b, (sq, nq, sk, nk) in enumerate(p.segments):
        if nq == 0 or nk == 0:
            continue
        if lib == "bidir":
            admit, walk = bidir_admit(nq, nk, bn), None
        elif lib == "prefix":
            admit, walk = prefix_admit(nq, nk, bn), prefix_walk(nq, nk, bn)
        else:
            W, S = min(p.W or nq, nq), min(p.S, nq)
            admit, walk = window_admit(nq, W, S, bn), win_walk(nq, W, S, bn)
        for h in range(Hq):
            sc = p.q[sq:sq + nq, h].astype(np.float64) @ p.k[sk:sk + nk, h // G].astype(np.float64).T
            t = tau
            if p.cap:
                sc, t = p.cap * np.tanh(tau * sc / p.cap), 1.0
            yield admit, sc, t, walk, (b, h)


def model_counts(p):
    """The model over every head of a problem: dict of totals (steps, redone, whole, partial, first, deferred, skipped, max_lane_sum)."""
    tot = dict(steps=0, redone=0, whole=0, partial=0, first=0, deferred=0, skipped=0, max_lane_sum=0.0)
    for admit, sc, tau, walk, _ in head_scores(p):
        st = reference_steps(admit, sc, BN[p.case.dtype], tau, walk)
        tot["steps"] += len(st)
        for kname in ("redone", "whole", "partial"):
            tot[kname] += getattr(st, kname)
        for kname in ("first", "deferred", "skipped"):
            tot[kname] += st.count(kname)
        tot["max_lane_sum"] = max(tot["max_lane_sum"], st.max_lane_sum)
    return tot


def row_lse(p):
    """fp64 logsumexp of every real row that admits a key, all heads and sequences, as one flat array."""
    out = []
    for admit, sc, tau, _, _ in head_scores(p):
        nq, nk = sc.shape
        z = np.where(admit[:nq, :nk], sc * tau, -np.inf)
        mx = z.max(1)
        ok = np.isfinite(mx)
        out.append(mx[ok] + np.log(np.exp(z[ok] - mx[ok, None]).sum(1)))
    return np.concatenate(out)


def p_rounding_estimate(p):
    """From the reference alone: what rounding P to bf16 (2^-9 relative, 2^-9 / sqrt(3) rms) can do to the two tensors P enters
    unsplit, at four standard deviations with v, dO in U(-1, 1) (rms 1 / sqrt(3)): out_i gathers p_ij over the keys, dv_j gathers it
    over the rows of its G query heads.  (max over rows of |p_i|_2, max over keys of the group's |p_.j|_2) x 4 x 2^-9 / 3."""
    G = p.q.shape[1] // p.k.shape[1]
    worst_o, cols = 0.0, {}
    for admit, sc, tau, _, (b, h) in head_scores(p):
        nq, nk = sc.shape
        z = np.where(admit[:nq, :nk], sc * tau, -np.inf)
        mx = z.max(1, keepdims=True)
        ok = np.isfinite(mx[:, 0])
        pr = np.zeros_like(z)
        pr[ok] = np.exp(z[ok] - mx[ok])
        pr[ok] /= pr[ok].sum(1, keepdims=True)
        many = admit[:nq, :nk].sum(1) >= 64   # (rows that admit fewer take P split into two bf16 fragments)
        if many.any():
            worst_o = max(worst_o, float(np.sqrt((pr[many] ** 2).sum(1)).max()))
        cols[(b, h // G)] = cols.get((b, h // G), 0.0) + (pr ** 2).sum(0)
    worst_dv = max(float(np.sqrt(c.max())) for c in cols.values())
    f = 4.0 * 2.0 ** -9 / 3.0
    return f * worst_o, f * worst_dv
