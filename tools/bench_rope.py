"""Rotary embeddings for the KV-cache calls on the MI355X: one JSON line per measurement.

What does the fused rotate-and-append cost, and what does it save over rotating with torch ops in front of the fused call?
Shapes (bf16, d = 128, rot = 128, NeoX pairs, [B][N][H][d], B = 32, H = 32, Hkv = 8):
  decode   Nq = 1 at length 4096
  extend   512 new tokens after a prefix of 8192
each on slab caches and through a block table (pages of 256 rows, the identity table on the same memory).  Per shape:
  (a) launch    fa_mi355x_rope_append (q -> q_rot, k rotated and v into the caches: ONE launch)   against   the plain append launch
                (k and v into the caches), with the bytes per second each achieves on a byte count from the shapes: q in and out
                (rope_append only), k and v in and out, and for rope_append one table row pair per new position of a sequence.
  (b) fused     the roped fused call (rope_append, then the attend-only call)   against   the unroped fused call (append, attention)
  (c) torch     the roped fused call   against   what a caller does without it: q and k_new rotated by torch element-wise ops (the
                table rows gathered by position, the halves multiplied and concatenated, cast back), then the unroped fused call
and once:
  (d) graph     a 4-layer GraphedStep (E = H * d = 4096, one token per step at length 4096) on a cache with rope   against   one without.
All sides of a measurement run in one process on the same tensors, window by window in turn (``--repeats`` windows per side, each of
at least ``--reps`` calls and ``--window-ms`` of device time); the baseline is measured TWICE (``base`` / ``base_again``): the A/A
ratio of the two is the noise the ratios are read against.  The baselines are the library's plain entry points, unchanged.

    python tools/bench_rope.py [--reps 20] [--warmup 3] [--repeats 5] [--window-ms 100] > profiles/rope_bench.txt
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flash_attention_minitorch_amd import _lib, device_ops, modules_transformer as mt  # noqa: E402
from bench_window import B, D, H, HKV, rnd, run  # noqa: E402

PAGE, ROT = 256, 128
SHAPES = {"decode-len4096": (False, 4095, 1), "extend-prefix8192-T512": (True, 8192, 512)}


def torch_rope(x, cos, sin, pos):
    """NeoX rotation of x (B, T, heads, D) at positions pos (B, T) with torch ops, as a caller without the library writes it."""
    c, s = cos[pos][:, :, None, :], sin[pos][:, :, None, :]
    x1, x2 = x[..., :ROT // 2].float(), x[..., ROT // 2:].float()
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).to(x.dtype)


class Case:
    """One shape: caches of ``prefix`` + T rows (``paged``: the same memory as a pool under the identity table), the T new tokens'
    q, k and v, the tables, and a q_rot buffer."""

    def __init__(self, extend, prefix, T, paged):
        g = torch.Generator(device="cuda").manual_seed(0)
        self.extend, self.T, self.N = extend, T, prefix + T
        self.kc, self.vc = rnd(g, B, self.N, HKV, D), rnd(g, B, self.N, HKV, D)
        self.q, self.kn, self.vn = rnd(g, B, T, H, D), rnd(g, B, T, HKV, D), rnd(g, B, T, HKV, D)
        self.q_rot = torch.empty_like(self.q)
        self.lens = torch.full((B,), self.N, dtype=torch.int32, device="cuda")
        self.pos = (self.lens.long()[:, None] - T + torch.arange(T, device="cuda")[None, :])
        self.cos, self.sin = device_ops.rotary_table(self.N, ROT, device="cuda")
        self.rope = dict(rotary_cos=self.cos, rotary_sin=self.sin)
        self.where = {}
        if paged:   # (the slab's memory as a pool: sequence b owns the pages b * mp .. b * mp + mp - 1)
            mp = self.N // PAGE
            assert mp * PAGE == self.N
            self.kc, self.vc = (c.view(B * mp, PAGE, HKV, D) for c in (self.kc, self.vc))
            self.where = dict(block_table=torch.arange(B * mp, dtype=torch.int32, device="cuda").view(B, mp))
        self.fn = device_ops.flash_attn_extend if extend else device_ops.flash_attn_decode
        self.ws = (device_ops.extend_workspace if extend else device_ops.decode_workspace)(self.q, self.kc, **self.where)

    # (a) the launches in front of the attention
    def append(self):
        device_ops.extend_append(self.kn, self.vn, self.kc, self.vc, self.lens, **self.where)

    def rope_append(self):
        """fa_mi355x_rope_append alone, its arguments by the names of the prototype (include/flash_attn_mi355x_decode_rope.h)."""
        table = self.where.get("block_table")
        num_pages, page_size, max_pages = (self.kc.shape[0], PAGE, table.shape[1]) if table is not None else (0, 0, 0)
        ptr = device_ops._ptr
        _lib.decode_check(device_ops._kv_call("fa_mi355x_rope_append", dict(
            q=ptr(self.q), q_rot=ptr(self.q_rot), k_new=ptr(self.kn), v_new=ptr(self.vn), k_cache=ptr(self.kc), v_cache=ptr(self.vc),
            k_scale=None, v_scale=None, cos=ptr(self.cos), sin=ptr(self.sin), cache_seqlens=ptr(self.lens), block_table=ptr(table), B=B, H=H,
            Hkv=HKV, Nq=self.T, Ncap=0 if table is not None else self.N, num_pages=num_pages, page_size=page_size, max_pages=max_pages,
            d_new=D, d=D, rot=ROT, max_pos=self.N, layout=_lib.FA_LAYOUT_BNHD, interleaved=0, cache_fp8=0, dtype=_lib.FA_DTYPE_BF16,
            stream=device_ops._stream_ptr())))

    # (b), (c) the fused calls
    def fused(self):
        return self.fn(self.q, self.kc, self.vc, self.lens, causal=True, workspace=self.ws, k_new=self.kn, v_new=self.vn, **self.where)

    def roped(self):
        return self.fn(self.q, self.kc, self.vc, self.lens, causal=True, workspace=self.ws, k_new=self.kn, v_new=self.vn, q_rot=self.q_rot,
                       **self.rope, **self.where)

    def torch_then_fused(self):
        q, kn = torch_rope(self.q, self.cos, self.sin, self.pos), torch_rope(self.kn, self.cos, self.sin, self.pos)
        return self.fn(q, self.kc, self.vc, self.lens, causal=True, workspace=self.ws, k_new=kn, v_new=self.vn, **self.where)

    def bytes(self):
        """(plain append, rope_append): q in and out, k and v in and out, one cos and one sin row per new position of a sequence."""
        kv = 2 * 2 * B * self.T * HKV * D * 2
        return kv, kv + 2 * B * self.T * H * D * 2 + 2 * self.T * (ROT // 2) * 4


def ab(sides, args):
    """sides: {"base": fn, other: fn, ...}; base is measured again at the end of every round.  -> the row's timing fields."""
    sides = dict(sides, base_again=sides["base"])
    res, reps = run(sides, args)
    m = lambda n: res[n]["median_ms"]
    row = {"calls_per_window": reps, **res, "aa": round(m("base_again") / m("base"), 3)}
    for n in sides:
        if n not in ("base", "base_again"):
            row[f"{n}_over_base"] = round(m(n) / m("base"), 3)
    return row, m


def measure(name, paged, args):
    extend, prefix, T = SHAPES[name]
    case = Case(extend, prefix, T, paged)
    head = {"shape": name, "cache": "paged" if paged else "slab", "B": B, "H": H, "Hkv": HKV, "T": T, "len": case.N, "rot": ROT}
    # the three paths compute the same thing (the torch path to rounding: it rounds as the kernel does, but contracts as it likes)
    o1, o2 = case.roped()[0].clone(), case.torch_then_fused()[0]
    torch.cuda.synchronize()
    head["max_abs_diff_roped_vs_torch_path"] = float((o1 - o2).abs().max())
    row, m = ab({"base": case.append, "rope_append": case.rope_append}, args)
    nb_plain, nb_rope = case.bytes()
    row.update(append_gbps=round(nb_plain / m("base") / 1e6, 1), rope_append_gbps=round(nb_rope / m("rope_append") / 1e6, 1),
               append_bytes=nb_plain, rope_append_bytes=nb_rope)
    print(json.dumps({**head, "what": "a-launch: rope_append / plain append (base)", **row}), flush=True)
    row, _ = ab({"base": case.fused, "roped": case.roped}, args)
    print(json.dumps({**head, "what": "b-fused: roped fused call / unroped fused call (base)", **row}), flush=True)
    row, _ = ab({"base": case.torch_then_fused, "roped": case.roped}, args)
    print(json.dumps({**head, "what": "c-torch: roped fused call / torch-op rotation + unroped fused call (base)", **row}), flush=True)


class Stepper:
    """A 4-layer GraphedStep at length 4096, rewound to that length before every window (the graph reads the lengths on the device)."""

    def __init__(self, layers, rope, start, cap):
        self.cache = mt.KVCache(len(layers), B, cap, H, D, torch.bfloat16, "cuda", n_kv_head=HKV, rope=rope)
        for t in self.cache.k + self.cache.v:
            t.uniform_(-1, 1)
        self.start, self.step = start, mt.GraphedStep(layers, H, self.cache, 1)
        self.x = torch.rand((B, 1, H * D), device="cuda").mul_(2).sub_(1).to(torch.bfloat16)
        self.rewind()

    def rewind(self):
        self.cache.lengths.fill_(self.start)
        self.cache.length_bound = self.start

    def __call__(self):
        if self.cache.length_bound + 1 > self.cache.capacity:
            self.rewind()
        return self.step.step(self.x)


def measure_graph(args):
    g = torch.Generator(device="cuda").manual_seed(1)
    E, start, cap = H * D, 4096, 4096 + 512
    layers = [tuple(rnd(g, E, c) / E ** 0.5 for c in (E, HKV * D, HKV * D, E)) for _ in range(4)]
    rope = mt.Rotary.table(cap, ROT, device="cuda")
    plain, roped = Stepper(layers, None, start, cap), Stepper(layers, rope, start, cap)
    row, _ = ab({"base": plain, "roped": roped}, args)
    print(json.dumps({"what": "d-graph: 4-layer GraphedStep with rope / without (base)", "B": B, "H": H, "Hkv": HKV, "E": E, "layers": 4,
                      "len": f"{start}..{cap}", **row}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=100.0, help="least device time of one timed window")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rope.py measures on the GPU; there is none here")
    print(json.dumps({"device": torch.cuda.get_device_name(0), "d": D, "dtype": "bf16", "layout": "bnhd", "causal": True, "rot": ROT,
                      "pairs": "neox", "reps": args.reps, "repeats": args.repeats, "page_size": PAGE}), flush=True)
    for name in SHAPES:
        for paged in (False, True):
            measure(name, paged, args)
            torch.cuda.empty_cache()
    measure_graph(args)


if __name__ == "__main__":
    main()
