#!/usr/bin/env python3
"""The kernel-plan grid of tests/test_plan_cpu.py and the generator of its fixture, tests/golden/plan_grid.npz.

fa_mi355x_plan needs no GPU (without a device the launch-size rules assume 256 CUs, which is what an MI355X reports), so the whole
selection logic is pinned on the CPU: every (return code, plan string) of the grid below, in its fixed nested order.  The fixture is
generated from a build of the PARENT of the change under test, never from the code under test:

    python tests/golden/make_plan_golden.py path/to/parent/libflash_attn_mi355x.so            # writes the fixture
    python tests/golden/make_plan_golden.py path/to/lib.so --dump plans.txt                   # one "rc plan" line per case instead
    python tests/golden/make_plan_golden.py path/to/lib.so --time 5                           # seconds per walk of the grid

Stored compactly: the table of distinct plan strings, one uint8 index per case, one uint8 return code per case (compressed)."""
import argparse
import ctypes
import itertools
import os
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "plan_grid.npz")

DTYPES = (0, 1)   # f32, bf16
DS = (32, 64, 128)
NS = (32, 63, 64, 128, 200, 256, 320, 512, 1024, 2000, 2048, 4096)
BATCHES = (1, 2, 8, 16, 64, 128, 256, 512)
CAUSAL = (0, 1)
VARIANTS = (1, 2)   # FA1, FA2
STAGES = (0, 1, 2, 3, 4, 6, 7)


def _opt(index, value):
    return (0,) * index + (value,)


OPTIONS = ((),) + tuple(_opt(i, v) for i, vals in ((8, (1, 2, 3)), (4, (1, 4, 5)), (0, (3, 4, 5)), (1, (2, 3, 4)), (2, (2, 3)), (5, (1,)),
                                                   (7, (1, 2))) for v in vals)
N_CASES = len(DTYPES) * len(DS) * len(NS) * len(BATCHES) * len(CAUSAL) * len(VARIANTS) * len(STAGES) * len(OPTIONS)   # 290,304


def cases():
    """(dtype, d, N, batch, causal, variant, stages, options) in the grid's fixed nested order."""
    return itertools.product(DTYPES, DS, NS, BATCHES, CAUSAL, VARIANTS, STAGES, OPTIONS)


def walk(lib):
    """[(return code, plan string)] of every case, from a ctypes handle of the core library."""
    f = lib.fa_mi355x_plan
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int] * 7 + [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
    arrays = {o: (ctypes.c_int * len(o))(*o) if o else None for o in OPTIONS}
    buf = ctypes.create_string_buffer(1024)
    out = []
    for dtype, d, n, batch, causal, variant, stages, o in cases():
        buf.value = b""
        rc = f(batch, n, d, causal, variant, dtype, stages, arrays[o], len(o), buf, 1024)
        out.append((rc, buf.value.decode()))
    return out


def load_fixture():
    with np.load(FIXTURE) as z:
        plans = [str(p) for p in z["plans"]]
        return [(int(rc), plans[i]) for rc, i in zip(z["rc"], z["index"])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lib")
    ap.add_argument("--dump")
    ap.add_argument("--time", type=int, default=0)
    args = ap.parse_args()
    lib = ctypes.CDLL(os.path.abspath(args.lib))
    if args.time:
        for _ in range(args.time):
            t0 = time.perf_counter()
            walk(lib)
            print(f"{time.perf_counter() - t0:.3f} s")
        return
    got = walk(lib)
    assert len(got) == N_CASES
    if args.dump:
        with open(args.dump, "w") as fh:
            fh.writelines(f"{rc} {plan}\n" for rc, plan in got)
        print(f"{len(got)} cases, {len(set(got))} distinct lines -> {args.dump}")
        return
    plans = sorted({p for _, p in got})
    assert len(plans) < 256
    where = {p: i for i, p in enumerate(plans)}
    np.savez_compressed(FIXTURE, plans=np.array(plans), index=np.array([where[p] for _, p in got], dtype=np.uint8),
                        rc=np.array([rc for rc, _ in got], dtype=np.uint8))
    print(f"{len(got)} cases, {len(plans)} distinct plans, return codes {sorted({rc for rc, _ in got})} -> {FIXTURE} "
          f"({os.path.getsize(FIXTURE)} bytes)")


if __name__ == "__main__":
    main()
