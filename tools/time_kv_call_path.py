"""The interpreter's share of a KV-cache call: the public calls of device_ops on CPU tensors against a stub library whose every symbol
returns 0 (``is_cuda`` and ``_stream_ptr`` patched as the recorder of tests/test_device_ops_cpu.py patches them), so that what is
timed is the checks, the buffers and the argument passing.  One JSON line: microseconds per call.

    python tools/time_kv_call_path.py [--tree DIR] [--label NAME] [--calls 20000] [--repeats 1]
    python tools/time_kv_call_path.py --against DIR [--calls 2000] [--rounds 40]

``--tree``: the checkout whose package is timed (default: this one), one figure per repeat, so that two trees can be run in turn.
``--against``: PAIRED mode, the low-noise one: the package of DIR (the baseline) and of ``--tree`` are both imported into this process
and timed in turn, ``--rounds`` rounds of ``--calls`` calls each; per call the two medians, the two minima and the median of the
per-round ratios tree / baseline with their quartiles (profiles/kv_python_call_path.txt; run DIR against DIR for the A/A spread).
The first entry is one level up: a two-layer attention_stack_step_fused of modules_transformer (profiles/model_call_path.txt)."""
import argparse
import ctypes
import importlib
import importlib.util
import json
import os
import statistics
import sys
import time

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--against")
ap.add_argument("--calls", type=int)
ap.add_argument("--repeats", type=int, default=1)
ap.add_argument("--rounds", type=int, default=40)
ap.add_argument("--label", default="this tree")
args = ap.parse_args()
PACKAGE = "flash_attention_minitorch_amd"


class Stub:
    zero = staticmethod(lambda *a: 0)

    def __getattr__(self, sym):
        return self.zero


stub, null = Stub(), ctypes.c_void_p(0)
torch.Tensor.is_cuda = property(lambda self: True)


def load(alias, tree):
    """(device_ops, modules_transformer) of the package in ``tree``, imported under ``alias`` (two trees side by side), on the stub
    library."""
    path = os.path.join(os.path.abspath(tree), PACKAGE)
    spec = importlib.util.spec_from_file_location(alias, os.path.join(path, "__init__.py"), submodule_search_locations=[path])
    sys.modules[alias] = module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    lib, ops = importlib.import_module(alias + "._lib"), importlib.import_module(alias + ".device_ops")
    lib.decode = lambda: stub
    ops._stream_ptr = lambda: null
    return ops, importlib.import_module(alias + ".modules_transformer")


bf = torch.bfloat16
B, H, Hkv, Ncap, d = 2, 4, 2, 256, 64
q, kn = torch.zeros(B, 1, H, d, dtype=bf), torch.zeros(B, 1, Hkv, d, dtype=bf)
kc, vc = torch.zeros(B, Ncap, Hkv, d, dtype=bf), torch.zeros(B, Ncap, Hkv, d, dtype=bf)
kp, vp, table = torch.zeros(5, 128, Hkv, d, dtype=bf), torch.zeros(5, 128, Hkv, d, dtype=bf), torch.zeros(B, 2, dtype=torch.int32)
lens = torch.full((B,), 9, dtype=torch.int32)
out, lse, ws = torch.zeros(B, 1, H, d), torch.zeros(B, H, 1), torch.zeros(1024)
qr, cu = torch.zeros(7, H, d, dtype=bf), torch.tensor([0, 3, 7], dtype=torch.int32)
x1, wq, wk = torch.zeros(B, 1, H * d), torch.zeros(H * d, H * d), torch.zeros(H * d, Hkv * d)   # (float32: the CPU's fast matmul)


def calls(ops, model):
    cos, sin = ops.rotary_table(512, 32)
    cache, layers = model.KVCache(2, B, Ncap, H, d, torch.float32, "cpu", n_kv_head=Hkv), [(wq, wk, wk, wq)] * 2

    def model_step_fused():   # the model layer above the calls: E = 256, and the four matmuls per layer are small beside the interpreter
        cache.length_bound = 0
        model.attention_stack_step_fused(x1, layers, H, cache)
    return {
        "model_step_fused_2_layers": model_step_fused,
        "decode_slab_out_lse": lambda: ops.flash_attn_decode(q, kc, vc, lens, out=out, lse=lse),
        "decode_paged_fused_rotary": lambda: ops.flash_attn_decode(q, kp, vp, lens, k_new=kn, v_new=kn, block_table=table, rotary_cos=cos,
                                                                   rotary_sin=sin),
        "ragged_window": lambda: ops.flash_attn_ragged(qr, kc, vc, cu, lens, window=100),
        # beside the three: what tools/bench_decode.py times (caller-owned out, lse and workspace: nothing but the call path)
        "decode_slab_out_lse_workspace": lambda: ops.flash_attn_decode(q, kc, vc, lens, out=out, lse=lse, workspace=ws),
    }


def us_per_call(fn, n):
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    return (time.perf_counter() - t0) / n * 1e6


tree = calls(*load("fa_tree", args.tree))
if args.against:
    base, n, res = calls(*load("fa_base", args.against)), args.calls or 2000, {}
    for name in tree:
        tree[name](), base[name]()
        xs = [(us_per_call(base[name], n), us_per_call(tree[name], n)) for _ in range(args.rounds)]
        b, t = [x[0] for x in xs], [x[1] for x in xs]
        res[name] = {"baseline_median": round(statistics.median(b), 3), "tree_median": round(statistics.median(t), 3),
                     "baseline_min": round(min(b), 3), "tree_min": round(min(t), 3),
                     "median_ratio": round(statistics.median(y / x for x, y in xs), 3),
                     "ratio_quartiles": [round(r, 3) for r in statistics.quantiles([y / x for x, y in xs], n=4)[::2]]}
    print(json.dumps({"mode": "paired", "calls": n, "rounds": args.rounds, "us_per_call": res}))
else:
    res = {}
    for name, fn in tree.items():
        fn()
        res[name] = [round(us_per_call(fn, args.calls or 20000), 3) for _ in range(args.repeats)]
    print(json.dumps({"tree": args.label, "calls": args.calls or 20000, "us_per_call": res}))
