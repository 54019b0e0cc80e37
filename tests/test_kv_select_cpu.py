"""The KV-cache library's kernel selection, pinned on the CPU.  tools/kv_launch_record.cpp (a host program: no GPU, no Python) loads
libflash_attn_mi355x_decode.so, answers the HIP launch calls itself and prints, for each call of a fixed grid, the return code, the
two size queries and every launch as kernel symbol : grid.x : block.x : dynamic LDS.  tests/golden/kv_launch_grid.json holds those
answers as the library gave them BEFORE its selection became a launch table.  Two builds that compute the same rows pass the GPU tests
equally; they do not pass this one.

The fixture is the recorder's output with everything that repeats interned (_pack and _unpack are each other's inverse):
  kernels    "<symbol up to its argument type>@<index into kernel_tails>", kernel_tails "<argument type>:<block.x>:<dynamic LDS>"
  sequences  the kernels of one call, in launch order
  shapes     [return code, splits, workspace bytes, grid.x of every launch]
  chunks     the sequences of consecutive calls that share a shape;  runs: [shape, chunk] in the grid's order

    python tests/test_kv_select_cpu.py <libflash_attn_mi355x_decode.so>     # records the fixture from that library
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "kv_launch_grid.json")
N_CASES, N_KERNELS = 8828, 327


def _walk(lib_path, out_dir):
    """Build the recorder with the host compiler and run it, as a child process, on lib_path: [(label, answer)] in the grid's order."""
    exe = os.path.join(str(out_dir), "kv_launch_record")
    subprocess.run([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "kv_launch_record.cpp"), "-o", exe, "-rdynamic", "-ldl"], check=True)
    out = subprocess.run([exe, lib_path], check=True, stdout=subprocess.PIPE, text=True).stdout
    return [tuple(line.split(" | ")) for line in out.splitlines()]


def _kernel_names(fixture):
    """[(symbol, ":block.x:lds")] of the fixture's kernels."""
    whole = (head + fixture["kernel_tails"][int(tail)] for head, tail in (k.split("@") for k in fixture["kernels"]))
    return [(k[:k.index(":")], k[k.index(":"):]) for k in whole]


def _unpack(fixture):
    """The recorder's answers, one string per call."""
    kernels = _kernel_names(fixture)
    answers = []
    for shape, chunk in fixture["runs"]:
        rc, splits, ws, *grids = fixture["shapes"][shape]
        for seq in fixture["chunks"][chunk]:
            launches = [f"{kernels[k][0]}:{grid}{kernels[k][1]}" for k, grid in zip(fixture["sequences"][seq], grids)]
            answers.append(" ".join([str(rc), str(splits), str(ws)] + launches))
    return answers


def _pack(answers):
    tails, kernels, shapes, sequences, chunks, runs = {}, {}, {}, {}, {}, []

    def kernel(name, block, lds):
        cut = name.index("EEv") if "EEv" in name else len(name)
        return kernels.setdefault(f"{name[:cut]}@{tails.setdefault(f'{name[cut:]}:{block}:{lds}', len(tails))}", len(kernels))

    for answer in answers:
        rc, splits, ws, *launches = answer.split(" ")
        launches = [l.split(":") for l in launches]
        shape = shapes.setdefault((int(rc), int(splits), int(ws)) + tuple(int(l[1]) for l in launches), len(shapes))
        if not runs or runs[-1][0] != shape:
            runs.append([shape, []])
        runs[-1][1].append(sequences.setdefault(tuple(kernel(l[0], l[2], l[3]) for l in launches), len(sequences)))
    runs = [[shape, chunks.setdefault(tuple(chunk), len(chunks))] for shape, chunk in runs]
    return {"cases": len(answers), "kernel_tails": list(tails), "kernels": list(kernels), "sequences": list(sequences),
            "shapes": list(shapes), "chunks": list(chunks), "runs": runs}


def test_every_call_launches_what_the_recorded_library_launched(tmp_path):
    import __graft_entry__ as g
    g.build()
    from flash_attention_minitorch_amd import _lib

    with open(FIXTURE) as f:
        fixture = json.load(f)
    want = _unpack(fixture)
    assert len(want) == fixture["cases"] == N_CASES   # the grid as the issue states it: a shortened one cannot pass
    got = _walk(_lib.lib_path(_lib.DECODE_NAME), tmp_path)
    assert len(got) == N_CASES
    bad = [(label, g_, w) for (label, g_), w in zip(got, want) if g_ != w]
    assert not bad, f"{len(bad)} of {len(got)} calls differ; first (call, got, recorded): {bad[:3]}"
    # every kernel the recorded library launched is still launched
    launched = {l.split(":")[0] for _, a in got for l in a.split(" ")[3:]}
    assert launched == {name for name, _ in _kernel_names(fixture)} and len(launched) == N_KERNELS


if __name__ == "__main__":
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        recorded = [answer for _, answer in _walk(sys.argv[1], tmp)]
    packed = _pack(recorded)
    assert _unpack(packed) == recorded
    with open(FIXTURE, "w") as f:   # (one key to a line)
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}:{json.dumps(v, separators=(',', ':'))}" for k, v in packed.items()) + "\n}\n")
    print(f"{len(recorded)} calls, {len(packed['kernels'])} kernels -> {FIXTURE}")
