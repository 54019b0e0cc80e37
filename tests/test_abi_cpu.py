"""CPU-side checks of the drop-in boundary: every symbol include/flash_attn_mi355x.h declares is exported by
the built libraries, the six reference library names exist, argument validation works without a GPU, and the
host-array operator surface enforces the reference's preconditions.  No compute calls (no GPU here)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from flash_attention_minitorch_amd import _lib
    return _lib


def _declared_symbols():
    """Entry points the header declares."""
    text = open(os.path.join(ROOT, "include", "flash_attn_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b((?:launch_flash_attn|fa_mi355x)_\w+)\s*\(", text)))


def test_header_declares_expected_entry_points():
    syms = _declared_symbols()
    for s in ("launch_flash_attn_fw", "launch_flash_attn_bw", "fa_mi355x_fwd", "fa_mi355x_bwd",
              "fa_mi355x_bwd_workspace_bytes", "fa_mi355x_launch_fw_host", "fa_mi355x_launch_bw_host",
              "fa_mi355x_bwd_stages", "fa_mi355x_fwd_layout", "fa_mi355x_bwd_layout", "fa_mi355x_fwd_masked", "fa_mi355x_bwd_masked", "fa_mi355x_fwd_dropout", "fa_mi355x_bwd_dropout", "fa_mi355x_last_error", "fa_mi355x_version", "fa_mi355x_fwd_ex", "fa_mi355x_bwd_ex", "fa_mi355x_bwd_status", "fa_mi355x_measure_mfma_peak", "fa_mi355x_probe", "fa_mi355x_plan", "fa_mi355x_fwd_padded", "fa_mi355x_bwd_padded", "fa_mi355x_fwd_scaled", "fa_mi355x_bwd_scaled"):
        assert s in syms


def test_core_library_exports_every_declared_symbol(built):
    core = built.core()
    for s in _declared_symbols():
        if s.startswith("launch_flash_attn"):
            continue
        assert hasattr(core, s), s


@pytest.mark.parametrize("name", ["flash_attn_fw.so", "flash_attn2_fw.so", "flash_attn_causal_fw.so"])
def test_forward_shims_export_reference_symbol(built, name):
    lib = built.load(name)
    assert hasattr(lib, "launch_flash_attn_fw")      # src/flash_attn_fw.cu:302
    out = subprocess.run(["nm", "-D", "--defined-only", built.lib_path(name)], capture_output=True, text=True).stdout
    assert " T launch_flash_attn_fw" in out and "launch_flash_attn_bw" not in out


@pytest.mark.parametrize("name", ["flash_attn_bw.so", "flash_attn2_bw.so", "flash_attn_causal_bw.so"])
def test_backward_shims_export_reference_symbol(built, name):
    lib = built.load(name)
    assert hasattr(lib, "launch_flash_attn_bw")      # src/flash_attn_bw.cu:277
    out = subprocess.run(["nm", "-D", "--defined-only", built.lib_path(name)], capture_output=True, text=True).stdout
    assert " T launch_flash_attn_bw" in out and "launch_flash_attn_fw" not in out


def _device_kernels(path):
    """(name, private_segment_fixed_size, vgpr_count) of every kernel in the gfx950 code object bundled in a built library."""
    import struct
    import tempfile
    objcopy, readelf = "/opt/rocm/lib/llvm/bin/llvm-objcopy", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    with tempfile.TemporaryDirectory() as td:
        fat = os.path.join(td, "fat.bin")
        subprocess.run([objcopy, "--dump-section", ".hip_fatbin=" + fat, path, os.path.join(td, "x")], check=True)
        b = open(fat, "rb").read()
        assert b.startswith(b"__CLANG_OFFLOAD_BUNDLE__")
        n = struct.unpack_from("<Q", b, 24)[0]
        off, co = 32, None
        for _ in range(n):
            o, sz, tl = struct.unpack_from("<QQQ", b, off)
            off += 24
            triple = b[off:off + tl].decode()
            off += tl
            if "gfx950" in triple:
                co = os.path.join(td, "dev.co")
                open(co, "wb").write(b[o:o + sz])
        assert co, "no gfx950 code object in " + path
        notes = subprocess.run([readelf, "--notes", co], capture_output=True, text=True, check=True).stdout
    out = []
    for blk in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
        vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1))
        out.append((name, scratch, vgpr))
    return out


def test_product_library_has_no_diagnostic_code_and_no_scratch(built):
    """no stamp build, timing ablation or tuning entry point in the library, and no kernel of it uses scratch
    memory (round 3: no exception left; the one-pass backward, which kept 8 B per lane, was retired)."""
    path = built.lib_path("libflash_attn_mi355x.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    for s in ("fa_mi355x_set_tuning", "fa_mi355x_debug_phase_cycles", "g_phase_cycles"):
        assert s not in syms, s
    kernels = _device_kernels(path)
    assert len(kernels) > 40
    for name, scratch, vgpr in kernels:
        assert vgpr <= 512
        assert scratch == 0, (name, scratch)
    # the retired stamp / register-staging builds of dK/dV (MODE 9 / 13 / 93) and the bf16 one-pass backwards
    names = " ".join(k[0] for k in kernels)
    assert not re.search(r"bwd_dkdv_kernelI\S*Li(9|13|93)ELb", names)
    assert "bwd_fused_kernel" not in names and "bwd_chain_kernel" not in names
    assert len(kernels) < 98, len(kernels)   # round 3 library diet (133 before, 88 then; round 4: + two scale-guard kernels, + four builds of the fp32 one-pass backward)


def test_library_contains_gfx950_code_object(built):
    blob = open(built.lib_path(built.CORE_NAME), "rb").read()
    assert b"gfx950" in blob
    assert b"fwd_kernel" in blob and b"bwd_dkdv_kernel" in blob and b"bwd_dq_kernel" in blob


def test_argument_validation_without_gpu(built):
    core = built.core()
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(16)
    assert core.fa_mi355x_version().decode().startswith("flash_attn_mi355x")
    # three row-constant vectors: -L/tau, -rowsum(dO*O), -L*log2(e)
    assert core.fa_mi355x_bwd_workspace_bytes(64, 4096, 128) == 3 * 64 * 4096 * 4
    assert core.fa_mi355x_bwd_workspace_bytes(64, 4100, 64) == 3 * 64 * 4100 * 4      # not a one-pass shape
    assert core.fa_mi355x_bwd_workspace_bytes(64, 4096, 64) == 3 * 64 * 4096 * 4
    assert core.fa_mi355x_bwd_workspace_bytes(0, 4096, 64) == 0
    # with options: no kernel of the library needs more, whatever the options say (opts[4] = 3 once sized a retired kernel's slabs)
    core.fa_mi355x_bwd_workspace_bytes_ex.restype = ctypes.c_size_t
    chain = (ctypes.c_int * 5)(0, 0, 0, 0, 3)
    assert core.fa_mi355x_bwd_workspace_bytes_ex(64, 4096, 64, chain, 5) == 3 * 64 * 4096 * 4
    assert core.fa_mi355x_bwd_workspace_bytes_ex(64, 4096, 64, None, 0) == 3 * 64 * 4096 * 4
    # round 4: the scale guard and the guarded entry points validate their arguments before any HIP call as well
    core.fa_mi355x_guard_bytes.restype = ctypes.c_size_t
    assert core.fa_mi355x_guard_bytes() == 2 * 256 * 4
    core.fa_mi355x_scale_guard.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    assert core.fa_mi355x_scale_guard(null, one, 16, 64, 1, one, null) == 1 and core.fa_mi355x_scale_guard(one, one, 0, 64, 1, one, null) == 1
    assert core.fa_mi355x_scale_guard(one, one, 16, 64, 7, one, null) == 1
    fw = core.fa_mi355x_fwd_guarded
    fw.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_int] * 5 + [ctypes.c_float] + [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                                                                                                    ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    assert fw(one, one, one, one, one, one, 1, 1, 16, 64, 0, 0.0, 0, 2, 1, None, 0, null, 1, null) == 1      # produce_guard without a guard
    assert b"produce_guard" in core.fa_mi355x_last_error()
    assert fw(one, one, one, one, one, one, 1, 1, 16, 64, 0, -1.0, 0, 2, 1, None, 0, null, 0, null) == 1     # negative softmax_scale
    assert fw(one, one, one, one, one, one, 1, 1, 16, 64, 5, 0.0, 0, 2, 1, None, 0, null, 0, null) == 1      # unknown layout
    assert fw(one, one, one, one, one, one, 1, 1, 16, 48, 0, 0.0, 0, 2, 1, None, 0, null, 0, null) == 2      # head dim
    mode9 = (ctypes.c_int * 10)(0, 0, 0, 0, 0, 0, 0, 0, 4, 0)
    assert fw(one, one, one, one, one, one, 1, 1, 16, 64, 0, 0.0, 0, 2, 1, mode9, 10, null, 0, null) == 1    # option 8 = 4 does not exist
    # per-call options: values outside the table (e.g. the retired stamp build 93) are rejected before any HIP call
    bad = (ctypes.c_int * 3)(93, 0, 0)
    assert core.fa_mi355x_fwd_ex(one, one, one, one, one, one, 1, 16, 64, 0, 2, 0, bad, 3, null) == 1
    assert b"diagnostic" in core.fa_mi355x_last_error()
    assert core.fa_mi355x_fwd_ex(one, one, one, one, one, one, 1, 16, 64, 0, 2, 0, None, 9, null) == 1
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(16)
    # bad sizes / null pointers / unsupported d are rejected before any HIP call
    assert core.fa_mi355x_fwd(one, one, one, one, one, one, 0, 16, 64, 0, 2, 0, null) == 1
    assert core.fa_mi355x_fwd(null, one, one, one, one, one, 1, 16, 64, 0, 2, 0, null) == 1
    assert core.fa_mi355x_fwd(one, one, one, one, one, one, 1, 16, 64, 0, 7, 0, null) == 1
    assert core.fa_mi355x_fwd(one, one, one, one, one, one, 1, 16, 64, 0, 2, 9, null) == 1
    assert core.fa_mi355x_fwd(one, one, one, one, one, one, 1, 16, 34, 0, 2, 0, null) == 2
    assert b"32, 64, 128" in core.fa_mi355x_last_error()
    assert core.fa_mi355x_fwd(one, one, one, one, one, null, 1, 16, 64, 0, 1, 0, null) == 1   # FA-1 needs m
    with pytest.raises(built.FlashAttnLibraryError):
        built.check(2)


def test_missing_library_fails_loudly(built, monkeypatch, tmp_path):
    monkeypatch.setattr(built, "KERNEL_DIR", str(tmp_path))
    monkeypatch.setattr(built, "_handles", {})
    with pytest.raises(built.FlashAttnLibraryError, match="no CPU fallback"):
        built.load("flash_attn2_fw.so")


def test_operator_surface_preconditions(built):
    from flash_attention_minitorch_amd import CudaKernelOps
    q = np.zeros((1, 2, 8, 64), np.float32)
    k = np.zeros((1, 2, 9, 64), np.float32)
    with pytest.raises(AssertionError):   # minitorch/cuda_kernel_ops.py:531
        CudaKernelOps.flash_attn2_fw(q, k, q, True)
    with pytest.raises(AssertionError):   # :592-593 l/m shape
        CudaKernelOps.flash_attn2_bw(q, q, q, q, q, np.zeros((1, 2, 7), np.float32), np.zeros((1, 2, 8), np.float32), 1)
    from flash_attention_minitorch_amd.cuda_kernel_ops import _causal_flag
    assert _causal_flag(True) and _causal_flag(np.array([1.0])) and not _causal_flag(0) and not _causal_flag([0.0])


def test_product_path_does_not_import_oracle():
    pkg = os.path.join(ROOT, "flash_attention_minitorch_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".cpp")):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M), f
    code = ("import sys; import flash_attention_minitorch_amd, flash_attention_minitorch_amd.device_ops, "
            "flash_attention_minitorch_amd.sharded; assert not any(m == 'oracle' or m.startswith('oracle.') "
            "for m in sys.modules)")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_native_backtrace_hook_fires_on_abort(tmp_path):
    """tests/abort_trace.c (the SIGABRT / SIGSEGV hook of the GPU runs) is itself tested: see gpu_util.check_abort_hook."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from gpu_util import check_abort_hook
    check_abort_hook(tmp_path)


def test_deterministic_switch_keeps_the_two_kernel_fp32_backward(built):
    """FA_MI355X_DETERMINISTIC=1 (read once per process: a child): the fp32 d = 64 backward stays on two kernels (dq bitwise repeatable)
    for callers of the reference ABI, which has no options argument; option 4 = 5 still forces the one-pass kernel.  fa_mi355x_plan
    runs the library's own dispatch without a GPU."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from flash_attention_minitorch_amd import _lib\n"
            "f32 = _lib.FA_DTYPE_F32\n"
            "print(_lib.plan(64, 2048, 64, False, 2, f32, 7, None), _lib.plan(64, 2048, 64, False, 2, f32, 7, (0, 0, 0, 0, 5)))\n") % root
    out = {}
    for val in ("0", "1"):
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120,
                           env=dict(os.environ, FA_MI355X_DETERMINISTIC=val))
        assert r.returncode == 0, r.stderr[-1000:]
        out[val] = r.stdout.strip()
    assert out["0"] == "['bwd_prep_kernel', 'bwd_onepass_f32_kernel'] ['bwd_prep_kernel', 'bwd_onepass_f32_kernel']", out["0"]
    assert out["1"] == "['bwd_dq_kernel', 'bwd_dkdv_kernel'] ['bwd_prep_kernel', 'bwd_onepass_f32_kernel']", out["1"]


# ---- validation of the device entry points, pinned argument by argument ------------------------------------------------------------
# Every call below is rejected before any HIP call (fake non-null pointers are never dereferenced).  No valid call is made here: on a
# GPU machine it would launch kernels on those pointers.
_P6 = ["q", "k", "v", "out", "l", "m"]
_P11 = ["q", "k", "v", "out", "dout", "dq", "dk", "dv", "l", "m", "ws"]
_P10 = _P11[:-1]
_ENTRY_ARGS = {
    "fwd": _P6 + ["batch", "N", "d", "causal", "variant", "dtype", "stream"],
    "fwd_ex": _P6 + ["batch", "N", "d", "causal", "variant", "dtype", "opts", "nopts", "stream"],
    "fwd_scaled": _P6 + ["B", "H", "N", "d", "layout", "scale", "causal", "variant", "dtype", "stream"],
    "fwd_padded": _P6 + ["batch", "N", "d", "dp", "causal", "variant", "dtype", "stream"],
    "fwd_layout": _P6 + ["B", "H", "N", "d", "layout", "causal", "variant", "dtype", "stream"],
    "fwd_masked": _P6 + ["mask", "B", "H", "N", "d", "layout", "causal", "variant", "dtype", "stream"],
    "fwd_dropout": _P6 + ["mask", "rate", "dscale", "seed", "B", "H", "N", "d", "layout", "causal", "variant", "dtype", "stream"],
    "fwd_guarded": _P6 + ["B", "H", "N", "d", "layout", "scale", "causal", "variant", "dtype", "opts", "nopts", "guard", "produce",
                          "stream"],
    "bwd": _P11 + ["batch", "N", "d", "causal", "variant", "dtype", "stream"],
    "bwd_stages": _P11 + ["batch", "N", "d", "causal", "variant", "dtype", "stages", "stream"],
    "bwd_ex": _P11 + ["batch", "N", "d", "causal", "variant", "dtype", "stages", "opts", "nopts", "stream"],
    "bwd_scaled": _P11 + ["B", "H", "N", "d", "layout", "scale", "causal", "variant", "dtype", "stream"],
    "bwd_padded": _P11 + ["batch", "N", "d", "dp", "causal", "variant", "dtype", "stream"],
    "bwd_layout": _P11 + ["B", "H", "N", "d", "layout", "causal", "variant", "dtype", "stream"],
    "bwd_masked": _P10 + ["mask", "ws", "B", "H", "N", "d", "layout", "causal", "variant", "dtype", "stream"],
    "bwd_dropout": _P10 + ["mask", "rate", "dscale", "seed", "ws", "B", "H", "N", "d", "layout", "causal", "variant", "dtype",
                           "stream"],
    "bwd_guarded": _P11 + ["B", "H", "N", "d", "layout", "scale", "causal", "variant", "dtype", "stages", "opts", "nopts", "guard",
                           "stream"],
    "plan": ["batch", "N", "d", "causal", "variant", "dtype", "stages", "opts", "nopts", "pout", "pn"],
}
_VALID = dict(batch=1, B=1, H=2, N=16, d=64, dp=64, layout=0, scale=0.125, causal=0, variant=2, dtype=1, stages=7, opts=None,
              nopts=0, mask=None, rate=0.0, dscale=1.0, seed=0, produce=0, pn=1024)
_FLOAT_ARGS = ("scale", "rate", "dscale")
_D_MSG = "device path supports d in {32, 64, 128}"
_PADDED_MSG = "padded row length dp must be 32, 64 or 128 and >= d"
_NULL = (1, "null pointer argument")
_BATCH = (1, "batch, N and d must be positive")
_BH = (1, "B and H must be positive")
_OPTS = (1, "option value not supported")
_STAGES = (1, "bad stages mask")
_LAYOUT = (1, "unknown layout")
_GIB = (1, "one batch element must stay under 2 GiB")
_SCALE = (1, "softmax_scale must be positive and finite")


def _single_bad_cases(entry):
    """(overrides, rc, message substring) for each single bad argument the entry point takes."""
    args = _ENTRY_ARGS[entry]
    padded = "dp" in args
    cases = []
    for p in args:
        if p in _P11 and not (entry == "fwd_guarded" and p == "guard"):
            cases.append(({p: None, "variant": 1} if p == "m" else {p: None}, *_NULL))
    if "opts" in args:
        cases += [({"opts": (93, 0, 0), "nopts": 3}, *_OPTS), ({"opts": (0,) * 8 + (4, 0), "nopts": 10}, *_OPTS),
                  ({"opts": None, "nopts": 9}, 1, "bad options array"), ({"opts": (0,) * 11, "nopts": 11}, 1, "bad options array"),
                  ({"opts": (0,), "nopts": -1}, 1, "bad options array")]
    if "stages" in args:
        cases += [({"stages": 8}, *_STAGES), ({"stages": -1}, *_STAGES)]
        if entry != "plan":
            cases.append(({"stages": 0}, *_STAGES))
    if "B" in args:
        cases += [({"B": 0}, *_BH), ({"H": 0}, *_BH), ({"B": -3}, *_BH), ({"layout": 5}, *_LAYOUT), ({"layout": -1}, *_LAYOUT),
                  ({"H": 64, "N": 65536, "d": 128}, *_GIB)]
    else:
        cases.append(({"batch": 0}, *_BATCH))
    cases += [({"N": 0}, *_BATCH), ({"N": 1 << 22}, 1, "N too large"), ({"d": 0}, *_BATCH), ({"d": -64}, *_BATCH),
              ({"variant": 7}, 1, "unknown variant"), ({"variant": 0}, 1, "unknown variant"), ({"dtype": 9}, 1, "unknown dtype")]
    if padded:
        cases += [({"dp": 48}, 2, _PADDED_MSG), ({"d": 128, "dp": 64}, 2, _PADDED_MSG), ({"d": 48, "dp": 48}, 2, _PADDED_MSG),
                  ({"dp": 0}, 2, _PADDED_MSG)]
    else:
        cases += [({"d": 48}, 2, _D_MSG), ({"d": 256}, 2, _D_MSG), ({"d": 34}, 2, _D_MSG)]
    if entry in ("fwd_scaled", "bwd_scaled"):
        cases += [({"scale": 0.0}, *_SCALE), ({"scale": -1.0}, *_SCALE), ({"scale": float("nan")}, *_SCALE),
                  ({"scale": float("inf")}, *_SCALE)]
    if entry in ("fwd_guarded", "bwd_guarded"):
        cases += [({"scale": -1.0}, 1, "(0: sqrt(1/d))"), ({"scale": float("nan")}, 1, "(0: sqrt(1/d))"),
                  ({"scale": float("inf")}, 1, "(0: sqrt(1/d))")]
    if entry == "fwd_guarded":
        cases.append(({"produce": 1, "guard": None}, 1, "produce_guard needs a guard buffer"))
    if "rate" in args:
        cases += [({"rate": 1.0}, 1, "dropout rate must be in [0, 1)"), ({"rate": -0.25}, 1, "dropout rate must be in [0, 1)"),
                  ({"rate": float("nan")}, 1, "dropout rate must be in [0, 1)")]
    if entry == "plan":
        cases += [({"pout": None}, 1, "null output buffer"), ({"pn": 0}, 1, "null output buffer"),
                  ({"pn": 4}, 1, "plan buffer too small")]
    return cases


def _multi_bad_cases(entry):
    """Several bad arguments at once: the first failing check of the entry point's order decides."""
    args = _ENTRY_ARGS[entry]
    ptr = "v"
    cases = [({"variant": 7, ptr: None}, 1, "unknown variant"), ({"dtype": 9, "d": 48}, 1, "unknown dtype"),
             ({ptr: None, "d": 48}, *_NULL)] if entry != "plan" else [({"variant": 7, "d": 48}, 1, "unknown variant")]
    if "opts" in args:
        cases += [({"opts": (93,), "nopts": 1, "N": 0}, *_OPTS)]
        cases += [({"opts": (93,), "nopts": 1, "stages": 0 if entry != "plan" else -1}, *_OPTS)] if "stages" in args else []
    if "stages" in args:
        cases += [({"stages": 9, "N": 0}, *_STAGES)]
        if "B" in args:
            cases += [({"stages": 9, "B": 0}, *_STAGES)]
    if "B" in args:
        cases += [({"B": 0, "N": 0}, *_BH), ({"H": 0, ptr: None}, *_BH), ({"layout": 5, "d": 48}, 2, _D_MSG),
                  ({"layout": 5, "H": 64, "N": 65536, "d": 128}, *_LAYOUT), ({ptr: None, "layout": 5}, *_NULL)]
    if "scale" in args:
        cases += [({"scale": -1.0, "layout": 5}, *_LAYOUT), ({"scale": -1.0, "H": 64, "N": 65536, "d": 128}, *_SCALE)]
    if "rate" in args:
        cases += [({"rate": 2.0, "H": 64, "N": 65536, "d": 128}, *_GIB), ({"rate": 2.0, "layout": 5}, *_LAYOUT),
                  ({"rate": 2.0, ptr: None}, *_NULL)]
    if entry == "fwd_guarded":
        cases += [({"produce": 1, "guard": None, "d": 48}, 1, "produce_guard"), ({"produce": 1, "guard": None, ptr: None}, *_NULL),
                  ({"produce": 1, "guard": None, "layout": 5}, 1, "produce_guard")]
    if "dp" in args:
        cases += [({"dp": 48, ptr: None}, *_NULL), ({"dp": 48, "N": 0}, *_BATCH)]
    if entry == "plan":
        cases += [({"pout": None, "d": 48}, 2, _D_MSG), ({"pout": None, "stages": 8}, *_STAGES)]
    return cases


def _call_entry(lib, entry, overrides):
    """Calls fa_mi355x_<entry> with the valid defaults, fake non-null pointers and the overrides; returns (rc, last error)."""
    args = dict(_VALID, **overrides)
    keep = []
    vals = []
    for name in _ENTRY_ARGS[entry]:
        if name == "stream":
            vals.append(ctypes.c_void_p(0))
        elif name in _P11 or name == "guard":
            vals.append(ctypes.c_void_p(16) if args.get(name, 16) is not None else ctypes.c_void_p(0))
        elif name == "mask":
            vals.append(ctypes.c_void_p(0) if args["mask"] is None else ctypes.c_void_p(16))
        elif name == "opts":
            arr = None if args["opts"] is None else (ctypes.c_int * max(1, len(args["opts"])))(*args["opts"])
            keep.append(arr)
            vals.append(arr)
        elif name == "pout":
            buf = ctypes.create_string_buffer(1024) if args.get("pout", 1) is not None else None
            keep.append(buf)
            vals.append(buf)
        elif name == "pn":
            vals.append(ctypes.c_size_t(args["pn"]))
        elif name in _FLOAT_ARGS:
            vals.append(ctypes.c_float(args[name]))
        elif name == "seed":
            vals.append(ctypes.c_uint(args[name]))
        else:
            vals.append(ctypes.c_int(args[name]))
    rc = getattr(lib, "fa_mi355x_" + entry)(*vals)   # (the values carry their own ctypes types)
    return rc, lib.fa_mi355x_last_error().decode()


@pytest.mark.parametrize("entry", sorted(_ENTRY_ARGS))
def test_entry_point_validation_table(built, entry):
    """Each device entry point answers every single bad argument, and combinations of them, with the return code and message of the
    first failing check in its order: options, stages, B/H, batch / N / d / variant / dtype / N size, null pointers, produce_guard
    without a guard, d (or dp), layout, softmax scale, one batch element under 2 GiB, dropout rate (fa_mi355x_plan: its output
    buffer last)."""
    lib = ctypes.CDLL(built.lib_path(built.CORE_NAME))   # a handle of its own: core()'s argtypes stay as they are
    lib.fa_mi355x_last_error.restype = ctypes.c_char_p
    for overrides, rc, msg in _single_bad_cases(entry) + _multi_bad_cases(entry):
        got_rc, got_msg = _call_entry(lib, entry, overrides)
        assert (got_rc, msg in got_msg) == (rc, True), (entry, overrides, got_rc, got_msg)
