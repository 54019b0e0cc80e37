"""ctypes loader for the HIP libraries built by ``compile_cuda.sh``.

Mirrors the six ``ctypes.CDLL`` handles of the reference (``minitorch/cuda_kernel_ops.py:30-35``), but with
paths resolved relative to this package instead of the current directory, and lazily, so importing the
package on a machine without the build (or without a GPU) does not fail until an op is called.
"""
from __future__ import annotations

import ctypes
import os

try:  # torch first: its bundled HIP runtime must be the one (and only) libamdhip64 in the process,
    import torch  # noqa: F401  so torch stream handles / device pointers are valid in our launches.
except Exception:  # pragma: no cover - torch-less host-array use
    torch = None

KERNEL_DIR = os.environ.get(
    "FA_MI355X_KERNEL_DIR", os.path.join(os.path.dirname(os.path.abspath(__file__)), "cuda_kernels")
)

CORE_NAME = "libflash_attn_mi355x.so"
VARIANT_LIBS = (
    "flash_attn_fw.so",
    "flash_attn_bw.so",
    "flash_attn2_fw.so",
    "flash_attn2_bw.so",
    "flash_attn_causal_fw.so",
    "flash_attn_causal_bw.so",
)

FA_VARIANT_FA1 = 1
FA_VARIANT_FA2 = 2
FA_DTYPE_F32 = 0
FA_DTYPE_BF16 = 1
FA_OK = 0
FA_LAYOUT_BHND = 0
FA_LAYOUT_BNHD = 1
FA_PAGE_ROWS = 128   # a paged cache's page_size is a multiple of this (include/flash_attn_mi355x_decode.h)

_handles: dict = {}


class FlashAttnLibraryError(RuntimeError):
    pass


def lib_path(name: str) -> str:
    return os.path.join(KERNEL_DIR, name)


def load(name: str) -> ctypes.CDLL:
    """dlopen one of the built libraries; raises loudly when it is missing (no fallback path exists)."""
    h = _handles.get(name)
    if h is not None:
        return h
    path = lib_path(name)
    if not os.path.exists(path):
        raise FlashAttnLibraryError(
            f"{path} not found: build the HIP libraries first (./compile_cuda.sh, or "
            f"python -c 'import __graft_entry__ as g; g.build()').  There is no CPU fallback."
        )
    try:
        h = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL if name == CORE_NAME else ctypes.DEFAULT_MODE)
    except OSError as e:  # e.g. libamdhip64.so missing
        raise FlashAttnLibraryError(f"could not load {path}: {e}") from e
    _handles[name] = h
    return h


_vp, _i, _u, _f, _d, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_float, ctypes.c_double, ctypes.c_size_t
_ip, _dp, _s = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double), ctypes.c_char_p

# symbol -> (restype, argtypes) of every entry point of include/flash_attn_mi355x.h but the host-pointer launchers
# (tests/test_lib_cpu.py holds this table against the header)
CORE_ABI = {
    "fa_mi355x_host_pin_stats": (None, [ctypes.POINTER(ctypes.c_ulonglong)] * 2),
    "fa_mi355x_fwd": (_i, [_vp] * 6 + [_i] * 6 + [_vp]),
    "fa_mi355x_bwd_workspace_bytes": (_sz, [_i] * 3),
    "fa_mi355x_bwd_workspace_bytes_ex": (_sz, [_i] * 3 + [_ip, _i]),
    "fa_mi355x_bwd_status": (_i, [_vp] + [_i] * 3 + [_ip]),
    "fa_mi355x_bwd": (_i, [_vp] * 11 + [_i] * 6 + [_vp]),
    "fa_mi355x_bwd_stages": (_i, [_vp] * 11 + [_i] * 7 + [_vp]),
    "fa_mi355x_fwd_ex": (_i, [_vp] * 6 + [_i] * 6 + [_ip, _i, _vp]),
    "fa_mi355x_bwd_ex": (_i, [_vp] * 11 + [_i] * 7 + [_ip, _i, _vp]),
    "fa_mi355x_guard_bytes": (_sz, []),
    "fa_mi355x_scale_guard": (_i, [_vp, _vp, ctypes.c_long, _i, _i, _vp, _vp]),
    "fa_mi355x_fwd_guarded": (_i, [_vp] * 6 + [_i] * 5 + [_f] + [_i] * 3 + [_ip, _i, _vp, _i, _vp]),
    "fa_mi355x_bwd_guarded": (_i, [_vp] * 11 + [_i] * 5 + [_f] + [_i] * 4 + [_ip, _i, _vp, _vp]),
    "fa_mi355x_bwd_workspace_bytes_gqa": (_sz, [_i] * 5),
    "fa_mi355x_scale_guard_gqa": (_i, [_vp, _vp, ctypes.c_long, ctypes.c_long, _i, _i, _vp, _vp]),
    "fa_mi355x_fwd_gqa": (_i, [_vp] * 6 + [_i] * 6 + [_f] + [_i] * 3 + [_ip, _i, _vp, _i, _vp]),
    "fa_mi355x_bwd_gqa": (_i, [_vp] * 11 + [_i] * 6 + [_f] + [_i] * 4 + [_ip, _i, _vp, _vp]),
    "fa_mi355x_plan_gqa": (_i, [_i] * 9 + [_ip, _i, _s, _sz]),
    "fa_mi355x_fwd_scaled": (_i, [_vp] * 6 + [_i] * 5 + [_f] + [_i] * 3 + [_vp]),
    "fa_mi355x_bwd_scaled": (_i, [_vp] * 11 + [_i] * 5 + [_f] + [_i] * 3 + [_vp]),
    "fa_mi355x_fwd_padded": (_i, [_vp] * 6 + [_i] * 7 + [_vp]),
    "fa_mi355x_bwd_padded": (_i, [_vp] * 11 + [_i] * 7 + [_vp]),
    "fa_mi355x_plan": (_i, [_i] * 7 + [_ip, _i, _s, _sz]),
    "fa_mi355x_plan_builds": (_i, [_i] * 7 + [_ip, _i, _s, _sz]),
    "fa_mi355x_fwd_layout": (_i, [_vp] * 6 + [_i] * 8 + [_vp]),
    "fa_mi355x_bwd_layout": (_i, [_vp] * 11 + [_i] * 8 + [_vp]),
    "fa_mi355x_fwd_masked": (_i, [_vp] * 7 + [_i] * 8 + [_vp]),
    "fa_mi355x_bwd_masked": (_i, [_vp] * 12 + [_i] * 8 + [_vp]),
    "fa_mi355x_fwd_dropout": (_i, [_vp] * 7 + [_f, _f, _u] + [_i] * 8 + [_vp]),
    "fa_mi355x_bwd_dropout": (_i, [_vp] * 11 + [_f, _f, _u] + [_vp] + [_i] * 8 + [_vp]),
    "fa_mi355x_last_error": (_s, []),
    "fa_mi355x_version": (_s, []),
    "fa_mi355x_measure_mfma_peak": (_i, [_d, _dp, _dp, _vp]),
    "fa_mi355x_probe": (_i, [_vp] * 6 + [_i, _i, _vp]),
}

# the same for include/flash_attn_mi355x_decode.h
DECODE_ABI = {
    "fa_mi355x_decode_workspace_bytes": (_sz, [_i] * 5),
    "fa_mi355x_decode_splits": (_i, [_i] * 6),
    "fa_mi355x_fwd_decode": (_i, [_vp] * 7 + [_i] * 6 + [_f, _i, _i, _vp]),
    "fa_mi355x_decode_workspace_bytes_gqa": (_sz, [_i] * 6),
    "fa_mi355x_decode_splits_gqa": (_i, [_i] * 7),
    "fa_mi355x_fwd_decode_gqa": (_i, [_vp] * 7 + [_i] * 7 + [_f, _i, _i, _vp]),
    "fa_mi355x_decode_append": (_i, [_vp] * 5 + [_i] * 8 + [_vp]),
    "fa_mi355x_fwd_decode_append": (_i, [_vp] * 9 + [_i] * 8 + [_f, _i, _i, _vp]),
    "fa_mi355x_extend_splits": (_i, [_i] * 7),
    "fa_mi355x_extend_workspace_bytes": (_sz, [_i] * 6),
    "fa_mi355x_fwd_extend": (_i, [_vp] * 7 + [_i] * 7 + [_f, _i, _i, _vp]),
    "fa_mi355x_extend_append": (_i, [_vp] * 5 + [_i] * 8 + [_vp]),
    "fa_mi355x_fwd_extend_append": (_i, [_vp] * 9 + [_i] * 8 + [_f, _i, _i, _vp]),
    "fa_mi355x_decode_last_error": (_s, []),
}

# the same for include/flash_attn_mi355x_decode_paged.h (the paged forms of the same library; tests/test_paged_cpu.py)
PAGED_ABI = {
    "fa_mi355x_fwd_decode_paged": (_i, [_vp] * 8 + [_i] * 9 + [_f, _i, _i, _vp]),
    "fa_mi355x_decode_append_paged": (_i, [_vp] * 6 + [_i] * 10 + [_vp]),
    "fa_mi355x_fwd_decode_append_paged": (_i, [_vp] * 10 + [_i] * 10 + [_f, _i, _i, _vp]),
    "fa_mi355x_fwd_extend_paged": (_i, [_vp] * 8 + [_i] * 9 + [_f, _i, _i, _vp]),
    "fa_mi355x_extend_append_paged": (_i, [_vp] * 6 + [_i] * 10 + [_vp]),
    "fa_mi355x_fwd_extend_append_paged": (_i, [_vp] * 10 + [_i] * 10 + [_f, _i, _i, _vp]),
}

# the same for include/flash_attn_mi355x_decode_ragged.h (the ragged-batch forms of the same library; tests/test_ragged_cpu.py)
RAGGED_ABI = {
    "fa_mi355x_ragged_splits": (_i, [_i] * 7),
    "fa_mi355x_ragged_workspace_bytes": (_sz, [_i] * 6),
    "fa_mi355x_fwd_ragged": (_i, [_vp] * 8 + [_i] * 7 + [_f, _i, _i, _vp]),
    "fa_mi355x_ragged_append": (_i, [_vp] * 6 + [_i] * 8 + [_vp]),
    "fa_mi355x_fwd_ragged_append": (_i, [_vp] * 10 + [_i] * 8 + [_f, _i, _i, _vp]),
    "fa_mi355x_fwd_ragged_paged": (_i, [_vp] * 9 + [_i] * 9 + [_f, _i, _i, _vp]),
    "fa_mi355x_ragged_append_paged": (_i, [_vp] * 7 + [_i] * 10 + [_vp]),
    "fa_mi355x_fwd_ragged_append_paged": (_i, [_vp] * 11 + [_i] * 10 + [_f, _i, _i, _vp]),
}

# the same for include/flash_attn_mi355x_decode_window.h (the sliding-window forms of the same library; tests/test_window_cpu.py)
WINDOW_ABI = {
    "fa_mi355x_decode_window_splits": (_i, [_i] * 8),
    "fa_mi355x_decode_window_workspace_bytes": (_sz, [_i] * 7),
    "fa_mi355x_fwd_decode_window": (_i, [_vp] * 10 + [_i] * 11 + [_f, _i, _i, _i, _vp]),
    "fa_mi355x_extend_window_splits": (_i, [_i] * 8),
    "fa_mi355x_extend_window_workspace_bytes": (_sz, [_i] * 7),
    "fa_mi355x_fwd_extend_window": (_i, [_vp] * 10 + [_i] * 11 + [_f, _i, _i, _i, _vp]),
    "fa_mi355x_ragged_window_splits": (_i, [_i] * 8),
    "fa_mi355x_ragged_window_workspace_bytes": (_sz, [_i] * 7),
    "fa_mi355x_fwd_ragged_window": (_i, [_vp] * 11 + [_i] * 11 + [_f, _i, _i, _i, _vp]),
}

# the same for include/flash_attn_mi355x_decode_sink.h (the windowed forms with attention-sink tokens; tests/test_sink_cpu.py)
SINK_ABI = {
    "fa_mi355x_decode_sink_splits": (_i, [_i] * 9),
    "fa_mi355x_decode_sink_workspace_bytes": (_sz, [_i] * 8),
    "fa_mi355x_fwd_decode_sink": (_i, [_vp] * 10 + [_i] * 11 + [_f, _i, _i, _i, _i, _vp]),
    "fa_mi355x_extend_sink_splits": (_i, [_i] * 9),
    "fa_mi355x_extend_sink_workspace_bytes": (_sz, [_i] * 8),
    "fa_mi355x_fwd_extend_sink": (_i, [_vp] * 10 + [_i] * 11 + [_f, _i, _i, _i, _i, _vp]),
    "fa_mi355x_ragged_sink_splits": (_i, [_i] * 9),
    "fa_mi355x_ragged_sink_workspace_bytes": (_sz, [_i] * 8),
    "fa_mi355x_fwd_ragged_sink": (_i, [_vp] * 11 + [_i] * 11 + [_f, _i, _i, _i, _i, _vp]),
}

# the same for include/flash_attn_mi355x_decode_fp8.h (caches of e4m3 bytes with per-kv-head scales; tests/test_fp8_cpu.py)
FP8_ABI = {
    "fa_mi355x_fwd_decode_fp8": (_i, [_vp] * 12 + [_i] * 11 + [_f, _i, _i, _vp]),
    "fa_mi355x_fwd_extend_fp8": (_i, [_vp] * 12 + [_i] * 11 + [_f, _i, _i, _vp]),
    "fa_mi355x_append_fp8": (_i, [_vp] * 8 + [_i] * 11 + [_vp]),
}

# the same for include/flash_attn_mi355x_decode_rope.h (rotary embeddings: a tensor rotated, and the roped append; tests/test_rope_cpu.py)
ROPE_ABI = {
    "fa_mi355x_rope": (_i, [_vp] * 5 + [_i] * 10 + [_vp]),
    "fa_mi355x_rope_append": (_i, [_vp] * 12 + [_i] * 16 + [_vp]),
    "fa_mi355x_rope_append_ragged": (_i, [_vp] * 11 + [_i] * 15 + [_vp]),
}

# the same for include/flash_attn_mi355x_decode_softcap.h (logit soft-capping: the _window forms with `float softcap` behind the
# window; tests/test_softcap_cpu.py)
SOFTCAP_ABI = {
    "fa_mi355x_fwd_decode_softcap": (_i, [_vp] * 10 + [_i] * 11 + [_f, _i, _i, _f, _i, _vp]),
    "fa_mi355x_fwd_extend_softcap": (_i, [_vp] * 10 + [_i] * 11 + [_f, _i, _i, _f, _i, _vp]),
    "fa_mi355x_fwd_ragged_softcap": (_i, [_vp] * 11 + [_i] * 11 + [_f, _i, _i, _f, _i, _vp]),
}

# the same for include/flash_attn_mi355x_decode_lsink.h (learned sink logits: the _window forms with `const float* sink_logits`
# behind the window; tests/test_lsink_cpu.py)
LSINK_ABI = {
    "fa_mi355x_fwd_decode_lsink": (_i, [_vp] * 10 + [_i] * 11 + [_f, _i, _i, _vp, _i, _vp]),
    "fa_mi355x_fwd_extend_lsink": (_i, [_vp] * 10 + [_i] * 11 + [_f, _i, _i, _vp, _i, _vp]),
    "fa_mi355x_fwd_ragged_lsink": (_i, [_vp] * 11 + [_i] * 11 + [_f, _i, _i, _vp, _i, _vp]),
}

# The positional order of every KV-cache symbol that device_ops calls, by the parameter names of the prototypes (k_pool / v_pool of
# the _paged ones read k_cache / v_cache, T of the ragged ones Nq: one field each).  device_ops fills one dict of fields per public
# call and every C call takes its arguments from it in this order; tests/test_kv_ops_cpu.py holds the table against the headers' text
# and against the argtypes above.
_PROLOGUE = "q k_new v_new k_cache v_cache"
_PAGED = "B H Hkv Nq num_pages page_size max_pages"
_EITHER = "B H Hkv Nq Ncap num_pages page_size max_pages"
_TAIL = "layout softmax_scale causal dtype stream"
_APPEND = "k_new v_new k_cache v_cache"
KV_PARAMS = {
    "fa_mi355x_fwd_decode": f"q k_cache v_cache out lse cache_seqlens workspace B H Nq Ncap d {_TAIL}",
    "fa_mi355x_fwd_decode_gqa": f"q k_cache v_cache out lse cache_seqlens workspace B H Hkv Nq Ncap d {_TAIL}",
    "fa_mi355x_fwd_extend": f"q k_cache v_cache out lse cache_seqlens workspace B H Hkv Nq Ncap d {_TAIL}",
    "fa_mi355x_fwd_ragged": f"q k_cache v_cache out lse cu_seqlens_q cache_seqlens workspace B H Hkv Nq Ncap d {_TAIL}",
    "fa_mi355x_fwd_decode_append": f"{_PROLOGUE} out lse cache_seqlens workspace B H Hkv Nq Ncap d_new d {_TAIL}",
    "fa_mi355x_fwd_extend_append": f"{_PROLOGUE} out lse cache_seqlens workspace B H Hkv Nq Ncap d_new d {_TAIL}",
    "fa_mi355x_fwd_ragged_append": f"{_PROLOGUE} out lse cu_seqlens_q cache_seqlens workspace B H Hkv Nq Ncap d_new d {_TAIL}",
    "fa_mi355x_fwd_decode_paged": f"q k_cache v_cache out lse cache_seqlens block_table workspace {_PAGED} d {_TAIL}",
    "fa_mi355x_fwd_extend_paged": f"q k_cache v_cache out lse cache_seqlens block_table workspace {_PAGED} d {_TAIL}",
    "fa_mi355x_fwd_ragged_paged": f"q k_cache v_cache out lse cu_seqlens_q cache_seqlens block_table workspace {_PAGED} d {_TAIL}",
    "fa_mi355x_fwd_decode_append_paged": f"{_PROLOGUE} out lse cache_seqlens block_table workspace {_PAGED} d_new d {_TAIL}",
    "fa_mi355x_fwd_extend_append_paged": f"{_PROLOGUE} out lse cache_seqlens block_table workspace {_PAGED} d_new d {_TAIL}",
    "fa_mi355x_fwd_ragged_append_paged": f"{_PROLOGUE} out lse cu_seqlens_q cache_seqlens block_table workspace {_PAGED} d_new d {_TAIL}",
    "fa_mi355x_fwd_decode_window": f"{_PROLOGUE} out lse cache_seqlens block_table workspace {_EITHER} d_new d "
                                   "layout softmax_scale causal window dtype stream",
    "fa_mi355x_fwd_extend_window": f"{_PROLOGUE} out lse cache_seqlens block_table workspace {_EITHER} d_new d "
                                   "layout softmax_scale causal window dtype stream",
    "fa_mi355x_fwd_ragged_window": f"{_PROLOGUE} out lse cu_seqlens_q cache_seqlens block_table workspace {_EITHER} d_new d "
                                   "layout softmax_scale causal window dtype stream",
    "fa_mi355x_fwd_decode_sink": f"{_PROLOGUE} out lse cache_seqlens block_table workspace {_EITHER} d_new d "
                                 "layout softmax_scale causal window sink dtype stream",
    "fa_mi355x_fwd_extend_sink": f"{_PROLOGUE} out lse cache_seqlens block_table workspace {_EITHER} d_new d "
                                 "layout softmax_scale causal window sink dtype stream",
    "fa_mi355x_fwd_ragged_sink": f"{_PROLOGUE} out lse cu_seqlens_q cache_seqlens block_table workspace {_EITHER} d_new d "
                                 "layout softmax_scale causal window sink dtype stream",
    "fa_mi355x_fwd_decode_fp8": f"{_PROLOGUE} k_scale v_scale out lse cache_seqlens block_table workspace {_EITHER} d_new d {_TAIL}",
    "fa_mi355x_fwd_extend_fp8": f"{_PROLOGUE} k_scale v_scale out lse cache_seqlens block_table workspace {_EITHER} d_new d {_TAIL}",
    "fa_mi355x_decode_append": f"{_APPEND} cache_seqlens B Hkv Nq Ncap d_new d layout dtype stream",
    "fa_mi355x_extend_append": f"{_APPEND} cache_seqlens B Hkv Nq Ncap d_new d layout dtype stream",
    "fa_mi355x_ragged_append": f"{_APPEND} cu_seqlens_q cache_seqlens B Hkv Nq Ncap d_new d layout dtype stream",
    "fa_mi355x_decode_append_paged": f"{_APPEND} cache_seqlens block_table B Hkv Nq num_pages page_size max_pages d_new d layout dtype stream",
    "fa_mi355x_extend_append_paged": f"{_APPEND} cache_seqlens block_table B Hkv Nq num_pages page_size max_pages d_new d layout dtype stream",
    "fa_mi355x_ragged_append_paged": f"{_APPEND} cu_seqlens_q cache_seqlens block_table B Hkv Nq num_pages page_size max_pages d_new d "
                                     "layout dtype stream",
    "fa_mi355x_append_fp8": f"{_APPEND} k_scale v_scale cache_seqlens block_table B Hkv Nq Ncap num_pages page_size max_pages d_new d "
                            "layout dtype stream",
    "fa_mi355x_rope_append": f"q q_rot {_APPEND} k_scale v_scale cos sin cache_seqlens block_table {_EITHER} d_new d rot max_pos "
                             "layout interleaved cache_fp8 dtype stream",
    "fa_mi355x_rope_append_ragged": f"q q_rot {_APPEND} cos sin cu_seqlens_q cache_seqlens block_table {_EITHER} d_new d rot max_pos "
                                    "layout interleaved dtype stream",
    "fa_mi355x_decode_workspace_bytes": "B H Nq Ncap d",
    "fa_mi355x_decode_workspace_bytes_gqa": "B H Hkv Nq Ncap d",
    "fa_mi355x_extend_workspace_bytes": "B H Hkv Nq Ncap d",
    "fa_mi355x_ragged_workspace_bytes": "B H Hkv Nq Ncap d",
    "fa_mi355x_decode_window_workspace_bytes": "B H Hkv Nq Ncap d window",
    "fa_mi355x_extend_window_workspace_bytes": "B H Hkv Nq Ncap d window",
    "fa_mi355x_ragged_window_workspace_bytes": "B H Hkv Nq Ncap d window",
    "fa_mi355x_decode_sink_workspace_bytes": "B H Hkv Nq Ncap d window sink",
    "fa_mi355x_extend_sink_workspace_bytes": "B H Hkv Nq Ncap d window sink",
    "fa_mi355x_ragged_sink_workspace_bytes": "B H Hkv Nq Ncap d window sink",
}
KV_PARAMS = {sym: tuple(names.split()) for sym, names in KV_PARAMS.items()}   # (split once, here)
# The soft-capping symbols, likewise (tests/test_softcap_cpu.py holds them against their header and SOFTCAP_ABI).  A table of their
# own: `softcap` is the one float beside softmax_scale, and KV_PARAMS above is held by tests/test_kv_ops_cpu.py to "every argument
# that is no pointer and not softmax_scale is an int".  device_ops reads the two tables as one, KV_CALL_PARAMS.
KV_SOFTCAP_PARAMS = {
    "fa_mi355x_fwd_decode_softcap": f"{_PROLOGUE} out lse cache_seqlens block_table workspace {_EITHER} d_new d "
                                    "layout softmax_scale causal window softcap dtype stream",
    "fa_mi355x_fwd_extend_softcap": f"{_PROLOGUE} out lse cache_seqlens block_table workspace {_EITHER} d_new d "
                                    "layout softmax_scale causal window softcap dtype stream",
    "fa_mi355x_fwd_ragged_softcap": f"{_PROLOGUE} out lse cu_seqlens_q cache_seqlens block_table workspace {_EITHER} d_new d "
                                    "layout softmax_scale causal window softcap dtype stream",
}
KV_SOFTCAP_PARAMS = {sym: tuple(names.split()) for sym, names in KV_SOFTCAP_PARAMS.items()}
# The learned-sink-logit symbols, likewise (tests/test_lsink_cpu.py holds them against their header and LSINK_ABI): a table of their
# own, since tests/test_kv_ops_cpu.py holds KV_PARAMS against a fixed list of ABI tables.
KV_LSINK_PARAMS = {
    "fa_mi355x_fwd_decode_lsink": f"{_PROLOGUE} out lse cache_seqlens block_table workspace {_EITHER} d_new d "
                                  "layout softmax_scale causal window sink_logits dtype stream",
    "fa_mi355x_fwd_extend_lsink": f"{_PROLOGUE} out lse cache_seqlens block_table workspace {_EITHER} d_new d "
                                  "layout softmax_scale causal window sink_logits dtype stream",
    "fa_mi355x_fwd_ragged_lsink": f"{_PROLOGUE} out lse cu_seqlens_q cache_seqlens block_table workspace {_EITHER} d_new d "
                                  "layout softmax_scale causal window sink_logits dtype stream",
}
KV_LSINK_PARAMS = {sym: tuple(names.split()) for sym, names in KV_LSINK_PARAMS.items()}
KV_CALL_PARAMS = {**KV_PARAMS, **KV_SOFTCAP_PARAMS, **KV_LSINK_PARAMS}
KV_POINTERS = frozenset("q q_rot k_new v_new k_cache v_cache k_scale v_scale cos sin out lse cu_seqlens_q cache_seqlens block_table "
                        "workspace sink_logits stream".split())

# the same for include/flash_attn_mi355x_window.h: libflash_attn_mi355x_window.so, the sliding-window / attention-sink forward and
# backward of the training side (tests/test_window_train_cpu.py).  WINDOW_ABI above is the decode library's windowed family.
WINDOW_TRAIN_ABI = {
    "fa_mi355x_fwd_window": (_i, [_vp] * 5 + [_i] * 6 + [_f, _i, _i, _i, _vp]),
    "fa_mi355x_bwd_window_workspace_bytes": (_sz, [_i] * 5),
    "fa_mi355x_bwd_window": (_i, [_vp] * 10 + [_i] * 6 + [_f, _i, _i, _i, _vp]),
    "fa_mi355x_window_last_error": (_s, []),
}
# the same for include/flash_attn_mi355x_window_softcap.h, which the same library exports: the two calls under logit soft-capping,
# `float softcap` behind `int window` (tests/test_softcap_train_cpu.py).  A table of its own: tests/test_window_train_cpu.py holds
# the one above to the window header's symbols.
WINDOW_TRAIN_SOFTCAP_ABI = {
    "fa_mi355x_fwd_window_softcap": (_i, [_vp] * 5 + [_i] * 6 + [_f, _i, _f, _i, _i, _vp]),
    "fa_mi355x_bwd_window_softcap": (_i, [_vp] * 10 + [_i] * 6 + [_f, _i, _f, _i, _i, _vp]),
}


def _typed(name: str, abi: dict) -> ctypes.CDLL:
    """The library with restype / argtypes of every symbol in ``abi`` set (once, on first load)."""
    h = load(name)
    if not getattr(h, "_fa_typed", False):
        for sym, (res, args) in abi.items():
            fn = getattr(h, sym)
            fn.restype, fn.argtypes = res, args
        h._fa_typed = True
    return h


def core() -> ctypes.CDLL:
    """libflash_attn_mi355x.so with argtypes set for the device-pointer entry points."""
    return _typed(CORE_NAME, CORE_ABI)


_guard_elems = None


def guard_elems() -> int:
    """float32 elements of a scale guard (fa_mi355x_guard_bytes() / 4, a constant of the build: read once)."""
    global _guard_elems
    if _guard_elems is None:
        _guard_elems = core().fa_mi355x_guard_bytes() // 4
    return _guard_elems


def opts_array(opts):
    """ctypes (pointer, count) of a per-call option list for the *_ex entry points (None: defaults)."""
    if not opts:
        return None, 0
    arr = (ctypes.c_int * len(opts))(*[int(x) for x in opts])
    return arr, len(opts)


def _plan(entry, dims, causal, variant, dtype, stages, opts):
    arr, cnt = opts_array(opts)
    buf = ctypes.create_string_buffer(1024)
    check(entry(*(int(x) for x in dims), int(bool(causal)), int(variant), int(dtype), int(stages), arr, cnt, buf, 1024))
    return [x for x in buf.value.decode().split(";") if x]


def plan(batch, n, d, causal, variant, dtype, stages, opts=None):
    """Kernel names, in launch order, of the call with these arguments (fa_mi355x_plan: the library's own dispatch code with the
    launches skipped).  stages = 0: the forward; otherwise the backward stage mask."""
    return _plan(core().fa_mi355x_plan, (batch, n, d), causal, variant, dtype, stages, opts)


def plan_builds(batch, n, d, causal, variant, dtype, stages, opts=None):
    """``plan`` with one name per build instead of one per kernel family (fa_mi355x_plan_builds), e.g. DKDV_SLOT64_TILED."""
    return _plan(core().fa_mi355x_plan_builds, (batch, n, d), causal, variant, dtype, stages, opts)


def plan_gqa(B, H, Hkv, n, d, causal, variant, dtype, stages, opts=None):
    """``plan`` for a grouped-query call (fa_mi355x_plan_gqa): B * H query heads reading Hkv key/value heads per batch element."""
    return _plan(core().fa_mi355x_plan_gqa, (B, H, Hkv, n, d), causal, variant, dtype, stages, opts)


def _raise(status: int, lib: ctypes.CDLL, last_error: str, what: str) -> None:
    """The library's error: ``status`` and the message of its ``last_error`` symbol."""
    raise FlashAttnLibraryError(f"{what} error {status}: {getattr(lib, last_error)().decode()}")


def check(status: int) -> None:
    if status != FA_OK:
        _raise(status, core(), "fa_mi355x_last_error", "flash_attn_mi355x")


DECODE_NAME = "libflash_attn_mi355x_decode.so"
_DECODE_LIB_ABI = {**DECODE_ABI, **PAGED_ABI, **RAGGED_ABI, **WINDOW_ABI, **FP8_ABI, **SINK_ABI, **ROPE_ABI, **SOFTCAP_ABI, **LSINK_ABI}


def decode() -> ctypes.CDLL:
    """libflash_attn_mi355x_decode.so (include/flash_attn_mi355x_decode.h, its _paged.h, its _ragged.h, its _window.h, its _fp8.h, its
    _sink.h, its _rope.h, its _softcap.h and its _lsink.h) with argtypes set.  (Every KV-cache call comes through here: the tables are merged once, above.)"""
    return _typed(DECODE_NAME, _DECODE_LIB_ABI)


def decode_check(status: int) -> None:
    if status != FA_OK:
        _raise(status, decode(), "fa_mi355x_decode_last_error", "flash_attn_mi355x_decode")


WINDOW_NAME = "libflash_attn_mi355x_window.so"
_WINDOW_LIB_ABI = {**WINDOW_TRAIN_ABI, **WINDOW_TRAIN_SOFTCAP_ABI}


def window() -> ctypes.CDLL:
    """libflash_attn_mi355x_window.so (include/flash_attn_mi355x_window.h and its _softcap.h) with argtypes set."""
    return _typed(WINDOW_NAME, _WINDOW_LIB_ABI)


def window_check(status: int) -> None:
    if status != FA_OK:
        _raise(status, window(), "fa_mi355x_window_last_error", "flash_attn_mi355x_window")


# the same for include/flash_attn_mi355x_lsink.h: libflash_attn_mi355x_lsink.so, the training side of learned sink logits: the windowed
# forward with one logit per query head in every softmax, and the gradient of the logits (tests/test_lsink_cpu.py).  (LSINK_ABI above
# is the decode library's family.)
LSINK_TRAIN_ABI = {
    "fa_mi355x_fwd_window_lsink": (_i, [_vp] * 6 + [_i] * 6 + [_f, _i, _i, _vp]),
    "fa_mi355x_sink_logits_grad_workspace_bytes": (_sz, [_i] * 4),
    "fa_mi355x_sink_logits_grad": (_i, [_vp] * 6 + [_i] * 6 + [_vp]),
    "fa_mi355x_lsink_last_error": (_s, []),
}
LSINK_NAME = "libflash_attn_mi355x_lsink.so"


def lsink() -> ctypes.CDLL:
    """libflash_attn_mi355x_lsink.so (include/flash_attn_mi355x_lsink.h) with argtypes set."""
    return _typed(LSINK_NAME, LSINK_TRAIN_ABI)


def lsink_check(status: int) -> None:
    if status != FA_OK:
        _raise(status, lsink(), "fa_mi355x_lsink_last_error", "flash_attn_mi355x_lsink")


# the same for include/flash_attn_mi355x_varlen.h: libflash_attn_mi355x_varlen.so, the packed variable-length (cu_seqlens) forward and
# backward of the training side and the rotary embedding that restarts at every sequence (tests/test_varlen_cpu.py)
VARLEN_ABI = {
    "fa_mi355x_fwd_varlen_workspace_bytes": (_sz, [_i] * 5),
    "fa_mi355x_bwd_varlen_workspace_bytes": (_sz, [_i] * 5),
    "fa_mi355x_fwd_varlen": (_i, [_vp] * 7 + [_i] * 5 + [_f, _i, _i, _i, _vp]),
    "fa_mi355x_bwd_varlen": (_i, [_vp] * 11 + [_i] * 5 + [_f, _i, _i, _i, _vp]),
    "fa_mi355x_rope_varlen": (_i, [_vp] * 5 + [_i] * 9 + [_vp]),
    "fa_mi355x_varlen_last_error": (_s, []),
}
VARLEN_NAME = "libflash_attn_mi355x_varlen.so"


def varlen() -> ctypes.CDLL:
    """libflash_attn_mi355x_varlen.so (include/flash_attn_mi355x_varlen.h) with argtypes set."""
    return _typed(VARLEN_NAME, VARLEN_ABI)


def varlen_check(status: int) -> None:
    if status != FA_OK:
        _raise(status, varlen(), "fa_mi355x_varlen_last_error", "flash_attn_mi355x_varlen")


# the same for include/flash_attn_mi355x_bidir.h: libflash_attn_mi355x_bidir.so, the bidirectional packed forward and backward with one
# cu_seqlens for the queries and one for the keys (tests/test_bidir_cpu.py)
BIDIR_ABI = {
    "fa_mi355x_fwd_bidir_workspace_bytes": (_sz, [_i] * 6),
    "fa_mi355x_bwd_bidir_workspace_bytes": (_sz, [_i] * 6),
    "fa_mi355x_fwd_bidir": (_i, [_vp] * 8 + [_i] * 6 + [_f, _i, _vp]),
    "fa_mi355x_bwd_bidir": (_i, [_vp] * 12 + [_i] * 6 + [_f, _i, _vp]),
    "fa_mi355x_bidir_last_error": (_s, []),
}
BIDIR_NAME = "libflash_attn_mi355x_bidir.so"


def bidir() -> ctypes.CDLL:
    """libflash_attn_mi355x_bidir.so (include/flash_attn_mi355x_bidir.h) with argtypes set."""
    return _typed(BIDIR_NAME, BIDIR_ABI)


def bidir_check(status: int) -> None:
    if status != FA_OK:
        _raise(status, bidir(), "fa_mi355x_bidir_last_error", "flash_attn_mi355x_bidir")


# the same for include/flash_attn_mi355x_prefix.h: libflash_attn_mi355x_prefix.so, the causal packed forward and backward under the
# same two arrays, the queries being the last positions of the keys (tests/test_prefix_cpu.py)
PREFIX_ABI = {
    "fa_mi355x_fwd_prefix_workspace_bytes": (_sz, [_i] * 6),
    "fa_mi355x_bwd_prefix_workspace_bytes": (_sz, [_i] * 6),
    "fa_mi355x_fwd_prefix": (_i, [_vp] * 8 + [_i] * 6 + [_f, _i, _vp]),
    "fa_mi355x_bwd_prefix": (_i, [_vp] * 12 + [_i] * 6 + [_f, _i, _vp]),
    "fa_mi355x_prefix_last_error": (_s, []),
}
PREFIX_NAME = "libflash_attn_mi355x_prefix.so"


def prefix() -> ctypes.CDLL:
    """libflash_attn_mi355x_prefix.so (include/flash_attn_mi355x_prefix.h) with argtypes set."""
    return _typed(PREFIX_NAME, PREFIX_ABI)


def prefix_check(status: int) -> None:
    if status != FA_OK:
        _raise(status, prefix(), "fa_mi355x_prefix_last_error", "flash_attn_mi355x_prefix")


# the same for include/flash_attn_mi355x_local.h: libflash_attn_mi355x_local.so, the packed forward and backward under a two-sided
# sliding window, `int window_left, int window_right` behind softmax_scale, under the same two arrays (tests/test_local_cpu.py)
LOCAL_ABI = {
    "fa_mi355x_fwd_local_workspace_bytes": (_sz, [_i] * 6),
    "fa_mi355x_bwd_local_workspace_bytes": (_sz, [_i] * 6),
    "fa_mi355x_fwd_local": (_i, [_vp] * 8 + [_i] * 6 + [_f, _i, _i, _i, _vp]),
    "fa_mi355x_bwd_local": (_i, [_vp] * 12 + [_i] * 6 + [_f, _i, _i, _i, _vp]),
    "fa_mi355x_local_last_error": (_s, []),
}
LOCAL_NAME = "libflash_attn_mi355x_local.so"


def local() -> ctypes.CDLL:
    """libflash_attn_mi355x_local.so (include/flash_attn_mi355x_local.h) with argtypes set."""
    return _typed(LOCAL_NAME, LOCAL_ABI)


def local_check(status: int) -> None:
    if status != FA_OK:
        _raise(status, local(), "fa_mi355x_local_last_error", "flash_attn_mi355x_local")
