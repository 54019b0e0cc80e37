#!/usr/bin/env bash
# Builds the MI355X (gfx950) FlashAttention libraries with hipcc.  Name kept from the reference
# (compile_cuda.sh / Makefile:28-50 there built the CUDA .so files with nvcc); the output directory
# holds the same six library names the reference's cuda_kernel_ops.py:30-35 opens, plus the core
# library they forward to and the KV-cache decode library.
#   OUT_DIR=minitorch/cuda_kernels ./compile_cuda.sh     # drop-in location inside a minitorch checkout
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
SRC="$HERE/flash_attention_minitorch_amd/csrc"
OUT_DIR="${OUT_DIR:-$HERE/flash_attention_minitorch_amd/cuda_kernels}"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
ARCH="${FA_ARCH:-gfx950}"
mkdir -p "$OUT_DIR"

FLAGS=(--offload-arch="$ARCH" -O3 -std=c++17 -fPIC -shared -Wno-unused-value -mllvm -amdgpu-mfma-vgpr-form=1 -fno-slp-vectorize ${FA_EXTRA_FLAGS:-})
stale() { [ ! -f "$1" ] || [ -n "$(find "$SRC" "$HERE/include" -newer "$1" \( -name '*.h' -o -name '*.hip' \) -print -quit)" ]; }
kernel_lib() {  # source stem, library suffix: one code object per library, so that a new library leaves the others' as they are
  local lib="$OUT_DIR/libflash_attn_mi355x$2.so"
  if stale "$lib"; then
    echo "[compile_cuda.sh] hipcc --offload-arch=$ARCH  $1.hip -> $lib"
    "$HIPCC" "${FLAGS[@]}" "$SRC/$1.hip" -o "$lib"
  else
    echo "[compile_cuda.sh] $lib is up to date"
  fi
}
kernel_lib fa_api    ""          # the core library: training forward and backward (include/flash_attn_mi355x.h)
kernel_lib fa_decode _decode     # KV-cache decode (include/flash_attn_mi355x_decode.h)
kernel_lib fa_window _window     # sliding-window / attention-sink forward and backward (include/flash_attn_mi355x_window.h)
kernel_lib fa_varlen _varlen     # packed variable-length (cu_seqlens) forward and backward (include/flash_attn_mi355x_varlen.h)
kernel_lib fa_bidir  _bidir      # bidirectional packed attention, cu_seqlens for q and for k (include/flash_attn_mi355x_bidir.h)
kernel_lib fa_prefix _prefix     # causal packed attention under the same two arrays, a cached prefix (include/flash_attn_mi355x_prefix.h)
kernel_lib fa_local  _local      # two-sided sliding window (a band) under the same two arrays (include/flash_attn_mi355x_local.h)
kernel_lib fa_lsink  _lsink      # learned sink logits in training: the forward and the logit gradient (include/flash_attn_mi355x_lsink.h)

shim() {  # name variant FW|BW
  "$HIPCC" -O2 -fPIC -shared -x c++ "$SRC/fa_shim.cpp" -DFA_SHIM_VARIANT="$2" -DFA_SHIM_"$3" \
      -L"$OUT_DIR" -lflash_attn_mi355x -Wl,-rpath,'$ORIGIN' -o "$OUT_DIR/$1.so"
}
shim flash_attn_fw        1 FW
shim flash_attn_bw        1 BW
shim flash_attn_causal_fw 1 FW
shim flash_attn_causal_bw 1 BW
shim flash_attn2_fw       2 FW
shim flash_attn2_bw       2 BW
echo "[compile_cuda.sh] built: $(ls "$OUT_DIR" | tr '\n' ' ')"
