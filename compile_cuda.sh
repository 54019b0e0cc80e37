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

CORE="$OUT_DIR/libflash_attn_mi355x.so"
FLAGS=(--offload-arch="$ARCH" -O3 -std=c++17 -fPIC -shared -Wno-unused-value -mllvm -amdgpu-mfma-vgpr-form=1 -fno-slp-vectorize ${FA_EXTRA_FLAGS:-})
stale() { [ ! -f "$1" ] || [ -n "$(find "$SRC" "$HERE/include" -newer "$1" \( -name '*.h' -o -name '*.hip' \) -print -quit)" ]; }
if stale "$CORE"; then
  echo "[compile_cuda.sh] hipcc --offload-arch=$ARCH  fa_api.hip -> $CORE"
  "$HIPCC" "${FLAGS[@]}" "$SRC/fa_api.hip" -o "$CORE"
else
  echo "[compile_cuda.sh] $CORE is up to date"
fi

# KV-cache decode (include/flash_attn_mi355x_decode.h): its own library, so the training library's code object stays as it is
DECODE="$OUT_DIR/libflash_attn_mi355x_decode.so"
if [ ! -f "$DECODE" ] || [ -n "$(find "$SRC" "$HERE/include" -newer "$DECODE" \( -name '*.h' -o -name '*.hip' \) -print -quit)" ]; then
  echo "[compile_cuda.sh] hipcc --offload-arch=$ARCH  fa_decode.hip -> $DECODE"
  "$HIPCC" "${FLAGS[@]}" "$SRC/fa_decode.hip" -o "$DECODE"
else
  echo "[compile_cuda.sh] $DECODE is up to date"
fi

# Sliding-window / attention-sink forward and backward (include/flash_attn_mi355x_window.h): a third library, for the same reason
WINDOW="$OUT_DIR/libflash_attn_mi355x_window.so"
if stale "$WINDOW"; then
  echo "[compile_cuda.sh] hipcc --offload-arch=$ARCH  fa_window.hip -> $WINDOW"
  "$HIPCC" "${FLAGS[@]}" "$SRC/fa_window.hip" -o "$WINDOW"
else
  echo "[compile_cuda.sh] $WINDOW is up to date"
fi

# Packed variable-length (cu_seqlens) forward and backward (include/flash_attn_mi355x_varlen.h): a fourth library, for the same reason
VARLEN="$OUT_DIR/libflash_attn_mi355x_varlen.so"
if stale "$VARLEN"; then
  echo "[compile_cuda.sh] hipcc --offload-arch=$ARCH  fa_varlen.hip -> $VARLEN"
  "$HIPCC" "${FLAGS[@]}" "$SRC/fa_varlen.hip" -o "$VARLEN"
else
  echo "[compile_cuda.sh] $VARLEN is up to date"
fi

# Bidirectional packed attention with separate cu_seqlens for q and k (include/flash_attn_mi355x_bidir.h): a fifth library, for the same reason
BIDIR="$OUT_DIR/libflash_attn_mi355x_bidir.so"
if stale "$BIDIR"; then
  echo "[compile_cuda.sh] hipcc --offload-arch=$ARCH  fa_bidir.hip -> $BIDIR"
  "$HIPCC" "${FLAGS[@]}" "$SRC/fa_bidir.hip" -o "$BIDIR"
else
  echo "[compile_cuda.sh] $BIDIR is up to date"
fi

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
