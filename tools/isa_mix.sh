#!/usr/bin/env bash
# Device assembly of the kernel libraries (csrc/fa_api.hip, csrc/fa_decode.hip, csrc/fa_window.hip, csrc/fa_varlen.hip, csrc/fa_bidir.hip, csrc/fa_prefix.hip, csrc/fa_local.hip, csrc/fa_lsink.hip), built with compile_cuda.sh's flags + -save-temps.
#   tools/isa_mix.sh mix   <tree> <out-dir> <mangled-kernel-substring>...   resource usage + per-basic-block instruction mix (fa_api)
#   tools/isa_mix.sh split <tree> <out-dir>                                 one normalised .s per kernel: <out-dir>/kernels/<lib>/<kernel>.s
# <tree> is a checkout of this repository, <out-dir> receives the temporaries (FA_ISA_NOBUILD=1: reuse what is there).
# split writes, for every .amdhsa_kernel symbol, the text from its label to its .Lfunc_end (the .amdhsa_* descriptor block lies in
# between) with the function index taken out of the local labels and the ';' comments dropped (they carry the names of compiler-
# internal IR blocks, whose numbering moves with unrelated edits), so that two trees compare with
#   diff -r <out-a>/kernels <out-b>/kernels
set -euo pipefail
usage() {
  echo "usage: $0 mix <tree> <out-dir> <mangled-kernel-substring>..." >&2
  echo "       $0 split <tree> <out-dir>" >&2
  exit 2
}
[ $# -ge 3 ] || usage
MODE=$1
TREE=$(cd "$2" && pwd)
mkdir -p "$3"
OUT=$(cd "$3" && pwd)
shift 3
SRC="$TREE/flash_attention_minitorch_amd/csrc"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS=(--offload-arch="${FA_ARCH:-gfx950}" -O3 -std=c++17 -fPIC -shared -Wno-unused-value -mllvm -amdgpu-mfma-vgpr-form=1 -fno-slp-vectorize ${FA_EXTRA_FLAGS:-})
cd "$OUT"
build() {   # library stem, extra flags...
  local lib=$1
  shift
  [ -n "${FA_ISA_NOBUILD:-}" ] && return 0
  "$HIPCC" "${FLAGS[@]}" "$@" -save-temps "$SRC/$lib.hip" -o "$OUT/$lib.so" 2> "$lib.res.txt" || { tail -n 60 "$lib.res.txt" >&2; exit 1; }
}
asm_of() { echo "$1-hip-amdgcn-amd-amdhsa-${FA_ARCH:-gfx950}.s"; }

case "$MODE" in
mix)
  build fa_api -Rpass-analysis=kernel-resource-usage
  S=$(asm_of fa_api)
  for K in "$@"; do
    echo "== $K"
    grep -A12 "Function Name: .*${K}" fa_api.res.txt | grep -E " VGPRs:|AGPRs|Scratch|Occupancy|LDS Size" | sed 's/\[-Rpass.*//; s/.*remark: [^ ]* //' | tr '\n' ' '; echo
    start=$(grep -n "^_ZN2fa.*${K}.*:" "$S" | head -1 | cut -d: -f1)
    awk -v s="$start" 'NR>=s' "$S" | awk '/^\.Lfunc_end/{exit} {print}' > "kern_$K.s"
    awk '/^\.LBB[0-9_]+:/{lbl=$1} {c[lbl]++; if($1 ~ /^v_mfma/) m[lbl]++; else if($1 ~ /^v_exp/) e[lbl]++; else if($1 ~ /^v_/) v[lbl]++; if($1 ~ /^ds_/) d[lbl]++; if ($1 ~ /^s_/) s[lbl]++; if ($1 ~ /^(global|buffer)_/) g[lbl]++} END{for(l in c) if (c[l]>'"${MINSZ:-30}"') print l, "total",c[l],"mfma",m[l]+0,"exp",e[l]+0,"valu",v[l]+0,"ds",d[l]+0,"salu",s[l]+0,"vmem",g[l]+0}' "kern_$K.s" | sort -t_ -k2 -n
  done
  ;;
split)
  for lib in fa_api fa_decode fa_window fa_varlen fa_bidir fa_prefix fa_local fa_lsink; do
    [ -f "$SRC/$lib.hip" ] || continue   # (a tree from before the window, the varlen, the bidir, the prefix, the local or the lsink library has no such .hip)
    build "$lib"
    rm -rf "kernels/$lib"
    mkdir -p "kernels/$lib"
    # (a mangled name can be longer than a file name may be: the file is named by the name's checksum then, the name is its first line)
    awk -v dir="kernels/$lib" '
      /^[A-Za-z_][A-Za-z0-9_$.]*:/ { name = $1; sub(/:.*/, "", name); buf = ""; inside = 1; kern = 0 }
      inside {
        line = $0
        gsub(/\.LBB[0-9]+_/, ".LBB_", line)
        gsub(/\.Lfunc_end[0-9]+/, ".Lfunc_end", line)
        sub(/[ \t]*;.*$/, "", line)
        if (line != "") buf = buf line "\n"
        if ($1 == ".amdhsa_kernel") kern = 1
      }
      /^\.Lfunc_end/ {
        if (inside && kern) {
          file = name
          if (length(file) > 200) { cmd = "printf %s \047" name "\047 | cksum"; cmd | getline sum; close(cmd); split(sum, p, " "); file = substr(name, 1, 180) "~" p[1] }
          printf "%s", buf > (dir "/" file ".s"); close(dir "/" file ".s"); n++
        }
        inside = 0
      }
      END { printf "%s: %d kernels\n", dir, n }' "$(asm_of "$lib")"
  done
  ;;
*)
  usage
  ;;
esac
