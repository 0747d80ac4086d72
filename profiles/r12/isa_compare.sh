#!/bin/sh
# The listing comparison of profiles/r12/README.md: k_dsc, k_navtex and k_same of a parent checkout against this tree's.
#   sh profiles/r12/isa_compare.sh PARENT_CHECKOUT [OUT_DIR]
# Compiles each bank's file with the Makefile's flags plus --cuda-device-only -S, drops directive and comment lines, puts
# fixed tokens for the kernel symbols, the .LBB numbers and the __hip_cuid_* label, and diffs.  Prints the metadata figures
# and the number of differing lines per kernel.
set -e
parent=$1
out=${2:-/tmp/isa_compare}
here=$(cd "$(dirname "$0")/../.." && pwd)
mkdir -p "$out"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
flags="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function --cuda-device-only -S"
for k in dsc navtex same; do
  for side in parent tree; do
    root=$parent
    [ $side = tree ] && root=$here
    $HIPCC $flags -I"$root/include" "$root/ka9q_sdr_amd/csrc/kq_$k.hip" -o "$out/$k.$side.s"
    sym=$(grep -oE '^_Z[A-Za-z0-9_]+:' "$out/$k.$side.s" | head -1 | tr -d :)
    grep -vE '^([[:space:]]+\.|[[:space:]]*;|[[:space:]]*$)' "$out/$k.$side.s" |  # (labels, .LBB at column 0, stay)
      sed -E "s/$sym/KERNEL/g; s/\.LBB[0-9]+_/.LBB_/g; s/__hip_cuid_[0-9a-f]+/CUID/g; s/[[:space:]]*;.*$//" > "$out/$k.$side.txt"
    printf '%s %s: %s lines,' k_$k $side "$(wc -l < "$out/$k.$side.txt")"
    grep -E '^[[:space:]]*\.(vgpr_count|sgpr_count|group_segment_fixed_size|private_segment_fixed_size):' "$out/$k.$side.s" | tr -s ' \n' ' '
    echo
  done
  if diff "$out/$k.parent.txt" "$out/$k.tree.txt" > "$out/$k.diff"; then
    echo "k_$k: listings equal"
  else
    echo "k_$k: $(grep -c '^[<>]' "$out/$k.diff") differing lines"
  fi
done
