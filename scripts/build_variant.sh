#!/bin/bash
# A narrowed libshipsim (the headline stream kernels only, -DSHIPSIM_REGCHECK=1: run_table / run_policy at LPE 16,
# detailed machinery) with the product's flags plus extra ones, for timing A/Bs through SHIPSIM_LIB (bench.py
# --no-c2 --no-policy-stream --sac-steps 0 runs on it).
#   bash scripts/build_variant.sh NAME [extra hipcc flags]  ->  ast_sac_amd/lib/abl/NAME.so
# SRC=<dir with the library's .hip files> builds another copy of the sources (default: the tree's; a copy from before
# the C2 kernel had a file of its own holds shipsim_kernels.hip alone).
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
NAME=$1; shift
SRC=${SRC:-$R/ast_sac_amd/csrc}
mkdir -p "$R/ast_sac_amd/lib/abl"
# object 1's flags and every .hip file of the library on one line (ast_sac_amd/build_hash.py)
F="$(cd "$R" && python3 -c 'from ast_sac_amd.build_hash import HIPFLAGS, lib_flag_sets; print(" ".join(HIPFLAGS + lib_flag_sets("shipsim")[0]))')"
S=$(for f in $(cd "$R" && python3 -c 'from ast_sac_amd.build_hash import OBJECTS; print(" ".join(s for s, _ in OBJECTS["shipsim"]))'); do [ -f "$SRC/$(basename $f)" ] && echo "$SRC/$(basename $f)"; done)
/opt/rocm/bin/hipcc $F -I"$R/include" -I"$SRC" -I"$R/ast_sac_amd/csrc" -DSHIPSIM_REGCHECK=1 -DSHIPSIM_SRC_HASH="\"variant-$NAME\"" "$@" \
  $S -o "$R/ast_sac_amd/lib/abl/$NAME.so"
