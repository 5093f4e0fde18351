#!/bin/bash
# A whole libshipsim (both objects, the product's flags) from the kernel sources of another git revision, with this
# tree's include/ (the C ABI header), for env timing A/Bs through SHIPSIM_LIB (scripts/gpu/env_abn.sh).
#   bash scripts/build_shipsim_at.sh NAME [GITREF=HEAD]  ->  ast_sac_amd/lib/abl/NAME.so
# EXTRA="flags" adds hipcc flags to every object; STRATEGY=name replaces the machine scheduler strategy.
# The file list, the objects and their flags are the revision's own (its ast_sac_amd/build_hash.py).
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
NAME=$1; REF=${2:-HEAD}
D=$(mktemp -d /tmp/shipsim_src.XXXX)
git -C "$R" show "$REF:ast_sac_amd/build_hash.py" > "$D/build_hash.py"
# "F <file>" per source file, "O <source> <flags>" per object (a revision whose objects are flag sets alone compiles
# shipsim_kernels.hip once per set)
LIST=$(cd "$D" && python3 -c 'import build_hash as b; K = "ast_sac_amd/csrc/shipsim_kernels.hip"; base = [f for f in b.HIPFLAGS if f != "-shared"] + b.LIB_FLAGS["shipsim"]; [print("F", f) for f in b.SOURCES["shipsim"]]; [print("O", *([o[0]] + base + o[1] if isinstance(o, tuple) else [K] + base + o)) for o in b.OBJECTS["shipsim"]]')
for f in $(echo "$LIST" | awk '$1 == "F" && $2 ~ /csrc\// {print $2}'); do
  git -C "$R" show "$REF:$f" > "$D/$(basename "$f")"
done
OUT=$R/ast_sac_amd/lib/abl/$NAME.so
mkdir -p "$R/ast_sac_amd/lib/abl"
OBJS=()
i=0
while read -r _ SRC SET; do
  if [ -n "${STRATEGY:-}" ]; then SET=${SET//amdgpu-sched-strategy=max-ilp/amdgpu-sched-strategy=$STRATEGY}; fi
  /opt/rocm/bin/hipcc $SET ${EXTRA:-} -I"$D" -I"$R/include" -DSHIPSIM_SRC_HASH="\"variant-$NAME\"" -c "$D/$(basename "$SRC")" \
    -o "$OUT.$i.o" &
  OBJS+=("$OUT.$i.o")
  i=$((i + 1))
done < <(echo "$LIST" | grep '^O ')
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC "${OBJS[@]}" -o "$OUT"
rm -f "${OBJS[@]}"
rm -rf "$D"
echo "built $OUT"
