# Ablation builds (timing diagnostics only; results intentionally differ). Output: ast_sac_amd/lib/abl/*.so
set -e
cd "$(dirname "$0")/.."
mkdir -p ast_sac_amd/lib/abl
# the product's code-generation flags (ast_sac_amd/build_hash.py), so the builds differ only by the ablation
# (object 1's flags, and every .hip file of the library on the one line)
F="$(python3 -c 'from ast_sac_amd.build_hash import HIPFLAGS, lib_flag_sets; print(" ".join(HIPFLAGS + lib_flag_sets("shipsim")[0]))') -Iinclude -Iast_sac_amd/csrc"
S="$(python3 -c 'from ast_sac_amd.build_hash import OBJECTS; print(" ".join(s for s, _ in OBJECTS["shipsim"]))')"
for v in NO_MAPDIST NO_GROUND NO_WIND; do
  /opt/rocm/bin/hipcc $F -DSHIPSIM_ABL_$v $S -o ast_sac_amd/lib/abl/lib_$v.so &
done
/opt/rocm/bin/hipcc $F -DSHIPSIM_ABL_NO_MAPDIST -DSHIPSIM_ABL_NO_GROUND -DSHIPSIM_ABL_NO_WIND $S -o ast_sac_amd/lib/abl/lib_ALL3.so &
wait
