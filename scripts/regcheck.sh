# Register usage / spills of a narrowed build (the whole-library report: python scripts/register_report.py).
#   bash scripts/regcheck.sh [N] [extra hipcc flags]   libshipsim with -DSHIPSIM_REGCHECK=N (one kernel set):
#     N = 1 (default): the headline stream kernels (chained, LPE 16, detailed; sbmpc and none)
#     N = 2: the LPE-8 stream kernels (the C4 shard's collector: policy and table streams)
#     N = 3: the multi-obstacle (K > 1) kernels: steps, table streams and policy streams (collav none and sbmpc)
#   bash scripts/regcheck.sh sac H [extra hipcc flags]   libsacfused's kernels of hidden width H only
set -e
cd "$(dirname "$0")/.."
N=${1:-1}; shift || true
FLAGS="-O3 --offload-arch=gfx950 -ffp-contract=off -fPIC -shared -std=c++17 -Iinclude -Iast_sac_amd/csrc"
if [ "$N" = sac ]; then
  H=${1:-256}; shift || true
  /opt/rocm/bin/hipcc $FLAGS -DSACF_REGCHECK_H=$H -Rpass-analysis=kernel-resource-usage "$@" \
    ast_sac_amd/csrc/sac_kernels.hip -o /tmp/regcheck_sac.so 2> /tmp/regcheck_sac.txt
  python3 scripts/regsummary.py /tmp/regcheck_sac.txt
  exit 0
fi
# object 1's flag set and every .hip file of the library (ast_sac_amd/build_hash.py)
LF="$(python3 -c 'from ast_sac_amd.build_hash import lib_flag_sets; print(" ".join(lib_flag_sets("shipsim")[0]))')"
S="$(python3 -c 'from ast_sac_amd.build_hash import OBJECTS; print(" ".join(s for s, _ in OBJECTS["shipsim"]))')"
/opt/rocm/bin/hipcc $FLAGS $LF -DSHIPSIM_REGCHECK=$N -Rpass-analysis=kernel-resource-usage "$@" \
  $S -o /tmp/regcheck.so 2> /tmp/regcheck.txt
python3 scripts/regsummary.py /tmp/regcheck.txt | grep -E "ast_step|sbmpc_eval|legacy"
