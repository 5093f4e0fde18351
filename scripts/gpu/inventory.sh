# Per-env-tick SQ counters of the headline stream for narrowed libshipsim variants (one rocprofv3 --pmc pass each):
#   bash scripts/gpu/inventory.sh TAG NAME...   (ast_sac_amd/lib/abl/NAME.so from scripts/build_variant.sh)
# WAITS=1: a second counters-only pass per variant with what the SQ block offers towards splitting the parked cycles
# by cause (the LDS issue-wait counter, the in-flight levels of the scalar / LDS / vector memory pipes and their
# instruction counts), summarized to inventory_waits_TAG.json. (A run of its own: eight more counters do not fit
# the first pass. What they do and do not tell: profiles/tick_waits.md.)
. "$(dirname "$0")/common.sh"
TAG=$1; shift
export TMPDIR=/tmp
cd /tmp
args=""; wargs=""
for n in "$@"; do
  SHIPSIM_LIB=$R/ast_sac_amd/lib/abl/$n.so timeout -s KILL 150 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_ACTIVE_INST_ANY \
    SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVES --output-format csv \
    -d "$O/inv_${TAG}_$n" -o run -- python3 "$R/scripts/tick_inventory.py" run "$O/inv_${TAG}_$n.json" \
    > "$O/inv_${TAG}_$n.log" 2>&1; hard $? "inventory $n"
  args="$args $O/inv_${TAG}_$n $O/inv_${TAG}_$n.json"
  if [ "${WAITS:-0}" = 1 ]; then
    SHIPSIM_LIB=$R/ast_sac_amd/lib/abl/$n.so timeout -s KILL 150 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_WAIT_INST_LDS \
      SQ_INST_LEVEL_SMEM SQ_INST_LEVEL_LDS SQ_INST_LEVEL_VMEM SQ_INSTS_SMEM SQ_INSTS_VMEM_RD SQ_WAVES --output-format csv \
      -d "$O/invw_${TAG}_$n" -o run -- python3 "$R/scripts/tick_inventory.py" run "$O/invw_${TAG}_$n.json" \
      > "$O/invw_${TAG}_$n.log" 2>&1; hard $? "inventory waits $n"
    wargs="$wargs $O/invw_${TAG}_$n $O/invw_${TAG}_$n.json"
  fi
done
cd "$R"
python scripts/tick_inventory.py summarize $args > "$O/inventory_$TAG.json"; hard $? summarize
cat "$O/inventory_$TAG.json"
if [ -n "$wargs" ]; then
  python scripts/tick_inventory.py summarize $wargs > "$O/inventory_waits_$TAG.json"; hard $? "summarize waits"
  cat "$O/inventory_waits_$TAG.json"
fi
find "$O" -name "*kernel_trace.csv" -delete
