#!/bin/bash
# PMC passes over a short bench run (one counter group per pass, --kernel-trace only beside --pmc).
# Usage: bash scripts/pmc.sh [workload]   -> $KGE_PMC_OUT/<workload>/<pass>/...counter_collection.csv
# (KGE_PMC_OUT: where the passes are written, pmc_out/ in the tree by default; scripts/pmc_summary.py takes
# the <workload> directory as its first argument)
set -u
R=${GRAFT_REPO_ROOT:-$(pwd)}
W=${1:-c2}
OUT=${KGE_PMC_OUT:-$R/pmc_out}/$W
export TMPDIR=/tmp
mkdir -p "$OUT"
i=0
for CTRS in "FETCH_SIZE" "WRITE_SIZE" "TCC_HIT_sum TCC_MISS_sum" "TCC_EA0_RDREQ_sum TCC_EA0_RDREQ_32B_sum" \
            "SQ_WAVES SQ_INSTS_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU" \
            "GRBM_GUI_ACTIVE GRBM_COUNT"; do
  i=$((i+1))
  echo "== pass $i: $CTRS"
  # --full: the train step's kernels (--train-steps 5) are counted beside the scoring step's
  timeout -k 10 300 rocprofv3 --pmc $CTRS --kernel-trace --output-format csv -d "$OUT/p$i" -o run -- \
      python3 "$R/bench.py" --full --steps 10 --warmup 2 --no-cpu-baseline --sharded-steps 0 --train-steps 5 --workload "$W" > "$OUT/p$i.log" 2>&1
  rc=$?
  echo "rc=$rc"
  if [ $rc -ge 124 ]; then echo "fatal rc=$rc: stopping"; exit $rc; fi
done
echo done
