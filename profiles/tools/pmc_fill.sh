#!/bin/bash
# Counter passes over the encode-only script (full bench volume) for the level loop's wide kernels: issue shares of
# k_fill16 / k_est_summ and their FETCH_SIZE / WRITE_SIZE, summed over the launches of one build and for the largest
# launch.  Counters only, each set in a run of its own.  usage: profiles/tools/pmc_fill.sh TAG  (output under $PMC_OUT, default build/pmc/)
set -o pipefail
TAG=${1:-f}
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
OUT=${PMC_OUT:-$ROOT/build/pmc}
mkdir -p "$OUT"
i=0
for set in "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY" "SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_VMEM SQ_ACTIVE_INST_SCA SQ_WAVES" "SQ_INSTS_VALU SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_SALU" "FETCH_SIZE" "WRITE_SIZE"; do
  i=$((i+1))
  ENC_REPS=1 timeout -k 10 240 rocprofv3 --pmc $set --output-format csv -d "$OUT/pmcf_${TAG}_$i" -- python3 "$ROOT/profiles/tools/enc_time.py" > "$OUT/pmcf_${TAG}_$i.log" 2>&1
  rc=$?
  tail -1 "$OUT/pmcf_${TAG}_$i.log"
  if [ $rc -ne 0 ]; then echo "pass $i failed ($rc): stopping"; exit $rc; fi
done
python3 "$ROOT/profiles/tools/pmc_fill_parse.py" "$OUT" "$TAG" | tee "$OUT/pmcf_${TAG}.txt"
