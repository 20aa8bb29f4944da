#!/bin/bash
# Counter passes over the encode-only script (full bench volume) for k_prune_emit12 and the kernels behind it on the
# stream: wave-cycles and the share of them spent waiting, VALU issue time, instruction counts by kind.  Counters only,
# each set in a run of its own.  usage: profiles/tools/pmc_prune.sh TAG  (output under $PMC_OUT, default build/pmc/)
set -o pipefail
TAG=${1:-p}
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
OUT=${PMC_OUT:-$ROOT/build/pmc}
mkdir -p "$OUT"
export PYTHONPATH="$ROOT${PYTHONPATH:+:$PYTHONPATH}"
i=0
for set in "SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_VALU SQ_BUSY_CYCLES" "SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_SALU SQ_WAVES" "GRBM_GUI_ACTIVE SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS SQ_ACTIVE_INST_SCA"; do
  i=$((i+1))
  timeout -k 10 240 rocprofv3 --pmc $set --output-format csv -d "$OUT/pmcp_${TAG}_$i" -- python3 "$ROOT/profiles/tools/enc_time.py" > "$OUT/pmcp_${TAG}_$i.log" 2>&1
  rc=$?
  tail -1 "$OUT/pmcp_${TAG}_$i.log"
  if [ $rc -ne 0 ]; then echo "pass $i failed ($rc): stopping"; exit $rc; fi
done
python3 - "$OUT" "$TAG" <<'PY' | tee "$OUT/pmcp_${TAG}.txt"
import csv, glob, sys, collections
out, tag = sys.argv[1], sys.argv[2]
agg = collections.defaultdict(lambda: collections.defaultdict(list))
for f in glob.glob('%s/pmcp_%s_*/*/*counter_collection.csv' % (out, tag)):
    for r in csv.DictReader(open(f)):
        nm = r['Kernel_Name'].split('(')[0].replace('void ', '').replace('vr::', '')
        if nm.startswith(('k_prune_emit12', 'k_index12', 'k_concat12')):
            agg[nm][r['Counter_Name']].append(float(r['Counter_Value']))
for k, d in sorted(agg.items()):
    print('==', k)
    for c, v in sorted(d.items()):
        print('  %-22s launches %d  mean %.5g' % (c, len(v), sum(v) / len(v)))
    if 'SQ_WAVE_CYCLES' in d and 'SQ_WAIT_INST_ANY' in d:
        print('  waiting share of wave-cycles  %.3f' % (sum(d['SQ_WAIT_INST_ANY']) / sum(d['SQ_WAVE_CYCLES'])))
    if 'SQ_ACTIVE_INST_VALU' in d and 'SQ_BUSY_CYCLES' in d:
        print('  SQ_ACTIVE_INST_VALU / SQ_BUSY_CYCLES  %.3f' % (sum(d['SQ_ACTIVE_INST_VALU']) / sum(d['SQ_BUSY_CYCLES'])))
PY
