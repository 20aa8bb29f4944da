#!/bin/bash
# Run on an MI355X machine: kernel statistics of the full bench command (bench.py --full) and of the serial one, and the
# two HBM-traffic PMC passes (separate --pmc runs, no tracing combined with counters).
# profiles/make_profiles.py then turns what gets merged into gpurun_out/ into the committed r03_* files.
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd /tmp && export TMPDIR=/tmp
R=/root/repo/gpurun_out
rm -rf $R/r3_stats $R/r3_stats_serial $R/r3_fetch $R/r3_write
rocprofv3 --kernel-trace --stats --output-format csv -d $R/r3_stats -- python3 "$ROOT/bench.py" --full --no-cpu --no-stream > $R/r3_stats.log 2>&1 || echo "stats pass failed"
rm -f $R/r3_stats/*/*kernel_trace.csv
rocprofv3 --kernel-trace --stats --output-format csv -d $R/r3_stats_serial -- python3 "$ROOT/bench.py" --full --pipeline 1 --level-loop-streams 1 --no-cpu --no-stream > $R/r3_stats_serial.log 2>&1 || echo "serial stats pass failed"
rm -f $R/r3_stats_serial/*/*kernel_trace.csv
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $R/r3_fetch -- python3 "$ROOT/bench.py" --full --steps 1 --warmup 0 --level-loop-streams 1 --no-cpu --no-render --no-stream > $R/r3_fetch.log 2>&1 || echo "fetch pass failed"
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $R/r3_write -- python3 "$ROOT/bench.py" --full --steps 1 --warmup 0 --level-loop-streams 1 --no-cpu --no-render --no-stream > $R/r3_write.log 2>&1 || echo "write pass failed"
tail -1 $R/r3_stats.log | cut -c1-600
