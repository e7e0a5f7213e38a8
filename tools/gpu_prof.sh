#!/bin/bash
# Kernel trace of the default bench step: warm-up + graph replays only (no op-timer repeats).
# Usage: tools/gpu_prof.sh TAG [extra bench args]
set -o pipefail
export OUT=${OUT:-bench_out}  # where this script and the ones it calls write
TAG=${1:-prof}
shift
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_prof -o run -- python -u bench.py --steps 10 --warmup 2 --cpu-baseline 0 --parity 0 --op-timers 0 "$@" > $OUT/${TAG}_prof.log 2>&1 || { tail -30 $OUT/${TAG}_prof.log; exit 1; }
tail -1 $OUT/${TAG}_prof.log | cut -c1-200
f=$(ls $OUT/${TAG}_prof/*kernel_trace.csv | head -1)
python tools/kstats.py "$f" ${NK:-30} > $OUT/${TAG}_kstats.txt
cat $OUT/${TAG}_kstats.txt
