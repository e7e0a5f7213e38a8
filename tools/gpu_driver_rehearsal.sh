#!/bin/bash
# What the driver runs at round end: smoke(), then the default bench (N=1, no flags).
set -o pipefail
export OUT=${OUT:-bench_out}  # where this script and the ones it calls write
TAG=${1:-dr}
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 300 python -u -c 'import __graft_entry__ as g; g.smoke()' > $OUT/${TAG}_smoke.txt 2>&1 || { tail -20 $OUT/${TAG}_smoke.txt; exit 1; }
tail -1 $OUT/${TAG}_smoke.txt
start=$(date +%s)
timeout -k 10 600 python -u bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err || { tail -20 $OUT/${TAG}_bench.err; exit 1; }
echo "bench wall $(( $(date +%s) - start )) s"
python tools/bench_line.py $OUT/${TAG}_bench.json
