#!/bin/bash
# config-3 GPU check: sliding-window parity tests, the encoder bench (driver line), the
# sliding-window bench, and a kernel trace of the encoder bench.
set -o pipefail
export OUT=${OUT:-bench_out}  # where this script and the ones it calls write
TAG=${1:-sw1}
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 300 python -u -m pytest tests/test_gpu_sliding_window.py -x -v --timeout 120 \
  --timeout-method thread -m gpu > $OUT/${TAG}_pytest.txt 2>&1 || { tail -30 $OUT/${TAG}_pytest.txt; exit 1; }
tail -3 $OUT/${TAG}_pytest.txt
timeout -k 10 400 python bench.py --full --steps 20 --warmup 5 > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err || { tail -20 $OUT/${TAG}_bench.err; exit 1; }
cat $OUT/${TAG}_bench.json
timeout -k 10 400 python bench.py --full --workload sliding --steps 3 --warmup 1 > $OUT/${TAG}_sliding.json 2> $OUT/${TAG}_sliding.err || { tail -20 $OUT/${TAG}_sliding.err; exit 1; }
cat $OUT/${TAG}_sliding.json
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_prof -o run -- python bench.py --full --steps 5 --warmup 2 --cpu-baseline 0 --parity 0 > $OUT/${TAG}_prof.log 2>&1 || { tail -20 $OUT/${TAG}_prof.log; exit 1; }
echo done
