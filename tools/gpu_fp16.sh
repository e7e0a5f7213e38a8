#!/bin/bash
# fp16 (config 5) check: measured errors per module case + Dice, the fp16 parity tests, then the
# 192^3 full-model fp16 bench line.  Usage: tools/gpu_fp16.sh TAG
set -o pipefail
export OUT=${OUT:-bench_out}  # where this script and the ones it calls write
TAG=${1:-f16}
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 300 python -u tools/prec_errs.py fp16 > $OUT/${TAG}_errs.txt 2>&1
rc=$?; cat $OUT/${TAG}_errs.txt | grep -v amdgpu.ids; [ $rc -ne 0 ] && exit $rc
timeout -k 10 400 python -u -m pytest -x -q --timeout 300 --timeout-method thread tests/test_gpu_parity.py -k "fp16 or attention_vs_oracle or stage1_fused" > $OUT/${TAG}_pytest.txt 2>&1
rc=$?; tail -15 $OUT/${TAG}_pytest.txt; [ $rc -ne 0 ] && exit $rc
timeout -k 10 400 python -u bench.py --full --workload full --img 192 --precision fp16 --steps 10 --warmup 3 > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err || { tail -20 $OUT/${TAG}_bench.err; exit 1; }
cat $OUT/${TAG}_bench.json
