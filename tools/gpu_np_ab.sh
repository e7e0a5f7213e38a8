#!/bin/bash
# per-op determinism + short bench for library variants (abso/libwf_<v>.so)
set -o pipefail
export OUT=${OUT:-bench_out}  # where this script and the ones it calls write
mkdir -p $OUT
for v in "$@"; do
  export WAVEFORMER_HIP_LIB=$PWD/abso/libwf_$v.so
  timeout -k 10 300 python -u tools/op_determinism.py > $OUT/opdet_$v.txt 2>&1 || { echo "opdet $v rc=$?"; tail -5 $OUT/opdet_$v.txt; exit 1; }
  grep SUMMARY $OUT/opdet_$v.txt
  timeout -k 10 200 python -u bench.py --full --steps 100 --warmup 5 --parity 0 --cpu-baseline 0 > $OUT/bench_$v.json 2> $OUT/bench_$v.err || { echo "bench $v rc=$?"; tail -5 $OUT/bench_$v.err; exit 1; }
  python -c "import json,sys; d=json.load(open('$OUT/bench_$v.json')); print('$v', round(d['value'],1), 'vol/s', {k: v['avg_launch_us'] for k, v in d.get('rooflines', {}).items()}, d['roofline']['avg_launch_us'])"
done
