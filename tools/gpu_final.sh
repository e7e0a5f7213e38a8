#!/bin/bash
# round-end rehearsal on the final tree: the driver's three GPU steps in its order
set -o pipefail
export OUT=${OUT:-bench_out}  # where this script and the ones it calls write
TAG=${1:-final}
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 600 python -u -m pytest tests -x -q -m gpu --timeout 300 --timeout-method thread > $OUT/${TAG}_pytest.txt 2>&1 || { tail -20 $OUT/${TAG}_pytest.txt; exit 1; }
tail -1 $OUT/${TAG}_pytest.txt
timeout -k 10 200 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.txt 2>&1 || { tail -20 $OUT/${TAG}_smoke.txt; exit 1; }
tail -1 $OUT/${TAG}_smoke.txt
timeout -k 10 400 python bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err || exit 1
cat $OUT/${TAG}_bench.json
