#!/bin/bash
# Round-4 GPU round trip: new tests, smoke, the GPU suite, the default bench.
# usage: tools/gpu_r04.sh TAG [pytest -k expr for the first leg]
set -o pipefail
tag=${1:-x}
cd "$GRAFT_REPO_ROOT" || exit 1
OUT=${OUT:-bench_out}; mkdir -p $OUT
if [ -n "$2" ]; then
  timeout -k 10 300 python3 -u -m pytest tests -m gpu -x -v --timeout 200 --timeout-method thread -k "$2" \
    > $OUT/new_$tag.log 2>&1 || { tail -40 $OUT/new_$tag.log; exit 1; }
  tail -3 $OUT/new_$tag.log
fi
timeout -k 10 300 python3 -u -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_$tag.log 2>&1 \
  || { tail -30 $OUT/smoke_$tag.log; exit 1; }
cat $OUT/smoke_$tag.log
timeout -k 10 600 python3 -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread \
  > $OUT/gt_$tag.log 2>&1 || { tail -30 $OUT/gt_$tag.log; exit 1; }
tail -2 $OUT/gt_$tag.log
timeout -k 10 300 python3 bench.py --full --no-cpu --stages > $OUT/b_$tag.json 2> $OUT/b_$tag.err \
  || { tail -20 $OUT/b_$tag.err; exit 1; }
cat $OUT/b_$tag.json; tail -40 $OUT/b_$tag.err
