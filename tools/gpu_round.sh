#!/bin/bash
# One GPU round trip: the GPU test suite, then the default bench (+ stages).
# usage: tools/gpu_round.sh TAG
set -o pipefail
tag=${1:-x}
cd "$GRAFT_REPO_ROOT" || exit 1
OUT=${OUT:-bench_out}; mkdir -p $OUT
timeout -k 10 400 python3 -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread \
  > $OUT/gt_$tag.log 2>&1 || { tail -30 $OUT/gt_$tag.log; exit 1; }
tail -2 $OUT/gt_$tag.log
timeout -k 10 240 python3 bench.py --full --no-cpu --stages > $OUT/b_$tag.json 2> $OUT/b_$tag.err || { cat $OUT/b_$tag.err | tail; exit 1; }
cat $OUT/b_$tag.json $OUT/b_$tag.err
