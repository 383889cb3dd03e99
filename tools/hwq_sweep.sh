set -o pipefail
cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-bench_out}; mkdir -p $OUT
for cfg in "24 16" "24 20" "32 24" "32 32" "24 16"; do
  set -- $cfg
  timeout -k 10 200 python3 bench.py --full --no-cpu --probe 0 --steps 6 --hw-queues $1 --streams $2 > $OUT/hwq.json 2>&1 || exit 1
  python3 -c "import json; d=json.loads(open('$OUT/hwq.json').read().strip().splitlines()[-1]); print('hwq $1 streams $2', d['value'])"
done
