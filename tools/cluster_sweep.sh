#!/usr/bin/env bash
# bench.py at a series of two-level cluster targets: LM it/s, PCG iterations and the CG phase per target.
#   usage: tools/cluster_sweep.sh [log_dir]
cd "$(dirname "$0")/.."
LOGS=${1:-$(mktemp -d)}
for K in 16 12 14 20 16 12 14; do
  timeout -k 10 100 python bench.py --full --no-cpu --no-solve --cluster-size $K > "$LOGS/k_$K.log" 2>&1 || exit 1
  echo "K=$K $(grep -o '"value": [0-9.]*' "$LOGS/k_$K.log" | head -1) $(grep -o '"pcg_iters": \[[^]]*\]' "$LOGS/k_$K.log") $(grep -o '"cg_iterations": [0-9.]*' "$LOGS/k_$K.log")"
done
