#!/bin/bash
# gpu_round.sh TAG plus the bench at the 8-GPU per-rank shard (8,192 proofs) on one GPU.
set -o pipefail
TAG=${1:-run}
bash tools/gpu_round.sh $TAG || exit 1
O=$(dirname "$(ls -d */$TAG/bench.json | head -1)")   # the folder gpu_round.sh wrote TAG's results to
timeout -k 10 120 python -u bench.py --full --no-cpu --no-configs --n 8192 > $O/bench_8192.json 2> $O/bench_8192.err || { echo "bench 8192 failed"; exit 1; }
cat $O/bench_8192.json
