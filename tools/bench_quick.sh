#!/bin/bash
# Quick A/B on a GPU box: the --full bench line without the CPU baseline and the train_ppo leg,
# reduced to (env-steps/s, ms/iteration) and the per-call times of the C-ABI entry points.
#   [BENCH_OUT=dir] tools/bench_quick.sh <tag> [ENV=value ...]   ->  dir/<tag>.json (bench_out/)
set -eo pipefail
tag=${1:-q}; shift || true
for kv in "$@"; do export "$kv"; done
out=${BENCH_OUT:-bench_out}
mkdir -p "$out"
python3 bench.py --full --no-cpu-baseline --no-train-ppo > "$out/$tag.json" 2> "$out/$tag.err"
python3 - "$tag" "$out/$tag.json" <<'P'
import json, sys
d = json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
print(sys.argv[1], round(d["value"] / 1e6, 2), "M env-steps/s", d["ms_per_step"], "ms/iter")
ks = d.get("kernels_ms_per_iter") or {}
for k, v in sorted(((k, v) for k, v in ks.items() if isinstance(v, dict)), key=lambda kv: -kv[1]["ms"])[:9]:
    print(f"  {k:42s} {v['calls']:4d} x {1e3 * v['ms'] / v['calls']:7.2f} us = {v['ms']:.4f} ms")
P
