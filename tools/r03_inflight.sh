#!/bin/bash
# clips in flight sweep (resident frames), fast mode
OUT=${OUT:-$PWD/out}; mkdir -p "$OUT"          # where the results go (run from the repository root)
for m in "$@"; do
  python bench.py --full --inflight $m --steps 24 --warmup 4 --cpu-frames 0 --repeats 5 --no-pcie --no-vit --no-extras > $OUT/r03_if.json 2> $OUT/r03_if.err || exit 1
  python - <<PY
import json
d=json.load(open('$OUT/r03_if.json'))
print('inflight $m', 'fps', round(d['value']), 'ms/step', d['ms_per_step'])
PY
done
