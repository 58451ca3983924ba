#!/bin/bash
# A/B of AVD_FB_VARIANT values in one box: one clip at a time, resident; prints latency + stage times per variant
OUT=${OUT:-$PWD/out}; mkdir -p "$OUT"          # where the results go (run from the repository root)
for v in "$@"; do
  AVD_FB_VARIANT=$v python bench.py --full --inflight 1 --steps 10 --warmup 3 --cpu-frames 0 --repeats 3 --no-pcie --no-vit --no-extras > $OUT/r03_ab_$v.json 2> $OUT/r03_ab_$v.err || exit 1
  python - <<PY
import json
d=json.load(open('$OUT/r03_ab_$v.json'))
print('variant $v', 'fps', round(d['value']), 'ms/step', d['ms_per_step'], 'stages', {k: v for k, v in d['stages_ms'].items() if k != 'note'})
PY
done
