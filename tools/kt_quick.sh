#!/bin/bash
# quick per-kernel stats of one clip at a time (rocprofv3 --kernel-trace --stats)
R=$GRAFT_REPO_ROOT
OUT=${OUT:-$R/out}; mkdir -p "$OUT"          # where the results go
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/ktq
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/ktq -- python3 $R/bench.py --full --inflight 1 --steps 5 --warmup 2 --cpu-frames 0 --repeats 1 --no-pcie --no-vit > $OUT/ktq.log 2>&1 || exit 1
cd $R
find $OUT/ktq -name "*kernel_stats.csv" | head -1 | xargs -I{} python tools/kstats.py {} 7 24
