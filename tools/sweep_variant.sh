#!/bin/bash
cd $GRAFT_REPO_ROOT
R=$PWD; OUT=${OUT:-$R/out}; mkdir -p "$OUT"          # where the results go
for v in $*; do
  (cd /tmp && TMPDIR=/tmp AVD_UV_VARIANT=$v timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/var_$v -- python3 $R/bench.py --full --steps 5 --warmup 2 --cpu-frames 0 > $OUT/var_$v.log 2>&1) || exit 1
  echo variant=$v done
done
