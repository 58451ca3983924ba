#!/bin/bash
# diagnostic PMC passes (separate runs, no tracing domains, small sets) over the bench workload
R=$GRAFT_REPO_ROOT
OUT=${OUT:-$R/out}; mkdir -p "$OUT"          # where the results go
cd /tmp && export TMPDIR=/tmp
i=0
while read -r set; do
  i=$((i+1))
  timeout -k 10 100 rocprofv3 --pmc $set --output-format csv -d $OUT/diag_$i -- python3 $R/bench.py --full --steps 2 --warmup 1 --cpu-frames 0 > $OUT/diag_$i.log 2>&1
  echo "pass $i rc=$? : $set" | tee -a $OUT/diag_progress.txt
done
