#!/bin/bash
# final per-round evidence: kernel trace stats (clips run alone = the durations bench.py's roofline uses; and the
# default serving mode with 3 clips in flight), PMC passes (separate, no tracing domains), bench line
R=$GRAFT_REPO_ROOT
OUT=${OUT:-$R/out}; mkdir -p "$OUT"          # where the results go
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/final_kt1 -- python3 $R/bench.py --full --inflight 1 --steps 5 --warmup 2 --cpu-frames 0 > $OUT/final_kt1.log 2>&1 || exit 1
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/final_kt -- python3 $R/bench.py --full --steps 5 --warmup 2 --cpu-frames 0 > $OUT/final_kt.log 2>&1 || exit 1
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/final_pmc_fetch -- python3 $R/bench.py --full --inflight 1 --steps 2 --warmup 1 --cpu-frames 0 > $OUT/final_pmc_fetch.log 2>&1 || exit 1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/final_pmc_write -- python3 $R/bench.py --full --inflight 1 --steps 2 --warmup 1 --cpu-frames 0 > $OUT/final_pmc_write.log 2>&1 || exit 1
cd $R && python bench.py --full --pcie > $OUT/final_bench.json 2> $OUT/final_bench.err || exit 1
python bench.py --full --inflight 1 --cpu-frames 0 > $OUT/final_bench_inflight1.json 2>> $OUT/final_bench.err || exit 1
head -c 250 $OUT/final_bench.json
