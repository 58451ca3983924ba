#!/bin/bash
# L1 (TCP) -> L2 read requests and L1 accesses of the level kernels (separate --pmc pass, no tracing domains)
R=$GRAFT_REPO_ROOT
OUT=${OUT:-$R/out}; mkdir -p "$OUT"          # where the results go
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/tcp_pmc
rocprofv3 --pmc TCP_TCC_READ_REQ_sum TCP_TOTAL_CACHE_ACCESSES_sum TCP_TCC_WRITE_REQ_sum --output-format csv -d $OUT/tcp_pmc -- python3 $R/bench.py --full --inflight 1 --steps 2 --warmup 1 --cpu-frames 0 --repeats 1 --no-pcie --no-vit > $OUT/tcp_pmc.log 2>&1 || { tail -5 $OUT/tcp_pmc.log; exit 1; }
cd $R
python tools/pmc_summary.py k_fb_level $OUT/tcp_pmc/*/*counter_collection.csv
python tools/pmc_summary.py k_polyexp $OUT/tcp_pmc/*/*counter_collection.csv
