#!/bin/bash
# LDS bank conflicts and MFMA busy cycles of the patch-embed GEMM (separate --pmc pass, no tracing domains)
R=$GRAFT_REPO_ROOT
OUT=${OUT:-$R/out}; mkdir -p "$OUT"          # where the results go
cd /tmp && export TMPDIR=/tmp
rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_VALU_MFMA_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY --output-format csv -d $OUT/gemm_pmc -- python3 $R/bench.py --full --cpu-frames 0 --repeats 1 --no-pcie --steps 2 --warmup 1 > $OUT/gemm_pmc.log 2>&1
cd $R
python tools/pmc_summary.py k_gemm $OUT/gemm_pmc/*/*counter_collection.csv
