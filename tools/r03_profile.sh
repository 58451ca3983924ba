#!/bin/bash
# round-3 evidence in one gpurun call: kernel-trace stats (fast mode: clips alone / default 3 in flight; exact mode alone),
# PMC passes (separate, no tracing domains, program directly after --), bench lines.  Results under $OUT/r03_*;
# summaries are copied to profiles/ by hand.
R=$GRAFT_REPO_ROOT
OUT=${OUT:-$R/out}; mkdir -p "$OUT"          # where the results go
cd /tmp && export TMPDIR=/tmp
B="--full --steps 5 --warmup 2 --cpu-frames 0 --repeats 1 --no-pcie --no-vit --no-extras"
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/r03_kt1 -- python3 $R/bench.py --inflight 1 $B > $OUT/r03_kt1.log 2>&1 || exit 1
echo kt1 done
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/r03_kt3 -- python3 $R/bench.py $B > $OUT/r03_kt3.log 2>&1 || exit 1
echo kt3 done
export AVD_FB_MODE=exact
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/r03_kt1_exact -- python3 $R/bench.py --inflight 1 $B > $OUT/r03_kt1_exact.log 2>&1 || exit 1
unset AVD_FB_MODE
echo kt1 exact done
P="--full --inflight 1 --steps 2 --warmup 1 --cpu-frames 0 --repeats 1 --no-pcie --no-vit --no-extras"
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/r03_pmc_fetch -- python3 $R/bench.py $P > $OUT/r03_pmc_fetch.log 2>&1 || exit 1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/r03_pmc_write -- python3 $R/bench.py $P > $OUT/r03_pmc_write.log 2>&1 || exit 1
rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_VALU --output-format csv -d $OUT/r03_pmc_sq -- python3 $R/bench.py $P > $OUT/r03_pmc_sq.log 2>&1 || echo "sq pass failed"
rocprofv3 --pmc TA_BUSY_avr TA_BUSY_max TCP_TOTAL_CACHE_ACCESSES_sum TCP_TCC_READ_REQ_sum --output-format csv -d $OUT/r03_pmc_ta -- python3 $R/bench.py $P > $OUT/r03_pmc_ta.log 2>&1 || echo "ta pass failed"
rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum TCC_REQ_sum --output-format csv -d $OUT/r03_pmc_tcc -- python3 $R/bench.py $P > $OUT/r03_pmc_tcc.log 2>&1 || echo "tcc pass failed"
echo pmc done
cd $R
python tools/pmc_to_json.py $OUT/r03_pmc.json "round 3 (fb_mode fast)" $OUT/r03_pmc_fetch $OUT/r03_pmc_write $OUT/r03_pmc_sq $OUT/r03_pmc_ta $OUT/r03_pmc_tcc > $OUT/r03_pmc_summary.txt
mkdir -p profiles && cp $OUT/r03_pmc.json profiles/r03_pmc.json     # bench.py reads the traffic figures from here
python bench.py --full > $OUT/r03_bench.json 2> $OUT/r03_bench.err || exit 1
python bench.py --full --inflight 1 --cpu-frames 0 --no-extras > $OUT/r03_bench_inflight1.json 2>> $OUT/r03_bench.err || exit 1
head -c 600 $OUT/r03_bench.json; echo
for t in kt1 kt3 kt1_exact; do echo "== $t"; find $OUT/r03_$t -name "*kernel_stats.csv" | head -1 | xargs -I{} python tools/kstats.py {} 7 16; done
