# PMC passes (one counter group per run, --kernel-trace only: the pool refuses pmc + sys traces) + a kernel-stats run of the same command
mkdir -p ${OUT:=out}; OUT=$(cd $OUT && pwd); export OUT   # where the summaries go (default out/)
R=$PWD; cd /tmp && export TMPDIR=/tmp
for c in FETCH_SIZE WRITE_SIZE "SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE" "TCC_HIT_sum TCC_MISS_sum"; do
  tag=$(echo $c | tr ' ' '_' | cut -c1-24)
  timeout 600 rocprofv3 --kernel-trace --pmc $c -d $OUT/pmc_$tag -o pmc -- python $R/bench.py --steps 5 --warmup 2 --full --no-cpu-baseline --no-train --no-clocks > $OUT/pmc_$tag.log 2>&1; echo "exit $?" >> $OUT/pmc_$tag.log
done
timeout 600 rocprofv3 --kernel-trace --stats -d $OUT/pmc_stats -o bench -- python $R/bench.py --steps 5 --warmup 2 --full --no-cpu-baseline --no-train --no-clocks > $OUT/rocprof_stats.log 2>&1
cd $R
grep -a '^{"metric"' $OUT/rocprof_stats.log | tail -1 > $OUT/pmc_bench_line.json
python tools/pmc_summary.py $OUT $OUT/pmc_summary_final.json $OUT/pmc_bench_line.json
python tools/kstats.py $OUT/pmc_stats "rocprofv3 --kernel-trace --stats : python bench.py --steps 5 --warmup 2 --no-cpu-baseline --no-train (MI355X)" > $OUT/bench_kernel_stats_final.md
head -12 $OUT/bench_kernel_stats_final.md
rm -rf $OUT/pmc_*/ $OUT/pmc_stats
# ---- the same passes over the batch-64 train step (the filter-gradient and BatchNorm kernels): folded under "train_step" of the same summary
mkdir -p $OUT/train
cd /tmp
for c in FETCH_SIZE WRITE_SIZE "SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE"; do
  tag=$(echo $c | tr ' ' '_' | cut -c1-24)
  Y3_NO_EXCHANGE_LEG=1 timeout 600 rocprofv3 --kernel-trace --pmc $c -d $OUT/train/pmc_$tag -o pmc -- python $R/bench.py --mode train --batch 64 --steps 3 --warmup 2 --full > $OUT/train/pmc_$tag.log 2>&1; echo "exit $?" >> $OUT/train/pmc_$tag.log
done
Y3_NO_EXCHANGE_LEG=1 timeout 600 rocprofv3 --kernel-trace --stats -d $OUT/train/pmc_stats -o bench -- python $R/bench.py --mode train --batch 64 --steps 3 --warmup 2 --full > $OUT/train/rocprof_stats.log 2>&1
cd $R
python tools/pmc_summary.py $OUT/train $OUT/pmc_summary_train.json
python tools/kstats.py $OUT/train/pmc_stats "rocprofv3 --kernel-trace --stats : python bench.py --mode train --batch 64 --steps 3 --warmup 2 (MI355X)" 40 > $OUT/train_kernel_stats_final.md
python - <<'PY'
import json
import os
O = os.environ["OUT"]
a = json.load(open(f"{O}/pmc_summary_final.json"))
a["train_step"] = json.load(open(f"{O}/pmc_summary_train.json"))
json.dump(a, open(f"{O}/pmc_summary_final.json", "w"), indent=1)
PY
rm -rf $OUT/train/pmc_*/ $OUT/train/pmc_stats
