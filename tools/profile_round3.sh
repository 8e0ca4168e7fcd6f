# Round-3 evidence run on the GPU box: (1) rocprofv3 --kernel-trace --stats of the full bench command (--full), (2) matrix-pipe
# utilisation per kernel (PMC) of a short bench, (3) HBM traffic of the dominant render launch and of ONE SDS step per kernel
# (FETCH_SIZE / WRITE_SIZE in separate passes), (4) per-kernel torch-profiler views.  Summaries land in $OUT/ and are
# copied into profiles/ as r3_*.
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
OUT=${MVIP_PROFILE_OUT:-profile_out}; export OUT            # where every file of this script lands, relative to the repository
cd $R
mkdir -p $OUT/prof_r3 $OUT/pmc_r3 $OUT/pmc_r3_fetch $OUT/pmc_r3_write $OUT/pmc_r3_sds_fetch $OUT/pmc_r3_sds_write
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_r3 -o run -- python3 bench.py --full > $OUT/prof_r3/bench_line.json 2> $OUT/prof_r3/err.log
find $OUT/prof_r3 -name '*kernel_stats.csv' | head -1 | xargs -I{} python3 -c "
import csv
rows=list(csv.reader(open('{}')))
w=csv.writer(open('$OUT/prof_r3/top40.csv','w'),quoting=csv.QUOTE_ALL)
w.writerow(rows[0])
for r in rows[1:41]:
    r[0]=r[0][:110]; w.writerow(r)
"
find $OUT/prof_r3 -name '*kernel_trace.csv' -delete; find $OUT/prof_r3 -name '*.db' -delete
rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE --kernel-trace --output-format csv -d $OUT/pmc_r3 -o run -- python3 bench.py --full --steps 1 --warmup 0 --train-steps 1 --sds-steps 1 --no-cpu-baseline --no-hashgrid > $OUT/pmc_r3/line.json 2> $OUT/pmc_r3/err.log
find $OUT/pmc_r3 -name '*counter_collection.csv' | head -1 | xargs -I{} python3 tools/pmc_summary.py {} $OUT/pmc_r3/summary.json > $OUT/pmc_r3/summary_top.txt
find $OUT/pmc_r3 -name '*.csv' -delete; find $OUT/pmc_r3 -name '*.db' -delete
for C in FETCH_SIZE WRITE_SIZE; do
  D=$OUT/pmc_r3_$(echo $C | tr A-Z a-z | sed 's/_size//')
  rocprofv3 --pmc $C --kernel-trace --output-format csv -d $D -o run -- python3 bench.py --full --steps 1 --warmup 0 --train-steps 0 --sds-steps 0 --no-cpu-baseline --no-hashgrid > $D/line.json 2> $D/err.log
  find $D -name '*counter_collection.csv' | head -1 | xargs -I{} python3 tools/pmc_summary.py {} --longest mlp_forward16_kernel > $D/dominant.json
  find $D -name '*.csv' -delete; find $D -name '*.db' -delete
  D=$OUT/pmc_r3_sds_$(echo $C | tr A-Z a-z | sed 's/_size//')
  rocprofv3 --pmc $C --kernel-trace --output-format csv -d $D -o run -- python3 tools/sds_profile_steps.py 3 > $D/out.txt 2> $D/err.log
  find $D -name '*counter_collection.csv' | head -1 | xargs -I{} cp {} $D/cc.csv
  find $D -name '*.db' -delete
done
python3 tools/pmc_sds_traffic.py $OUT/pmc_r3_sds_fetch/cc.csv $OUT/pmc_r3_sds_write/cc.csv 3 $OUT/r3_pmc_sds_traffic.json > $OUT/r3_pmc_sds_traffic.txt 2>&1
find $OUT/pmc_r3_sds_fetch $OUT/pmc_r3_sds_write -name '*.csv' -delete
python3 tools/sds_step_profile.py --graphs --out=r3_sds_step_f32.json > $OUT/r3_sds_step_f32.txt 2>&1
python3 tools/sds_step_profile.py --fp16 --graphs --out=r3_sds_step_fp16.json > $OUT/r3_sds_step_fp16.txt 2>&1
python3 tools/conv_kernel_times.py > $OUT/r3_conv_kernel_times.txt 2>&1
tail -c 300 $OUT/prof_r3/bench_line.json; echo; head -c 1500 $OUT/pmc_r3/summary_top.txt; cat $OUT/pmc_r3_fetch/dominant.json $OUT/pmc_r3_write/dominant.json; head -16 $OUT/r3_pmc_sds_traffic.txt
