cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
OUT=${MVIP_PROFILE_OUT:-profile_out}; export OUT            # where every file of this script lands, relative to the repository
mkdir -p $R/$OUT/prof_r1h $R/$OUT/pmc_r1h
cd $R
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_r1h -o run -- python3 bench.py --full > $OUT/prof_r1h/bench_line.json 2> $OUT/prof_r1h/err.log
find $OUT/prof_r1h -name '*kernel_stats.csv' | head -1 | xargs -I{} python3 -c "
import csv,sys
rows=list(csv.reader(open('{}')))
w=csv.writer(open('$OUT/prof_r1h/top30.csv','w'),quoting=csv.QUOTE_ALL)
w.writerow(rows[0])
for r in rows[1:31]:
    r[0]=r[0][:110]; w.writerow(r)
"
find $OUT/prof_r1h -name '*kernel_trace.csv' -delete
rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE --kernel-trace --output-format csv -d $OUT/pmc_r1h -o run -- python3 bench.py --full --steps 1 --warmup 0 --train-steps 1 --sds-steps 1 --no-cpu-baseline --no-hashgrid > $OUT/pmc_r1h/line.json 2> $OUT/pmc_r1h/err.log
find $OUT/pmc_r1h -name '*counter_collection.csv' | head -1 | xargs -I{} python3 tools/pmc_summary.py {} $OUT/pmc_r1h/summary.json > $OUT/pmc_r1h/summary_top.txt
find $OUT/pmc_r1h -name '*.csv' -delete
tail -c 600 $OUT/prof_r1h/bench_line.json; head -c 2500 $OUT/pmc_r1h/summary_top.txt
