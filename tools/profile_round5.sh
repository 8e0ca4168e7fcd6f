# Round-5 evidence run on the GPU box -- run as the LAST step of the round, after the last kernel change:
#     gpurun --timeout 2400 -- "MVIP_HEAD=$(git rev-parse HEAD) bash tools/profile_round5.sh"
# (the snapshot carries no .git: the commit the files belong to comes in through MVIP_HEAD and is written INTO every JSON the
# script produces, and into r5_profile_head.json for the CSV / text files).  Every file lands in $OUT/ under the name it is
# committed as in profiles/:
#  (1) rocprofv3 --kernel-trace --stats of the full bench command (--full)        -> r5_bench_kernel_stats.csv, r5_bench_line_under_rocprof.json
#  (2) matrix-pipe utilisation per kernel (PMC) of a short bench            -> r5_pmc_mfma_util.json        (render, training, SDS kernels)
#  (3) HBM traffic of the dominant render launch (FETCH_SIZE / WRITE_SIZE)  -> r5_pmc_mlp_forward.json
#  (4) HBM traffic of STEADY-STATE SDS steps per kernel                     -> r5_pmc_sds_traffic.json
#  (5) one SDS step per kernel + hipGraph replay, fp32 networks and --fp16  -> r5_sds_step_f32.json, r5_sds_step_fp16.json
#  (6) isolated HBM-bound stage kernels                                      -> r5_micro_hbm_kernels.jsonl
#  (7) configs[2] / configs[3] iterations per kernel                         -> r5_config2_step_kernels.json, r5_config3_step_kernels.json
#  (8) the round's A/Bs on the final build: split-precision forward (one vs two waves per SIMD), fused render vs chain,
#      SDS step on one vs two streams                                        -> r5_f16x3_w16_ab.json, r5_fused_render_ab.json, r5_sds_two_stream_ab.json
# PMC runs are their own processes with --kernel-trace only (never combined with --stats / sys-trace), with the SDS steps launched
# kernel by kernel (MVIP_SDS_GRAPHS=0) and under their own timeouts.
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
OUT=${MVIP_PROFILE_OUT:-profile_out}; export OUT            # where every file of this script lands, relative to the repository
cd $R
HEAD=${MVIP_HEAD:-unknown}
mkdir -p $OUT/prof_r5 $OUT/pmc_r5
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_r5 -o run -- python3 bench.py --full > $OUT/r5_bench_line_under_rocprof.json 2> $OUT/prof_r5/err.log
find $OUT/prof_r5 -name '*kernel_stats.csv' | head -1 | xargs -I{} python3 -c "
import csv
rows=list(csv.reader(open('{}')))
w=csv.writer(open('$OUT/r5_bench_kernel_stats.csv','w'),quoting=csv.QUOTE_ALL)
w.writerow(rows[0])
for r in rows[1:41]:
    r[0]=r[0][:110]; w.writerow(r)
"
find $OUT/prof_r5 -name '*kernel_trace.csv' -delete; find $OUT/prof_r5 -name '*.db' -delete
MVIP_HEAD=$HEAD bash tools/pmc_mfma_util.sh > $OUT/pmc_r5/summary_top.txt 2>&1     # three bounded passes (see the script)
cd /tmp; cd $GRAFT_REPO_ROOT
for C in FETCH_SIZE WRITE_SIZE; do
  c=$(echo $C | tr A-Z a-z | sed 's/_size//')
  D=$OUT/pmc_r5_$c; mkdir -p $D
  MVIP_SDS_GRAPHS=0 timeout 600 rocprofv3 --pmc $C --kernel-trace --output-format csv -d $D -o run -- python3 bench.py --full --steps 1 --warmup 0 --train-steps 0 --sds-steps 0 --no-cpu-baseline --no-hashgrid > $D/line.json 2> $D/err.log
  find $D -name '*counter_collection.csv' | head -1 | xargs -I{} python3 tools/pmc_summary.py {} --longest mlp_forward16_kernel > $D/dominant.json
  find $D -name '*.csv' -delete; find $D -name '*.db' -delete
  D=$OUT/pmc_r5_sds_$c; mkdir -p $D
  timeout 420 rocprofv3 --pmc $C --kernel-trace --output-format csv -d $D -o run -- python3 tools/sds_profile_steps.py 5 > $D/out.txt 2> $D/err.log
  find $D -name '*counter_collection.csv' | head -1 | xargs -I{} cp {} $D/cc.csv
  find $D -name '*.db' -delete
done
python3 - <<'P'
import json, os
f = json.load(open(os.environ['OUT'] + '/pmc_r5_fetch/dominant.json')); w = json.load(open(os.environ['OUT'] + '/pmc_r5_write/dominant.json'))
pts = 190512 * 128
json.dump({'kernel': 'mvip::f16p::mlp_forward16_kernel<true,false,0> (fine pass of one 378x504 frame: 190,512 rays x 128 samples; the longest dispatch)',
           'fetch_size_KB': f['value_KB'], 'write_size_KB': w['value_KB'], 'hbm_bytes_per_launch': (2 * f['value_KB'] + w['value_KB']) * 1024,
           'launch_ms': max(f['ms'], w['ms']), 'algorithmic_bytes': pts * 20 + 190512 * 44,
           'command': 'rocprofv3 --pmc FETCH_SIZE (resp. WRITE_SIZE) --kernel-trace --output-format csv -- python3 bench.py --full --steps 1 --warmup 0 --train-steps 0 --sds-steps 0 --no-cpu-baseline --no-hashgrid; longest mlp_forward16_kernel dispatch (tools/pmc_summary.py --longest); FETCH doubled per the gfx950 note'},
          open(os.environ['OUT'] + '/r5_pmc_mlp_forward.json', 'w'), indent=1)
P
python3 tools/pmc_sds_traffic.py $OUT/pmc_r5_sds_fetch/cc.csv $OUT/pmc_r5_sds_write/cc.csv 5 $OUT/r5_pmc_sds_traffic.json 2 > $OUT/r5_pmc_sds_traffic.txt 2>&1
find $OUT/pmc_r5_sds_fetch $OUT/pmc_r5_sds_write -name '*.csv' -delete
python3 tools/sds_step_profile.py --graphs --out=r5_sds_step_f32.json > $OUT/r5_sds_step_f32.txt 2>&1
python3 tools/sds_step_profile.py --fp16 --graphs --out=r5_sds_step_fp16.json > $OUT/r5_sds_step_fp16.txt 2>&1
python3 tools/micro_bench.py 2>/dev/null | grep '^{' > $OUT/r5_micro_hbm_kernels.jsonl
python3 tools/config_step_profile.py 2 > $OUT/r5_config2.txt 2>&1
python3 tools/config_step_profile.py 3 > $OUT/r5_config3.txt 2>&1
python3 tools/f16x3_w16_ab.py > $OUT/r5_f16x3_w16_ab.txt 2>&1
python3 tools/fused_render_ab.py > $OUT/r5_fused_render_ab.txt 2>&1
python3 tools/sds_two_stream_ab.py > $OUT/r5_sds_two_stream_ab.txt 2>&1
# ---- stamp: the commit goes INTO every JSON (a list becomes {"head", "rows"}), and next to the CSV / text files ----
MVIP_HEAD=$HEAD python3 - <<'P'
import glob, json, os
head = os.environ.get('MVIP_HEAD', 'unknown')
stamped = []
for p in sorted(glob.glob(os.environ['OUT'] + '/r5_*.json')):
    if p.endswith('r5_profile_head.json'):
        continue
    try:
        d = json.load(open(p))
    except Exception:
        continue
    if isinstance(d, list):
        d = {'head': head, 'rows': d}
    else:
        d['head'] = head
    json.dump(d, open(p, 'w'), indent=1)
    stamped.append(os.path.basename(p))
others = sorted(os.path.basename(p) for p in glob.glob(os.environ['OUT'] + '/r5_*') if not p.endswith('.json'))
json.dump({'head': head, 'what': 'every r5_* file of the output folder below was produced by ONE run of tools/profile_round5.sh on a snapshot of this commit',
           'json_files_stamped': stamped, 'other_files': others}, open(os.environ['OUT'] + '/r5_profile_head.json', 'w'), indent=1)
P
tail -c 400 $OUT/r5_bench_line_under_rocprof.json; echo; head -c 1500 $OUT/pmc_r5/summary_top.txt; cat $OUT/r5_pmc_mlp_forward.json; head -18 $OUT/r5_pmc_sds_traffic.txt
