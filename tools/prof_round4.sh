#!/bin/bash
# GPU box: everything profiles/ holds for round 4.  Outputs under gpurun_out/round4/ (copied to profiles/r04_* by hand).
#   usage: tools/prof_round4.sh <commit>      (the GPU box has no .git: the commit the tree was built from is passed in)
export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-/root/repo}
C=${1:-unrecorded}
O=$R/gpurun_out/round4
mkdir -p $O
cd $R
echo "commit $C" > $O/commit.txt
python bench.py --full > $O/bench_line.json 2> $O/bench_stderr.log
tail -1 $O/bench_line.json | cut -c1-200
python bench.py --full --n 100000 --pairs 32 --steps 3 --warmup 1 --no-cpu-baseline --sustain-s 0 > $O/bench_line_n100k.json 2>> $O/bench_stderr.log
python bench.py --full --mode GPF --no-cpu-baseline --sustain-s 0 > $O/bench_line_gpf.json 2>> $O/bench_stderr.log
python bench.py --full --codebase GC --no-cpu-baseline --sustain-s 0 > $O/bench_line_gc.json 2>> $O/bench_stderr.log
cd /tmp
prof() {   # tag, then bench args
  tag=$1; shift
  rm -rf /tmp/p_$tag
  rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/p_$tag -o $tag -- python3 $R/bench.py --no-cpu-baseline "$@" > /tmp/p_$tag.log 2>&1
  cp "$(find /tmp/p_$tag -name '*kernel_stats.csv' | head -1)" $O/${tag}_kernel_stats.csv
}
prof bench_streams1 --streams 1 --pairs 64 --steps 3 --warmup 1 --sustain-s 0
prof bench_default --steps 3 --warmup 1 --sustain-s 0
prof bench_sustained --steps 10 --warmup 2 --sustain-s 10 --full          # the >= 10 s run: AverageNs of the filter pass over ~600 steps
grep -o '"sustained": {[^}]*}' /tmp/p_bench_sustained.log > $O/bench_sustained_under_profiler.txt
prof bench_gpf_streams1 --mode GPF --streams 1 --pairs 64 --steps 3 --warmup 1 --sustain-s 0
prof bench_n100k_streams1 --n 100000 --streams 1 --pairs 16 --batch 8 --steps 3 --warmup 1 --sustain-s 0
prof bench_gc_streams1 --codebase GC --streams 1 --pairs 64 --steps 3 --warmup 1 --sustain-s 0
for c in FETCH_SIZE WRITE_SIZE; do
  rm -rf /tmp/p_$c
  rocprofv3 --pmc $c --output-format csv -d /tmp/p_$c -o c -- python3 $R/bench.py --steps 2 --warmup 1 --streams 1 --pairs 32 --no-cpu-baseline --sustain-s 0 > /tmp/p_$c.log 2>&1
  cp "$(find /tmp/p_$c -name '*counter_collection.csv' | head -1)" /tmp/pmc_$c.csv
done
python3 $R/tools/pmc_to_json.py /tmp/pmc_FETCH_SIZE.csv /tmp/pmc_WRITE_SIZE.csv $O/pmc_traffic.json "$C" > $O/pmc_traffic.txt
bash $R/tools/pmc_bench.sh --sustain-s 0 > $O/pmc_sq_summary.txt 2>&1
bash $R/tools/pmc_passb.sh > $O/pmc_passb_summary.txt 2>&1
for l in A B; do python $R/bench.py --list $l --no-cpu-baseline > $O/list_${l}_bench_line.json 2>> $O/bench_stderr.log; done
( cd $R && STREAMS=1 LISTS="A B" STRIDE=8 tools/r4_listprof.sh > /dev/null 2>&1; cp gpurun_out/r4_listprof/list_A_s1_kernel_stats.csv $O/list_A_streams1_kernel_stats.csv; cp gpurun_out/r4_listprof/list_B_s1_kernel_stats.csv $O/list_B_streams1_kernel_stats.csv )
( cd $R && [ -f tools/bin/liblidarreg_probe.so ] && STRIDE=8 tools/r4_loprobe.sh run > /dev/null 2>&1 && cp gpurun_out/r4_loprobe/probe.txt $O/lo_probe.txt )
bash $R/tools/single_pair_prof.sh > $O/single_pair_kernels.txt 2>&1
python $R/tools/fr_latency.py 2>/dev/null > $O/fr_latency.txt
( cd $R && tools/bin/pb_micro_new 30000 32 1 > $O/pb_micro.txt 2>&1; tools/bin/pb_micro_new 30000 1 6 > $O/pb_micro_single.txt 2>&1 )
ls -la $O
