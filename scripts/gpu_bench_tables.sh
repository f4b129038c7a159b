# round-2 bench tables: the bench line (--full) and rocprofv3 kernel tables of the bench command (files land in $OUT, default results/)
OUT=${OUT:-results}
mkdir -p $OUT
python bench.py --full > $OUT/r02_bench.json 2> $OUT/r02_bench.err; tail -2 $OUT/r02_bench.err; head -c 600 $OUT/r02_bench.json; echo
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
rocprofv3 --kernel-trace --stats -d $OUT/prof_bench -o bench -- python bench.py --full --no-extras --no-cpu-baseline > $OUT/prof_bench.log 2>&1
grep '^{' $OUT/prof_bench.log > $OUT/r02_bench_under_rocprof.json
python scripts/prof_summary.py $OUT/prof_bench/bench_results.db > $OUT/r02_rocprof_kernel_stats_bench.txt
KBA_GROUPS=1 rocprofv3 --kernel-trace --stats -d $OUT/prof_bench1 -o bench -- python bench.py --full --no-extras --no-cpu-baseline > $OUT/prof_bench1.log 2>&1
python scripts/prof_summary.py $OUT/prof_bench1/bench_results.db > $OUT/r02_rocprof_kernel_stats_bench_one_group.txt; head -12 $OUT/r02_rocprof_kernel_stats_bench_one_group.txt
