#!/bin/bash
# GPU tests + smoke + bench (--full: rooflines, extras, CPU baseline) + rocprofv3 kernel-trace summary of the SAME bench command
# (files land in $OUT, default results/)
OUT=${OUT:-results}
mkdir -p $OUT profiles
python -m pytest tests -m gpu -x -q 2>&1 | tail -6
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -2
python bench.py --full > $OUT/bench.json 2> $OUT/bench.err; tail -2 $OUT/bench.err; cat $OUT/bench.json
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
rocprofv3 --kernel-trace --stats -d $OUT/prof_bench -o bench -- python bench.py --full > $OUT/prof_bench.log 2>&1
grep '^{' $OUT/prof_bench.log > $OUT/bench_under_rocprof.json
python scripts/prof_summary.py $OUT/prof_bench/bench_results.db > $OUT/rocprof_kernel_stats.txt; cat $OUT/rocprof_kernel_stats.txt
