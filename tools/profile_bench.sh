#!/bin/bash
# usage (on a box with the GPU, from the repository's root): tools/profile_bench.sh <tag> [bench args...]
# Runs bench.py once with --full (JSON line with cpu_baseline -> $OUT/<tag>_bench.json) and once plain under
# rocprofv3 --kernel-trace --stats; keeps only the text summary (-> $OUT/<tag>_kernel_stats.txt).  OUT: bench_outputs/profile unless set.
set -u
tag=$1; shift
OUT=${OUT:-bench_outputs/profile}
work=$(mktemp -d)
mkdir -p $OUT
python bench.py "$@" --full 2>/dev/null | grep '^{"metric"' > $OUT/${tag}_bench.json
rocprofv3 --kernel-trace --stats -d $work -o p -- python bench.py "$@" > $work/log.txt 2>&1
python tools/rocpd_summary.py $(ls $work/*.db | head -1) > $OUT/${tag}_kernel_stats.txt
grep '^{"metric"' $work/log.txt > $OUT/${tag}_bench_under_rocprof.json
head -c 1500 $OUT/${tag}_bench.json; echo
