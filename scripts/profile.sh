#!/bin/bash
# usage (on the MI355X, from the repository root): bash scripts/profile.sh <tag> [bench args...]
# writes $OUT/prof_<tag>/ and prints the kernel stats; copy the csv into profiles/ afterwards.
tag=$1; shift
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-out}; export OUT; mkdir -p "$OUT"      # results go under $OUT (default: out/ in the repository root)
rm -rf $OUT/prof_$tag
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$tag -- python3 bench.py --full --steps 50 --warmup 5 --no-cpu-baseline --no-graph --min-seconds 0 "$@" > $OUT/prof_$tag.log 2>&1
cat $OUT/prof_$tag/*/*_kernel_stats.csv | cut -c1-200 | head -16
grep -E '^\{' $OUT/prof_$tag.log | cut -c1-400
