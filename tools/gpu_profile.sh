#!/bin/bash
# usage (on the GPU box, from the repo root): tools/gpu_profile.sh <tag> [bench args...]
# runs rocprofv3 --kernel-trace --stats on bench.py (eager launches so every kernel is a dispatch) and writes
# $OUT/<tag>_summary.txt (per-kernel table) + $OUT/<tag>_step.txt (one step's dispatch sequence); $OUT defaults to out
out=${OUT:-out}      # output folder, relative to the repository root
tag=$1; shift
R=$(pwd)
mkdir -p $R/$out
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $R/$out/$tag -o r -- python $R/bench.py --full --steps 50 --warmup 5 --profile-steps 1 --no-cpu-baseline --no-graph --sustained-steps 2000 --per-call-steps 0 --no-secondary "$@" > $R/$out/${tag}.log 2>&1
python $R/tools/rocprof_summary.py $R/$out/$tag/r_results.db > $R/$out/${tag}_summary.txt
python $R/tools/rocprof_step.py $R/$out/$tag/r_results.db > $R/$out/${tag}_step.txt
rm -rf $R/$out/$tag
tail -1 $R/$out/${tag}.log | cut -c1-300
