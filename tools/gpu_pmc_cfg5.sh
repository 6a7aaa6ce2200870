#!/bin/bash
# usage: tools/gpu_pmc_cfg5.sh <tag> "<counters>"   -- one rocprofv3 --kernel-trace --pmc pass of the config-5 bench (B=512, u8, 1e6 transitions)
out=${OUT:-out}      # output folder, relative to the repository root
tag=$1; ctrs=$2
R=$(pwd); mkdir -p $R/$out; cd /tmp; export TMPDIR=/tmp
rocprofv3 --kernel-trace --pmc $ctrs -d $R/$out/$tag -o r -- python $R/bench.py --full --batch 512 --u8 --replay 1000000 --device-fill --steps 6 --warmup 3 --profile-steps 1 --no-cpu-baseline --env-steps 0 --no-graph > $R/$out/${tag}.log 2>&1
python $R/tools/rocprof_pmc.py $R/$out/$tag/r_results.db | grep -v "^columns" > $R/$out/${tag}_pmc.txt
rm -rf $R/$out/$tag
