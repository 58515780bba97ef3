#!/bin/bash
# usage: tools/pmc_step.sh <tag>  — HBM traffic (FETCH_SIZE, WRITE_SIZE; separate passes, counters only) of ONE
# step of the default bench with `--full` (the stage-1 launch of its first untimed leg closes the step), per kernel.  Writes
# $PROF_OUT/pmc_step_<tag>.json (default PROF_OUT: build/profiles).
tag=$1
root=$GRAFT_REPO_ROOT
out=${PROF_OUT:-$root/build/profiles}
mkdir -p $out
cd /tmp && export TMPDIR=/tmp
for c in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --pmc $c --output-format csv -d $out/pmc_step_${tag}/$c -- python $root/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-exact-leg > $out/pmc_step_${tag}_$c.log 2>&1
  echo "pass $c done"
done
cd $root
python3 tools/pmc_step.py $out/pmc_step_${tag} > $out/pmc_step_${tag}.json
cat $out/pmc_step_${tag}.json
