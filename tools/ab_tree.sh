#!/bin/bash
# Same-box A/B of two TREES (library + compiler + engine): the baseline exported with `git archive <rev>` into .ab_base/ and built there
# in the build container, against the working tree.  Headline workload (configs[1], B = 1024, 64 steps), alternating.
#   tools/ab_tree.sh [bench args ...]
# Every run has its own time limit, and the first run that fails ends the comparison (nothing more is started on the GPU).
set -o pipefail
Q="${@:---full --no-breakdown --no-cpu-baseline --no-exact-f32 --no-other-configs --steps 3 --warmup 1}"
one() { (cd $1 && timeout -k 10 ${AB_TIMEOUT:-300} python bench.py $Q 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); e=d.get('unet_eval') or {}; print('$2', d['value'], e.get('ms_avg_graph_replay'), e.get('launches'))"); }
for i in 1 2 3; do
  one .ab_base base || { echo "base run $i failed: stopping"; exit 1; }
  one . current || { echo "current run $i failed: stopping"; exit 1; }
done
