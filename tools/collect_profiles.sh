#!/bin/bash
# usage (after tools/profile_forward.sh <tag> and tools/profile_round.sh <tag> ran and their $PROFILE_OUT folder is in this tree):
# tools/collect_profiles.sh <tag>  -- copies the summaries the judge reads into profiles/<tag>_*
out=${PROFILE_OUT:-profile_out}      # where the profiles land (relative to the repo root, git-ignored)
tag=${1:-r03}
o=$out/$tag
python tools/trim_stats.py $o/stats/s_kernel_stats.csv profiles/${tag}_train_step_kernel_stats.csv
cp $o/hbm_traffic.json profiles/${tag}_hbm_traffic.json
cp $o/bench.json profiles/${tag}_train_step_bench_under_rocprof.json
for B in 65536 1048576; do
  python tools/trim_stats.py $o/fwd_$B/stats/s_kernel_stats.csv profiles/${tag}_forward_bs${B}_kernel_stats.csv
  cp $o/fwd_$B/hbm_traffic.json profiles/${tag}_forward_bs${B}_hbm_traffic.json
done
[ -f $out/pmc_${tag}_fwd1m.txt ] && cp $out/pmc_${tag}_fwd1m.txt profiles/${tag}_forward_bs1048576_sq_counters.txt
ls -la profiles/${tag}_*
