#!/bin/bash
# Same-box A/B of the pose chains WITHOUT the scene filter between two checkouts, each with its own built library, package and scripts (in
# the manner of scripts/ab_pose_refine.sh): what an object that never called set_scene_filter costs before and after the filter was added.
#   scripts/ab_scene_filter.sh <checkout root A> <checkout root B> [rounds] [repeats]
# alternates A and B, one process each: <root>/scripts/pose_chain_bench.py and <root>/scripts/rough_pose_bench.py on their 64-frame
# workload, and prints each run's wall-time and kernel-time lines.  Give the same root twice for the spread a build shows against itself.
set -o pipefail
unset LMX_SO_PATH
a=$1; b=$2; rounds=${3:-2}; repeats=${4:-20}
tmp=$(mktemp -d)
for r in $(seq $rounds); do
  for w in A B; do
    root=$a; [ $w = B ] && root=$b
    timeout -k 10 300 python "$root/scripts/pose_chain_bench.py" --repeats $repeats --blocks 2 --block-steps 5 --cap-clusters 512 --out "$tmp/chain.txt" >/dev/null 2>&1 || exit 1
    grep -E "^ +(staged|chain) |k_pose_refine" "$tmp/chain.txt" | sed "s/^/$w round $r  pose_chain /"
    timeout -k 10 300 python "$root/scripts/rough_pose_bench.py" --repeats $repeats --out "$tmp/rough.txt" >/dev/null 2>&1 || exit 1
    grep -E "median|k_rough|k_pose" "$tmp/rough.txt" | sed "s/^/$w round $r  rough_pose /"
  done
done
rm -rf "$tmp"
