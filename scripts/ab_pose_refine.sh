#!/bin/bash
# Same-box A/B of k_pose_refine without a schedule between two checkouts, each with its own built library and Python package (what
# scripts/ab_libs.sh does for the matching workload; a library from before the refinement schedule lacks symbols today's package asks
# for, so each side runs its own package):
#   scripts/ab_pose_refine.sh <checkout root A> <checkout root B> [rounds] [repeats]
# alternates A and B, one process each: scripts/pose_refine_bench.py --plain, the 1 / 16 / 256-job rows.  Give the same root twice for the
# spread a build shows against itself.
set -o pipefail
unset LMX_SO_PATH
a=$1; b=$2; rounds=${3:-2}; repeats=${4:-20}
here=$(cd "$(dirname "$0")" && pwd)
for r in $(seq $rounds); do
  for w in A B; do
    root=$a; [ $w = B ] && root=$b
    timeout -k 10 300 python "$here/pose_refine_bench.py" --plain --rounds 2 --repeats $repeats --package-root "$root" 2>/dev/null | sed "s/^/$w round $r  /" || exit 1
  done
done
