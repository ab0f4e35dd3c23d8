#!/bin/bash
# The measurements of profiles/r20_base_trajectory/, one session on one GPU:
#   bash scripts/base_trajectory_bench.sh <out dir> [<tree of the parent commit, built>]
# Rates of scripts/base_trajectory_bench.py at N=2 and on the mesh refined twice
# (forward and adjoint, every variant) and beside them -- with a parent tree --
# the constant-base loop of the parent commit by its own
# scripts/linearised_bench.py.  Every step that uses the GPU has its own time
# limit; a step that fails ends the script.
set -o pipefail
OUT=${1:?out dir}
PARENT=${2:-}
R=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$OUT"
OUT=$(cd "$OUT" && pwd)
cd "$R" || exit 1

parent_leg() {   # <refine> <repeats> <file>
    [ -z "$PARENT" ] && return 0
    (cd "$PARENT" && timeout -k 10 420 python scripts/linearised_bench.py \
        --legs forward,adjoint --refine "$1" --repeats "$2" --out "$3")
}

timeout -k 10 420 python scripts/base_trajectory_bench.py --repeats 3 \
    --out "$OUT/legs_n2.json" > "$OUT/n2.stdout.txt" &&
parent_leg 0 3 "$OUT/parent_n2.json" > "$OUT/parent_n2.stdout.txt" &&
timeout -k 10 900 python scripts/base_trajectory_bench.py --refine 2 \
    --repeats 3 --out "$OUT/legs_refine2.json" > "$OUT/refine2.stdout.txt" &&
parent_leg 2 3 "$OUT/parent_refine2.json" > "$OUT/parent_refine2.stdout.txt" &&
echo "base_trajectory_bench: done"
