#!/bin/bash
# The recipe of profiles/r32_stems.txt (tools/stems_cost.py says what each part measures).  Run on the GPU box from the
# repository root with the library built; every GPU step runs under a time limit of its own and the steps are chained
# with &&: a step that fails, faults or runs into its limit ends the recipe.  The counters of a kernel, if a figure
# needs explaining (k_mix_levels above twice k_noise_sums), are collected in a run of their own, never beside a trace.
#   PARENT=DIR  a checkout of the parent commit with its library built: its bench.py runs alternate with this tree's,
#               and its jb_mix_pcm_batch runs the seam baseline; without it both are left out
set -euo pipefail
cd "$(dirname "$0")/.."
OUT=${OUT:-tools/_ab_stems}
PARENT=${PARENT:-}
mkdir -p "$OUT"
rm -f "$OUT"/bench_parent.jsonl "$OUT"/bench_tree.jsonl
# one bench.py run in the checkout $1, its JSON line appended to $2
bench() {
  (cd "$1" && timeout -k 10 400 python bench.py --gpus 1 --steps 10 --warmup 3 | tail -1) >> "$2"
}
# (one && chain and no loop: in a loop or under `if` a failing step would not end the shell.  pipefail is set: a
# bench.py that fails, faults or runs into its limit fails its step though `tail` succeeds)
if [ -n "$PARENT" ]; then
  bench "$PARENT" "$OUT"/bench_parent.jsonl && bench . "$OUT"/bench_tree.jsonl &&
  bench "$PARENT" "$OUT"/bench_parent.jsonl && bench . "$OUT"/bench_tree.jsonl &&
  bench "$PARENT" "$OUT"/bench_parent.jsonl && bench . "$OUT"/bench_tree.jsonl &&
  (cd "$PARENT" && timeout -k 10 300 rocprofv3 --kernel-trace -d "$OLDPWD/$OUT/seam_parent" -o seam -- \
     env JB_COST_ROOT="$PWD" python "$OLDPWD"/tools/stems_cost.py --seam-run) || exit 1
fi
timeout -k 10 300 rocprofv3 --kernel-trace -d "$OUT"/seam_tree -o seam -- python tools/stems_cost.py --seam-run &&
timeout -k 10 600 rocprofv3 --kernel-trace -d "$OUT"/trace -o stems -- python tools/stems_cost.py --trace-run &&
timeout -k 10 300 python -m pytest tests/test_stems_abi.py -k long_double -s -q -p no:cacheprovider > "$OUT"/gate.log &&
timeout -k 10 900 python tools/stems_cost.py --kernels "$OUT" --gate "$OUT"/gate.log \
  ${PARENT:+--bench-before "$OUT"/bench_parent.jsonl --bench-after "$OUT"/bench_tree.jsonl} "$@"
