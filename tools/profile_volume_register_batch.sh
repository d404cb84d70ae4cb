#!/bin/bash
# profile_volume_register_batch.sh OUT_DIR -- the measurements behind profiles/volume_register_batch_times.json:
#   1. examples/cpp/PoseCorrection.bin --synthetic 200 5 1 --res 0.005 --path refine --iters 10, --refine single against --refine batch of the SAME
#      binary, at --perturb 20 and --perturb 200 (every frame) and at --stride 4 and --stride 1: a fresh process per run, the two modes alternating,
#      one untimed pass of each and five timed ones; the last line (JSON) of every timed run in OUT_DIR/times.jsonl, tagged with its setting.  What is
#      compared is "refine"."estimate_ms": the K registrations, frames resident on the device in both modes
#   2. the batch mode of --perturb 20 --stride 4 under the kernel tracer, in a run of its own; the k_volume_register* / k_register_* rows in
#      OUT_DIR/kernel_stats.csv
# Every run has its own time limit and the first failure ends the script.  Run from the repository root after __graft_entry__.build().
out=${1:?usage: profile_volume_register_batch.sh OUT_DIR}
mkdir -p "$out"
exe=examples/cpp/PoseCorrection.bin
args="--synthetic 200 5 1 --res 0.005 --path refine --iters 10"
: > "$out/times.jsonl"
for perturb in 20 200; do
  for stride in 4 1; do
    for pass in 0 1 2 3 4 5; do
      for mode in single batch; do
        echo "== perturb $perturb stride $stride pass $pass $mode"
        timeout -k 10 200 $exe $args --perturb $perturb --stride $stride --refine $mode > "$out/last.log" 2>&1 || { echo "run failed"; tail -5 "$out/last.log"; exit 1; }
        if [ $pass -gt 0 ]; then echo "{\"perturb\": $perturb, \"stride\": $stride, \"mode\": \"$mode\", \"run\": $(tail -1 "$out/last.log")}" | tee -a "$out/times.jsonl"; fi
      done
    done
  done
done
: > "$out/kernel_stats.csv"
d=$(mktemp -d)
echo "== batch (kernel trace)"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$d" -o run -- $exe $args --perturb 20 --stride 4 --refine batch > "$out/last.log" 2>&1 || { echo "run failed"; tail -5 "$out/last.log"; exit 1; }
f=$(find "$d" -name '*kernel_stats.csv' | head -1)
[ -n "$f" ] || { echo "no kernel stats written"; exit 1; }
echo "\"setting\",$(head -1 "$f")" >> "$out/kernel_stats.csv"
grep -E "k_volume_register|k_register_" "$f" | sed "s/^/\"batch\",/" | tee -a "$out/kernel_stats.csv"
rm -rf "$d"
