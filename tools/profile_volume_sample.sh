#!/bin/bash
# profile_volume_sample.sh OUT_DIR -- the measurements behind profiles/volume_sample_times.json and profiles/volume_sample_kernel_stats.csv:
#   1. examples/cpp/ModelQuery.bin --synthetic 200 5 1 --res 0.005 --warmup 1 --repeat 5 for every query set, mode and path: a fresh process per setting,
#      the host and the device path alternating; one JSON line per run in OUT_DIR/times.jsonl
#   2. the device path of the mesh and mesh-shuffled sets under the kernel tracer, in runs of their own; the k_volume_sample rows in OUT_DIR/kernel_stats.csv
# Every run has its own time limit and the first failure ends the script.  Run from the repository root after __graft_entry__.build().
out=${1:?usage: profile_volume_sample.sh OUT_DIR}
mkdir -p "$out"
exe=examples/cpp/ModelQuery.bin
args="--synthetic 200 5 1 --res 0.005 --warmup 1 --repeat 5"
: > "$out/times.jsonl"
for q in mesh mesh-shuffled frame; do
  for m in "--mode trilinear" "--mode trilinear --gradients" "--mode reference"; do
    for p in host device; do
      echo "== $q $m $p"
      timeout -k 10 300 $exe $args --queries $q $m --path $p > "$out/last.log" 2>&1 || { echo "run failed"; tail -5 "$out/last.log"; exit 1; }
      tail -1 "$out/last.log" | tee -a "$out/times.jsonl"
    done
  done
done
: > "$out/kernel_stats.csv"
for q in mesh mesh-shuffled; do
  for m in "--mode trilinear" "--mode trilinear --gradients" "--mode reference"; do
    d=$(mktemp -d)
    echo "== $q $m (kernel trace)"
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$d" -o run -- $exe $args --queries $q $m --path device > "$out/last.log" 2>&1 || { echo "run failed"; tail -5 "$out/last.log"; exit 1; }
    f=$(find "$d" -name '*kernel_stats.csv' | head -1)
    [ -n "$f" ] || { echo "no kernel stats written"; exit 1; }
    [ -s "$out/kernel_stats.csv" ] || echo "\"setting\",$(head -1 "$f")" >> "$out/kernel_stats.csv"
    grep k_volume_sample "$f" | sed "s/^/\"$q $m\",/" | tee -a "$out/kernel_stats.csv"
    rm -rf "$d"
  done
done
