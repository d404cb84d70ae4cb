#!/bin/bash
# profile_volume_register.sh OUT_DIR -- the measurements behind profiles/volume_register_times.json:
#   1. examples/cpp/ModelRegistration.bin --synthetic 200 5 1 --res 0.005 --perturb 20 --iters 10 --path sample|fused: a fresh process per run, the
#      paths alternating, one untimed pass of each and five timed ones; one JSON line per timed run in OUT_DIR/times.jsonl
#   2. the fused path under the kernel tracer, in a run of its own; the k_volume_register / k_register_fold rows in OUT_DIR/kernel_stats.csv, and the
#      sample path likewise for its k_volume_sample row
# Every run has its own time limit and the first failure ends the script.  Run from the repository root after __graft_entry__.build().
out=${1:?usage: profile_volume_register.sh OUT_DIR}
mkdir -p "$out"
exe=examples/cpp/ModelRegistration.bin
args="--synthetic 200 5 1 --res 0.005 --perturb 20 --iters 10"
: > "$out/times.jsonl"
for pass in 0 1 2 3 4 5; do
  for p in sample fused; do
    echo "== pass $pass $p"
    timeout -k 10 200 $exe $args --path $p > "$out/last.log" 2>&1 || { echo "run failed"; tail -5 "$out/last.log"; exit 1; }
    if [ $pass -gt 0 ]; then tail -1 "$out/last.log" | tee -a "$out/times.jsonl"; fi
  done
done
: > "$out/kernel_stats.csv"
for p in fused sample; do
  d=$(mktemp -d)
  echo "== $p (kernel trace)"
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$d" -o run -- $exe $args --path $p > "$out/last.log" 2>&1 || { echo "run failed"; tail -5 "$out/last.log"; exit 1; }
  f=$(find "$d" -name '*kernel_stats.csv' | head -1)
  [ -n "$f" ] || { echo "no kernel stats written"; exit 1; }
  [ -s "$out/kernel_stats.csv" ] || echo "\"path\",$(head -1 "$f")" >> "$out/kernel_stats.csv"
  grep -E "k_volume_register|k_register_|k_volume_sample" "$f" | sed "s/^/\"$p\",/" | tee -a "$out/kernel_stats.csv"
  rm -rf "$d"
done
