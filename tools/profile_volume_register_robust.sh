#!/bin/bash
# profile_volume_register_robust.sh OUT_DIR [PARENT_EXE] -- the measurements behind profiles/volume_register_robust_times.json:
#   1. examples/cpp/ModelRegistration.bin --synthetic 200 5 1 --res 0.005 --perturb 20 --iters 10 --path fused: a fresh process per run, the settings
#      alternating, one untimed pass of each and five timed ones; the last line (JSON) of every timed run in OUT_DIR/times.jsonl, tagged with its
#      setting.  "new" is the command as it stands (no option: the entries that existed before the linearisations), "metric" the same with
#      --linearization metric.  With PARENT_EXE -- a ModelRegistration.bin built from the commit before the linearisations -- the same command takes
#      its turn in every pass ("parent"): what the zero-options path must cost, and the spread of its own repeats
#   2. the per-frame lines (pose error, iterations, status, last step) of --iters 30 --min-step 1e-5 under each linearisation, and of
#      --linearization normal with min_step 0 (the thirty iterations the documentation's figures were taken with), in OUT_DIR/frames_<what>.txt
#   3. --linearization metric under the kernel tracer, in a run of its own; the k_volume_register / k_register_fold rows in OUT_DIR/kernel_stats.csv
# Every run has its own time limit and the first failure ends the script.  Run from the repository root after __graft_entry__.build().
out=${1:?usage: profile_volume_register_robust.sh OUT_DIR [PARENT_EXE]}
parent=$2
mkdir -p "$out"
exe=examples/cpp/ModelRegistration.bin
args="--synthetic 200 5 1 --res 0.005 --perturb 20 --iters 10 --path fused"
settings="new metric"
[ -n "$parent" ] && settings="parent new metric"
: > "$out/times.jsonl"
for pass in 0 1 2 3 4 5; do
  for s in $settings; do
    echo "== pass $pass $s"
    case $s in
      parent) cmd="$parent $args" ;;
      new) cmd="$exe $args" ;;
      *) cmd="$exe $args --linearization $s" ;;
    esac
    timeout -k 10 200 $cmd > "$out/last.log" 2>&1 || { echo "run failed"; tail -5 "$out/last.log"; exit 1; }
    if [ $pass -gt 0 ]; then echo "{\"setting\": \"$s\", \"run\": $(tail -1 "$out/last.log")}" | tee -a "$out/times.jsonl"; fi
  done
done
long="--synthetic 200 5 1 --res 0.005 --perturb 20 --iters 30 --path fused"
for s in normal gradient metric; do
  echo "== $s, 30 iterations at the most"
  timeout -k 10 200 $exe $long --linearization $s --min-step 1e-5 > "$out/last.log" 2>&1 || { echo "run failed"; tail -5 "$out/last.log"; exit 1; }
  grep '^frame ' "$out/last.log" | tee "$out/frames_$s.txt"
  tail -1 "$out/last.log" | tee "$out/summary_$s.json"
done
echo "== normal, all 30 iterations"
timeout -k 10 200 $exe $long --linearization normal > "$out/last.log" 2>&1 || { echo "run failed"; tail -5 "$out/last.log"; exit 1; }
grep '^frame ' "$out/last.log" | tee "$out/frames_normal_all30.txt"
echo "== metric, huber 0.01, 30 iterations at the most"
timeout -k 10 200 $exe $long --linearization metric --huber 0.01 --min-step 1e-5 > "$out/last.log" 2>&1 || { echo "run failed"; tail -5 "$out/last.log"; exit 1; }
grep '^frame ' "$out/last.log" | tee "$out/frames_metric_huber.txt"
: > "$out/kernel_stats.csv"
d=$(mktemp -d)
echo "== metric (kernel trace)"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$d" -o run -- $exe $args --linearization metric > "$out/last.log" 2>&1 || { echo "run failed"; tail -5 "$out/last.log"; exit 1; }
f=$(find "$d" -name '*kernel_stats.csv' | head -1)
[ -n "$f" ] || { echo "no kernel stats written"; exit 1; }
echo "\"setting\",$(head -1 "$f")" >> "$out/kernel_stats.csv"
grep -E "k_volume_register|k_register_" "$f" | sed "s/^/\"metric\",/" | tee -a "$out/kernel_stats.csv"
rm -rf "$d"
