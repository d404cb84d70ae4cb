#!/bin/bash
# profile_volume_register_color.sh OUT_DIR [PARENT_EXE] -- the measurements behind profiles/volume_register_color_times.json:
#   1. examples/cpp/ModelRegistration.bin --synthetic 200 5 1 --res 0.005 --perturb 20 --iters 10 --path fused --color off|on: a fresh process per run,
#      the settings alternating, one untimed pass of each and five timed ones; the last line (JSON) of every timed run in OUT_DIR/times.jsonl, tagged
#      with its setting.  With PARENT_EXE -- a ModelRegistration.bin built from the commit before the colour term, which knows no --color -- the same
#      command without the flag takes its turn in every pass ("parent"): what `--color off` must cost, and the spread of its own repeats
#   2. the per-frame lines of one `--color on` run and of one `--color on --color-scale 0` run (the geometric registration through the rgbd entry) in
#      OUT_DIR/frames_on.txt and OUT_DIR/frames_geometric.txt
#   3. `--color on` under the kernel tracer, in a run of its own; the k_volume_register / k_register_fold rows in OUT_DIR/kernel_stats.csv, and
#      `--color off` likewise
# Every run has its own time limit and the first failure ends the script.  Run from the repository root after __graft_entry__.build().
out=${1:?usage: profile_volume_register_color.sh OUT_DIR [PARENT_EXE]}
parent=$2
mkdir -p "$out"
exe=examples/cpp/ModelRegistration.bin
args="--synthetic 200 5 1 --res 0.005 --perturb 20 --iters 10 --path fused"
settings="off on"
[ -n "$parent" ] && settings="parent off on"
: > "$out/times.jsonl"
for pass in 0 1 2 3 4 5; do
  for s in $settings; do
    echo "== pass $pass $s"
    if [ "$s" = parent ]; then cmd="$parent $args"; else cmd="$exe $args --color $s"; fi
    timeout -k 10 200 $cmd > "$out/last.log" 2>&1 || { echo "run failed"; tail -5 "$out/last.log"; exit 1; }
    if [ $pass -gt 0 ]; then echo "{\"setting\": \"$s\", \"run\": $(tail -1 "$out/last.log")}" | tee -a "$out/times.jsonl"; fi
    if [ $pass -eq 5 ] && [ "$s" = on ]; then grep '^frame ' "$out/last.log" > "$out/frames_on.txt"; fi
  done
done
timeout -k 10 200 $exe $args --color on --color-scale 0 > "$out/last.log" 2>&1 || { echo "run failed"; tail -5 "$out/last.log"; exit 1; }
grep '^frame ' "$out/last.log" | tee "$out/frames_geometric.txt"
cat "$out/frames_on.txt"
: > "$out/kernel_stats.csv"
for s in on off; do
  d=$(mktemp -d)
  echo "== $s (kernel trace)"
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$d" -o run -- $exe $args --color $s > "$out/last.log" 2>&1 || { echo "run failed"; tail -5 "$out/last.log"; exit 1; }
  f=$(find "$d" -name '*kernel_stats.csv' | head -1)
  [ -n "$f" ] || { echo "no kernel stats written"; exit 1; }
  [ -s "$out/kernel_stats.csv" ] || echo "\"setting\",$(head -1 "$f")" >> "$out/kernel_stats.csv"
  grep -E "k_volume_register|k_register_" "$f" | sed "s/^/\"$s\",/" | tee -a "$out/kernel_stats.csv"
  rm -rf "$d"
done
