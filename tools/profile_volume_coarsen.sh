#!/bin/bash
# profile_volume_coarsen.sh OUT_DIR [lod|trace|register|all] -- the measurements behind profiles/volume_coarsen_times.json:
#   lod       examples/cpp/ModelLod.bin --synthetic 200 5 1 --res 0.005 --levels 2, --path device against --path host: a fresh process per run, the
#             two paths alternating, one untimed pass of each and five timed ones; the JSON line of every level of every timed run in
#             OUT_DIR/times.jsonl (per level: blocks, counts, the coarsening's time, triangles, extraction and render times, the fidelity figures)
#   trace     the device path under the kernel tracer, in a run of its own (--warmup 1 --repeat 5: six coarsenings per level); the k_coarsen_* rows
#             in OUT_DIR/kernel_stats.csv
#   register  examples/cpp/ModelRegistration.bin --synthetic 200 5 1 --res 0.005 --path fused at --coarse 0, 1 and 2, alternating, one untimed pass
#             and five timed ones; the JSON line of every timed run in OUT_DIR/register.jsonl.  With PARENT_EXE set to a ModelRegistration.bin built
#             from the parent commit, that binary joins the alternation (without --coarse) as "parent"
# Every run has its own time limit and the first failure ends the script.  Run from the repository root after __graft_entry__.build().
out=${1:?usage: profile_volume_coarsen.sh OUT_DIR [lod|trace|register|all]}
what=${2:-all}
mkdir -p "$out"
lod=examples/cpp/ModelLod.bin
reg=examples/cpp/ModelRegistration.bin
args="--synthetic 200 5 1 --res 0.005"
if [ "$what" = lod ] || [ "$what" = all ]; then
  : > "$out/times.jsonl"
  for pass in 0 1 2 3 4 5; do
    for path in device host; do
      echo "== lod pass $pass $path"
      timeout -k 10 300 $lod $args --levels 2 --path $path > "$out/last.log" 2>&1 || { echo "run failed"; tail -5 "$out/last.log"; exit 1; }
      if [ $pass -gt 0 ]; then grep '^{' "$out/last.log" | sed "s/^{/{\"pass\": $pass, /" | tee -a "$out/times.jsonl"; fi
    done
  done
fi
if [ "$what" = trace ] || [ "$what" = all ]; then
  : > "$out/kernel_stats.csv"
  d=$(mktemp -d)
  echo "== device path (kernel trace)"
  timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$d" -o run -- $lod $args --levels 2 --path device --warmup 1 --repeat 5 > "$out/last.log" 2>&1 || { echo "run failed"; tail -5 "$out/last.log"; exit 1; }
  f=$(find "$d" -name '*kernel_stats.csv' | head -1)
  [ -n "$f" ] || { echo "no kernel stats written"; exit 1; }
  head -1 "$f" >> "$out/kernel_stats.csv"
  grep -E "k_coarsen_" "$f" | tee -a "$out/kernel_stats.csv"
  t=$(find "$d" -name '*kernel_trace.csv' | head -1)
  if [ -n "$t" ]; then head -1 "$t" > "$out/kernel_trace_coarsen.csv"; grep -E "k_coarsen_" "$t" >> "$out/kernel_trace_coarsen.csv"; fi
  grep '^{' "$out/last.log" | tee "$out/trace_run.jsonl"
  rm -rf "$d"
fi
if [ "$what" = register ] || [ "$what" = all ]; then
  : > "$out/register.jsonl"
  for pass in 0 1 2 3 4 5; do
    for mode in 0 parent 1 2; do
      if [ $mode = parent ]; then
        [ -n "$PARENT_EXE" ] || continue
        cmd="$PARENT_EXE $args --path fused"
      elif [ $mode = 0 ]; then cmd="$reg $args --path fused"
      else cmd="$reg $args --path fused --coarse $mode"; fi
      echo "== register pass $pass $mode"
      timeout -k 10 300 $cmd > "$out/last.log" 2>&1 || { echo "run failed"; tail -5 "$out/last.log"; exit 1; }
      if [ $pass -gt 0 ]; then echo "{\"mode\": \"$mode\", \"pass\": $pass, \"run\": $(grep '^{' "$out/last.log" | tail -1)}" | tee -a "$out/register.jsonl"; fi
    done
  done
fi
