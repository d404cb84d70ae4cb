#!/bin/bash
# profile_volume_register_volume.sh OUT_DIR [STAGES] [PARENT_EXE] -- the measurements behind profiles/volume_register_volume_times.json (DESIGN.md
# section 3.8).  STAGES is a list of the stages to run (default "paths color_off sweeps trace"; "parent" needs PARENT_EXE):
#   paths      examples/cpp/SubmapAlignment.bin --synthetic 200 5 1 --submaps 4 --res 0.005 --perturb 20, one run per path (cloud, mesh, volume): a
#              fresh process per run, the paths alternating, one untimed pass of each and five timed ones; the last line (JSON) of every timed run in
#              OUT_DIR/times.jsonl, tagged with its setting
#   color_off  the same three paths with --color off, one run each (OUT_DIR/sweeps.jsonl)
#   sweeps     the volume path with the band at 1, 2, 4 voxels and the truncation, and with --voxel-stride 2, with and without the colour term, one
#              run each (OUT_DIR/sweeps.jsonl)
#   parent     examples/cpp/ModelRegistration.bin --synthetic 200 5 1 --res 0.005 --perturb 20 --iters 10 --path fused --linearization metric on this
#              tree and PARENT_EXE -- the same driver built from the commit before this feature -- alternating, one untimed pass and five timed
#              ones (OUT_DIR/parent.jsonl): what the new template parameter costs the existing instantiations
#   trace      the volume path under the kernel tracer, in a run of its own; the k_volume_register / k_register_fold / k_band_voxels rows in
#              OUT_DIR/kernel_stats.csv
# Every run has its own time limit and the first failure ends the script.  Run from the repository root after __graft_entry__.build().
out=${1:?usage: profile_volume_register_volume.sh OUT_DIR [STAGES] [PARENT_EXE]}
stages=${2:-paths color_off sweeps trace}
parent=$3
mkdir -p "$out"
exe=examples/cpp/SubmapAlignment.bin
args="--synthetic 200 5 1 --submaps 4 --res 0.005 --perturb 20"
run() { # run TAG FILE LIMIT command...: the command's last line into FILE, tagged
  local tag=$1 file=$2 limit=$3
  shift 3
  timeout -k 10 "$limit" "$@" > "$out/last.log" 2>&1 || { echo "run failed: $*"; tail -5 "$out/last.log"; exit 1; }
  grep '^submap ' "$out/last.log"
  [ -n "$file" ] && echo "{\"setting\": \"$tag\", \"run\": $(tail -1 "$out/last.log")}" | tee -a "$out/$file"
  return 0
}
for stage in $stages; do
  case $stage in
    paths)
      : > "$out/times.jsonl"
      for pass in 0 1 2 3 4 5; do
        for p in cloud mesh volume; do
          echo "== pass $pass $p"
          if [ $pass -gt 0 ]; then run "$p" times.jsonl 280 $exe $args --path $p; else run "$p" "" 280 $exe $args --path $p; fi
        done
      done ;;
    color_off)
      for p in cloud mesh volume; do
        echo "== $p, --color off"
        run "$p color off" sweeps.jsonl 280 $exe $args --path $p --color off
      done ;;
    sweeps)
      for c in on off; do
        for b in 0.005 0.01 0.02 -1; do
          echo "== volume, band $b, --color $c"
          run "volume band $b color $c" sweeps.jsonl 280 $exe $args --path volume --band $b --color $c
        done
        echo "== volume, stride 2, --color $c"
        run "volume stride 2 color $c" sweeps.jsonl 280 $exe $args --path volume --voxel-stride 2 --color $c
      done ;;
    parent)
      [ -n "$parent" ] || { echo "the parent stage needs PARENT_EXE"; exit 1; }
      : > "$out/parent.jsonl"
      margs="--synthetic 200 5 1 --res 0.005 --perturb 20 --iters 10 --path fused --linearization metric"
      for pass in 0 1 2 3 4 5; do
        for s in parent new; do
          echo "== pass $pass $s"
          if [ $s = parent ]; then cmd="$parent $margs"; else cmd="examples/cpp/ModelRegistration.bin $margs"; fi
          if [ $pass -gt 0 ]; then run "$s" parent.jsonl 200 $cmd; else run "$s" "" 200 $cmd; fi
        done
      done ;;
    trace)
      : > "$out/kernel_stats.csv"
      d=$(mktemp -d)
      echo "== volume (kernel trace)"
      timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$d" -o run -- $exe $args --path volume > "$out/last.log" 2>&1 || { echo "run failed"; tail -5 "$out/last.log"; exit 1; }
      f=$(find "$d" -name '*kernel_stats.csv' | head -1)
      [ -n "$f" ] || { echo "no kernel stats written"; exit 1; }
      head -1 "$f" >> "$out/kernel_stats.csv"
      grep -E "k_volume_register|k_register_|k_band_voxels" "$f" | tee -a "$out/kernel_stats.csv"
      tail -1 "$out/last.log" > "$out/trace_run.json"
      rm -rf "$d" ;;
    *) echo "unknown stage $stage"; exit 1 ;;
  esac
done
