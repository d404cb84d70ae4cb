#!/bin/bash
# profile_volume_merge_transformed.sh OUT_DIR [STAGES] [PARENT_EXE] -- the measurements behind profiles/volume_merge_transformed_times.json (DESIGN.md
# section 3.11).  Every stage runs examples/cpp/SubmapAlignment.bin --synthetic 200 5 1 --submaps 4 --res 0.005 --perturb 20 --path volume (the setting
# of profiles/volume_register_volume_times.json), a fresh process per run.  STAGES (default "merge recompose trace"; "merge" and "trace" take the
# parent's rows only with PARENT_EXE, the same driver built from the commit before this feature):
#   merge      PARENT_EXE, --merge two-step and --merge fused alternating, one untimed pass of each and five timed ones; the last line (JSON) of
#              every timed run in OUT_DIR/merge.jsonl, tagged parent / two-step / fused: merge_ms per submap is what is compared
#   recompose  --merge fused with --recompose single and --recompose batch alternating, one untimed pass and three timed ones (OUT_DIR/recompose.jsonl):
#              recompose_ms, all four submaps into a fresh model by four calls or by one
#   trace      under the kernel tracer, each in a run of its own: --merge fused (the three merges' k_merge_claim / k_merge_fill calls:
#              OUT_DIR/kernel_stats_fused.csv), --merge two-step --recompose batch (there the two kernels' single calls are the re-composition's:
#              _recompose.csv) and PARENT_EXE (k_transform_alloc, k_transform_fill_wave, k_insert_keys, k_merge_blocks: _parent.csv)
# Every run has its own time limit and the first failure ends the script.  Run from the repository root after __graft_entry__.build().
out=${1:?usage: profile_volume_merge_transformed.sh OUT_DIR [STAGES] [PARENT_EXE]}
stages=${2:-merge recompose trace}
parent=$3
mkdir -p "$out"
exe=examples/cpp/SubmapAlignment.bin
args="--synthetic 200 5 1 --submaps 4 --res 0.005 --perturb 20 --path volume"
run() { # run TAG FILE LIMIT command...: the command's last line into FILE, tagged
  local tag=$1 file=$2 limit=$3
  shift 3
  timeout -k 10 "$limit" "$@" > "$out/last.log" 2>&1 || { echo "run failed: $*"; tail -5 "$out/last.log"; exit 1; }
  grep -E '^(submap|recompose) ' "$out/last.log"
  [ -n "$file" ] && echo "{\"setting\": \"$tag\", \"run\": $(tail -1 "$out/last.log")}" >> "$out/$file"
  return 0
}
trace() { # trace NAME command...: the merge kernels' rows of one traced run
  local name=$1
  shift
  local d
  d=$(mktemp -d)
  timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$d" -o run -- "$@" > "$out/last.log" 2>&1 || { echo "run failed"; tail -5 "$out/last.log"; exit 1; }
  local f
  f=$(find "$d" -name '*kernel_stats.csv' | head -1)
  [ -n "$f" ] || { echo "no kernel stats written"; exit 1; }
  head -1 "$f" > "$out/kernel_stats_$name.csv"
  grep -E "k_merge_claim|k_merge_fill|k_transform_alloc|k_transform_fill_wave|k_insert_keys|k_merge_blocks" "$f" | tee -a "$out/kernel_stats_$name.csv"
  tail -1 "$out/last.log" > "$out/trace_run_$name.json"
  rm -rf "$d"
}
for stage in $stages; do
  case $stage in
    merge)
      : > "$out/merge.jsonl"
      for pass in 0 1 2 3 4 5; do
        for s in parent two-step fused; do
          if [ $s = parent ]; then
            [ -n "$parent" ] || continue
            cmd="$parent $args"
          else
            cmd="$exe $args --merge $s"
          fi
          echo "== pass $pass $s"
          if [ $pass -gt 0 ]; then run "$s" merge.jsonl 280 $cmd; else run "$s" "" 280 $cmd; fi
        done
      done ;;
    recompose)
      : > "$out/recompose.jsonl"
      for pass in 0 1 2 3; do
        for s in single batch; do
          echo "== pass $pass recompose $s"
          if [ $pass -gt 0 ]; then run "$s" recompose.jsonl 280 $exe $args --merge fused --recompose $s; else run "$s" "" 280 $exe $args --merge fused --recompose $s; fi
        done
      done ;;
    trace)
      echo "== fused (kernel trace)"
      trace fused $exe $args --merge fused
      echo "== two-step + recompose batch (kernel trace)"
      trace recompose $exe $args --merge two-step --recompose batch
      if [ -n "$parent" ]; then
        echo "== parent (kernel trace)"
        trace parent $parent $args
      fi ;;
    *) echo "unknown stage $stage"; exit 1 ;;
  esac
done
