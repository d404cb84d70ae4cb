#!/bin/bash
# Needs an MI355X: what profiles/collect_garbage_times.json and profiles/collect_garbage_kernel_stats.csv hold.
#   tools/profile_collect_garbage.sh OUT_DIR
#   1. examples/cpp/PoseCorrection.bin --synthetic 200 5 1 --perturb K --res 0.005 --runs 5 --collect none|device|roundtrip for K = 20 and 100:
#      a fresh process per setting, one untimed pass and five timed ones (the driver's medians), one JSON line each
#   2. device and roundtrip dump equal volumes (a smaller volume: the dumps are whole pools)
#   3. rocprofv3 --kernel-trace --stats of the device setting
# Every step has its own time limit and the script stops at the first step that fails.
set -e -o pipefail
REPO=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mkdir -p "${1:?usage: profile_collect_garbage.sh OUT_DIR}" && cd "$1" && pwd)
BIN=$REPO/examples/cpp/PoseCorrection.bin
mkdir -p $OUT
export TMPDIR=/tmp
: > $OUT/collect_garbage_lines.json
for K in 20 100; do
    for C in none device roundtrip; do
        timeout -k 10 240 $BIN --synthetic 200 5 1 --perturb $K --res 0.005 --runs 5 --collect $C | tail -1 >> $OUT/collect_garbage_lines.json
    done
done
cat $OUT/collect_garbage_lines.json
D=$(mktemp -d /tmp/collect_dump.XXXXXX)
timeout -k 10 120 $BIN --synthetic 40 5 1 --perturb 8 --res 0.02 --collect device --dump $D/device.bin | tail -1
timeout -k 10 120 $BIN --synthetic 40 5 1 --perturb 8 --res 0.02 --collect roundtrip --dump $D/roundtrip.bin | tail -1
cmp $D/device.bin $D/roundtrip.bin && echo "dumps equal: $(stat -c %s $D/device.bin) bytes" | tee $OUT/collect_garbage_dumps.txt
rm -rf $D
rm -rf /tmp/prof_collect
cd /tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_collect -o collect -- $BIN --synthetic 200 5 1 --perturb 20 --res 0.005 --runs 5 --collect device > $OUT/collect_garbage_prof.log 2>&1
find /tmp/prof_collect -name "*kernel_stats.csv" -exec cp {} $OUT/collect_garbage_kernel_stats.csv \;
rm -rf /tmp/prof_collect
head -20 $OUT/collect_garbage_kernel_stats.csv
