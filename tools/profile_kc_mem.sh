#!/bin/bash
# Runs ON THE GPU BOX: the vector-memory side of k_integrate (texture addresser, vector L1, wait cycles) with the torch-free driver: 96 bench frames,
# three 32-frame launches.  Counters-only passes (rocprofv3 --pmc and no tracing option), one counter block per pass; a counter the device does
# not list is left out.  usage: [TAG=name] [OUT=<output directory>] [KC_LIB_DIR=<directory of another libonepiece_hip.so>] bash tools/profile_kc_mem.sh
R=$(cd "$(dirname "$0")/.." && pwd)
TAG=${TAG:-tree}
OUT=${OUT:-/tmp/kc_mem}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
[ -n "$KC_LIB_DIR" ] && export LD_LIBRARY_PATH=$KC_LIB_DIR:$LD_LIBRARY_PATH
[ -f /tmp/frames96.bin ] || python $R/tools/dump_frames.py /tmp/frames96.bin 96 0 > /dev/null || exit 1
[ -f /tmp/kc_mem_avail.txt ] || rocprofv3 --list-avail > /tmp/kc_mem_avail.txt 2>&1
P=0
for C in "TA_BUSY_avr TA_BUFFER_READ_WAVEFRONTS_sum" "TCP_TOTAL_CACHE_ACCESSES_sum TCP_TCC_READ_REQ_sum TCP_PENDING_STALL_CYCLES_sum" \
         "SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_VMEM SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_INSTS_VALU SQ_INSTS_VMEM_RD SQ_INSTS_SALU"; do
  P=$((P + 1)); L=""
  # (without a usable listing every counter is tried)
  for c in $C; do if grep -qw $c /tmp/kc_mem_avail.txt || ! grep -qw SQ_WAVES /tmp/kc_mem_avail.txt; then L="$L $c"; else echo "$TAG: the device does not list $c"; fi; done
  [ -n "$L" ] || continue
  rm -rf /tmp/kcm_${TAG}_$P
  timeout -k 10 240 rocprofv3 --pmc $L --output-format csv -d /tmp/kcm_${TAG}_$P -o p -- $R/tools/prof_driver.bin /tmp/frames96.bin 1 > $OUT/${TAG}_pass$P.log 2>&1
  E=$?
  if [ $E -ne 0 ]; then echo "$TAG pass $P [$L]: exit $E"; tail -3 $OUT/${TAG}_pass$P.log; fi
  if [ $E -ge 124 ]; then exit $E; fi   # a time limit, an abort or a fault: nothing more is started on the device
  python $R/tools/pmc_summary.py /tmp/kcm_${TAG}_$P $OUT/${TAG}_pass$P
done
grep -h k_integrate $OUT/${TAG}_pass*.pmc.csv
