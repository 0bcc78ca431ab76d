#!/bin/bash
# kernel-trace passes only (forked + serial roles of the default workload, the batched TRACK leg): bash tools/profile_kernel_stats.sh TAG [BATCH]
TAG=${1:-r06_v3}; B=${2:-49152}
R=$(cd "$(dirname "$0")/.." && pwd); export OUT=${OUT:-prof_out}   # OUT: output folder, relative to the repository root
cd $R; export TMPDIR=/tmp; mkdir -p $OUT
python -c "import __graft_entry__ as g; g.build()"
for d in a s; do
  [ $d = s ] && export LIW_SERIAL_ROLES=1 || unset LIW_SERIAL_ROLES
  name=$([ $d = s ] && echo _serial_roles || echo "")
  timeout 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_$d -o $d -- python bench.py --full --batch $B --no-cpu-baseline --no-single --skip-sharded > $OUT/${TAG}_bench_b${B}${name}_under_rocprof.json 2> $OUT/prof_$d.err < /dev/null
  db=$(find $OUT/prof_$d -name "*.db" | head -1)
  [ -n "$db" ] && python tools/rocprof_summary.py $db $OUT/${TAG}_kernel_stats_b${B}${name}.csv > /dev/null
done
unset LIW_SERIAL_ROLES
cd /tmp
timeout 600 rocprofv3 --kernel-trace --stats -d $R/$OUT/prof_tk -o track -- python $R/tools/track_batch_probe.py $B 8 --no-cpu > /dev/null 2>&1
cd $R; db=$(find $OUT/prof_tk -name "*.db" | head -1); [ -n "$db" ] && python tools/rocprof_summary.py $db $OUT/${TAG}_track_batch_kernel_stats_b${B}.csv > /dev/null
rm -rf $OUT/prof_a $OUT/prof_s $OUT/prof_tk
python tools/ktimes.py $B > $OUT/${TAG}_ktimes.log 2>&1
ls -la $OUT | grep ${TAG}
