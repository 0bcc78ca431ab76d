#!/bin/bash
# Round-6 evidence pass (one gpurun call): bash tools/profile_round6.sh TAG
#   1. tools/profile_round.sh TAG (C2: SQ issue / MFMA passes, kernel trace forked + serial roles, FETCH_SIZE / WRITE_SIZE -> profiles/pmc_traffic.json,
#      stand-alone kernel times, quad phases, tracking frame probe; its bench line is skipped here),
#   2. the batched TRACK leg: kernel trace + FETCH_SIZE / WRITE_SIZE passes of tools/track_batch_probe.py -> pmc_track.json,
#   3. the ragged leg (tools/ragged_probe.py), 4. the default bench line LAST.
TAG=${1:-r06_v1}; B=${2:-49152}
R=$(cd "$(dirname "$0")/.." && pwd); export OUT=${OUT:-prof_out}   # OUT: output folder, relative to the repository root
cd $R; export TMPDIR=/tmp; mkdir -p $OUT
SKIP_BENCH=1 bash tools/profile_round.sh $TAG $B > $OUT/${TAG}_profile_round.log 2>&1
cd /tmp
timeout 600 rocprofv3 --kernel-trace --stats -d $R/$OUT/prof_tk -o track -- python $R/tools/track_batch_probe.py $B 8 --no-cpu > $R/$OUT/${TAG}_track_batch_under_rocprof.json 2> /dev/null
timeout 600 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $R/$OUT/prof_tf --output-format csv -- python $R/tools/track_batch_probe.py $B 4 --no-cpu > /dev/null 2>&1
timeout 600 rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $R/$OUT/prof_tw --output-format csv -- python $R/tools/track_batch_probe.py $B 4 --no-cpu > /dev/null 2>&1
cd $R
db=$(find $OUT/prof_tk -name "*.db" | head -1); [ -n "$db" ] && python tools/rocprof_summary.py $db $OUT/${TAG}_track_batch_kernel_stats_b${B}.csv > /dev/null
ff=$(find $OUT/prof_tf -name "*counter_collection.csv" | head -1); fw=$(find $OUT/prof_tw -name "*counter_collection.csv" | head -1)
[ -n "$ff" ] && cp $ff $OUT/${TAG}_track_pmc_fetch_size_b${B}.csv; [ -n "$fw" ] && cp $fw $OUT/${TAG}_track_pmc_write_size_b${B}.csv
[ -n "$ff" ] && [ -n "$fw" ] && python tools/pmc_track.py $ff $fw $B $OUT/${TAG}_pmc_track.json > $OUT/${TAG}_pmc_track.log 2>&1 && cp $OUT/${TAG}_pmc_track.json profiles/pmc_track.json
rm -rf $OUT/prof_tk $OUT/prof_tf $OUT/prof_tw
python tools/track_batch_probe.py $B 8 > $OUT/${TAG}_track_batch_probe.json 2> /dev/null
python tools/ragged_probe.py $B > $OUT/${TAG}_ragged_probe.json 2> /dev/null
python bench.py --full --batch $B > $OUT/${TAG}_bench_default.json 2> $OUT/${TAG}_bench_default.err < /dev/null
ls -la $OUT | grep ${TAG}
