#!/bin/bash
# THE evidence pass of a round on the MI355X box (one gpurun call; usage: bash tools/profile_round.sh TAG [BATCH]):
#   1. SQ issue / MFMA counter passes (tools/pmc_stall_passes.sh; --pmc runs carry --kernel-trace only),
#   2. rocprofv3 --kernel-trace --stats of the bench command, role kernels forked and serial (LIW_SERIAL_ROLES=1) -> *_kernel_stats_*.csv,
#   3. FETCH_SIZE / WRITE_SIZE passes (separate runs) + per-kernel calibration (tools/pmc_traffic.py) -> profiles/pmc_traffic.json,
#   4. stand-alone kernel times (tools/ktimes.py), per-phase stamps of the quad step kernel, the staging micro-benchmark,
#   5. the default bench line LAST, with the traffic / issue statistics of this very build in place.
# Outputs under $OUT/${TAG}_*; copy what is to be judged into profiles/.
TAG=${1:-r05_v1}; B=${2:-49152}
R=$(cd "$(dirname "$0")/.." && pwd); export OUT=${OUT:-prof_out}   # OUT: output folder, relative to the repository root
cd $R; export TMPDIR=/tmp
mkdir -p $OUT
python -c "import __graft_entry__ as g; g.build()"
B=$B bash tools/pmc_stall_passes.sh > $OUT/${TAG}_stall.log 2>&1
cp $OUT/pmc_st.csv $OUT/${TAG}_pmc_wave_cycles_b${B}.csv; cp $OUT/pmc_st2.csv $OUT/${TAG}_pmc_mfma_b${B}.csv
for d in a s; do
  [ $d = s ] && export LIW_SERIAL_ROLES=1 || unset LIW_SERIAL_ROLES
  name=$([ $d = s ] && echo _serial_roles || echo "")
  timeout 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_$d -o $d -- python bench.py --full --batch $B --no-cpu-baseline --no-single --skip-sharded > $OUT/${TAG}_bench_b${B}${name}_under_rocprof.json 2> $OUT/prof_$d.err < /dev/null
  db=$(find $OUT/prof_$d -name "*.db" | head -1)
  [ -n "$db" ] && python tools/rocprof_summary.py $db $OUT/${TAG}_kernel_stats_b${B}${name}.csv > /dev/null
done
unset LIW_SERIAL_ROLES
timeout 600 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $OUT/prof_f --output-format csv -- python bench.py --batch $B --steps 1 --warmup 0 --no-cpu-baseline --no-single --skip-sharded > /dev/null 2> $OUT/prof_f.err < /dev/null
timeout 600 rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $OUT/prof_w --output-format csv -- python bench.py --batch $B --steps 1 --warmup 0 --no-cpu-baseline --no-single --skip-sharded > /dev/null 2> $OUT/prof_w.err < /dev/null
ff=$(find $OUT/prof_f -name "*counter_collection.csv" | head -1); fw=$(find $OUT/prof_w -name "*counter_collection.csv" | head -1)
[ -n "$ff" ] && cp $ff $OUT/${TAG}_pmc_fetch_size_b${B}.csv
[ -n "$fw" ] && cp $fw $OUT/${TAG}_pmc_write_size_b${B}.csv
cp profiles/pmc_traffic.json $OUT/${TAG}_pmc_traffic.json
[ -n "$ff" ] && [ -n "$fw" ] && python tools/pmc_traffic.py $OUT/${TAG}_pmc_fetch_size_b${B}.csv $OUT/${TAG}_pmc_write_size_b${B}.csv $B 30 2000 $OUT/${TAG}_pmc_traffic.json
[ -f $OUT/${TAG}_kernel_stats_b${B}_serial_roles.csv ] && python tools/serial_roles_frac.py $OUT/${TAG}_kernel_stats_b${B}_serial_roles.csv $OUT/${TAG}_bench_b${B}_serial_roles_under_rocprof.json $OUT/${TAG}_pmc_traffic.json
rm -rf $OUT/prof_a $OUT/prof_s $OUT/prof_f $OUT/prof_w
python tools/pmc_issue_stats.py $OUT/${TAG}_pmc_wave_cycles_b${B}.csv $OUT/${TAG}_pmc_mfma_b${B}.csv $OUT/${TAG}_pmc_traffic.json "$TAG" > $OUT/${TAG}_issue.log 2>&1
cp $OUT/${TAG}_pmc_traffic.json profiles/pmc_traffic.json
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 tools/ubench/dma_rate.hip -o tools/ubench/dma_rate 2> /dev/null && ./tools/ubench/dma_rate > $OUT/${TAG}_ubench_dma_rate.log 2>&1
python tools/ktimes.py $B > $OUT/${TAG}_ktimes.log 2>&1
LIW_NO_LASER_SLAB=1 python tools/ktimes.py $B >> $OUT/${TAG}_ktimes.log 2>&1
python tools/clk_probe_quad.py $B 100 15 3 > $OUT/${TAG}_quad_phases.log 2>&1
python tools/track_probe.py > $OUT/${TAG}_track_probe.log 2>&1
# the default bench line LAST, with the traffic / issue statistics of this very build in place
[ -z "$SKIP_BENCH" ] && python bench.py --full --batch $B > $OUT/${TAG}_bench_default.json 2> $OUT/${TAG}_bench_default.err < /dev/null
ls -la $OUT | grep ${TAG}
