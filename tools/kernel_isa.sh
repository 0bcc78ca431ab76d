#!/bin/bash
# device-only assembly of every HIP unit of the library, built with build.FLAGS (no GPU needed): run it on two trees and
# `diff -r` the two directories to show that a refactor left the device code as it was
# usage: tools/kernel_isa.sh OUTDIR [extra hipcc flags]
OUT=$1; shift
B=$(dirname "$0")/../2dliw-slam_amd
mkdir -p "$OUT" || exit 1
{ read -r FLAGS; read -r UNITS; } < <(python3 -c 'import runpy, sys; b = runpy.run_path(sys.argv[1])
print(" ".join(b["FLAGS"])); print(" ".join(s for s in b["SOURCES"] if s.endswith(".hip")))' "$B/build.py")
pids=()
for u in $UNITS; do   # (the path-dependent __hip_cuid_<hash> lines are left out)
  (set -o pipefail; /opt/rocm/bin/hipcc $FLAGS "$@" --cuda-device-only -S "$B/csrc/$u" -o - | grep -v __hip_cuid_ > "$OUT/${u%.hip}.s") & pids+=($!)
done
rc=0; for p in "${pids[@]}"; do wait "$p" || rc=1; done; exit $rc
