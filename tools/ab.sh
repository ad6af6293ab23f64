#!/bin/bash
# A/B builds of the library in ONE GPU call (machines differ by several %), three rounds interleaved:  tools/ab.sh NAME_A NAME_B ...
# Build the variants first:  tools/ab_build.sh NAME "<flags>"      Another workload than the headline's:  AB_WORKLOAD=interp_t04_64k AB_STEPS=3 AB_WARMUP=1 tools/ab.sh A B
# Stops at the first run that fails (its exit status is this script's): nothing more is started on the GPU after a fault.
set -e -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); cd "$R"
out=$(mktemp)
trap 'rm -f "$out"' EXIT
for round in 1 2 3; do
  for v in "$@"; do
    rc=0
    SRT_LIB_OVERRIDE=$R/stanford_raytracer_amd/lib/libsrt_hip_$v.so timeout -k 10 300 python bench.py --steps ${AB_STEPS:-20} --warmup ${AB_WARMUP:-5} --cpu-seconds 0 --damping-rays 0 --traffic off --other-configs 0 ${AB_WORKLOAD:+--workload $AB_WORKLOAD} > "$out" 2>/dev/null || rc=$?
    if [ $rc -ne 0 ]; then echo "$v round $round: bench.py exited with status $rc -- stopping" >&2; exit $rc; fi
    python -c "import sys,json; d=json.loads(open(sys.argv[1]).readlines()[-1]); print('$v', 'round $round', 'kernel_ms', round(d['roofline']['kernel_ms'],2), 'steps/s %.4g' % d['value'], int(d['roofline']['accepted_steps_per_launch']), d['detail'].get('rows_checksum'))" "$out"
  done
done
