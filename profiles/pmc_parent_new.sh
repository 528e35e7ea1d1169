#!/bin/bash
# One counter pass each of two builds of librtr_hip.so, counters only (no tracing in the run):
#   bash profiles/pmc_parent_new.sh <parent librtr_hip.so> <output directory> [<counter> ...]
# default counters SQ_INSTS_VALU SQ_WAVE_CYCLES SQ_WAIT_ANY; the launches are the driver's (ten frames per launch, given explicitly:
# the latency probe would time launches under the profiler).  Per-kernel means of the queue build and the resolve -> <out>/pmc.log.
set -o pipefail
PARENT=$(realpath "$1"); OUT=$(realpath -m "$2"); shift 2
COUNTERS=${*:-SQ_INSTS_VALU SQ_WAVE_CYCLES SQ_WAIT_ANY}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
LIB=$ROOT/realtimeraytracer_amd/librtr_hip.so
mkdir -p "$OUT"
cp "$LIB" "$OUT/librtr_hip_new.so"
restore() { cp "$OUT/librtr_hip_new.so" "$LIB"; rm -f "$OUT/librtr_hip_new.so"; }
trap restore EXIT
cd "$ROOT"
: > "$OUT/pmc.log"
for build in parent new; do
    if [ "$build" = parent ]; then cp "$PARENT" "$LIB"; else cp "$OUT/librtr_hip_new.so" "$LIB"; fi
    timeout -k 10 300 rocprofv3 --pmc $COUNTERS --output-format csv -d "$OUT/pass_$build" -- python bench.py --gpus 1 --steps 20 --warmup 5 --batch 10 --no-cpu-baseline --isolated-frames 0 --present-frames 0 \
        > "$OUT/bench_pmc_$build.out" 2> "$OUT/rocprof_$build.err" || { echo "pass $build failed ($?)"; tail -5 "$OUT/rocprof_$build.err"; exit 1; }
    python - "$OUT/pass_$build" "$build" <<'PY' | tee -a "$OUT/pmc.log"
import csv, glob, os, sys
from collections import defaultdict
agg = defaultdict(lambda: defaultdict(list))
for f in glob.glob(os.path.join(sys.argv[1], "**", "*counter_collection.csv"), recursive=True):
    for row in csv.DictReader(open(f)):
        agg[row["Kernel_Name"]][row["Counter_Name"]].append(float(row["Counter_Value"] or 0))
for k in sorted(agg):
    if "k_shadow_gen_oct" not in k and "k_resolve_compact" not in k:
        continue
    print(f"[{sys.argv[2]}] " + k.split("(")[0].replace("void ", "") + "  " + "  ".join(f"{c}={sum(v) / len(v):.0f} (n={len(v)})" for c, v in sorted(agg[k].items())))
PY
    rm -rf "$OUT/pass_$build"
done
