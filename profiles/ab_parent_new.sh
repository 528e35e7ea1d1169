#!/bin/bash
# Alternating A/B of two builds of librtr_hip.so on one box, in one session:
#   bash profiles/ab_parent_new.sh <parent librtr_hip.so> <output directory>        (profiles/build_variant.sh builds a parent)
# Three rounds of `bench.py --gpus 1 --steps 20 --warmup 5` and three of `bench.py --gpus 1` (192 steps), parent and new alternating,
# every run a process of its own under its own time limit; then one --dump-outputs run of the 20-step command per build and the
# comparison of the two framebuffers.  A run that fails ends the script (the working tree's library is put back first).
set -o pipefail
PARENT=$(realpath "$1"); OUT=$(realpath -m "$2")
ROOT=$(cd "$(dirname "$0")/.." && pwd)
LIB=$ROOT/realtimeraytracer_amd/librtr_hip.so
mkdir -p "$OUT"
cp "$LIB" "$OUT/librtr_hip_new.so"
restore() { cp "$OUT/librtr_hip_new.so" "$LIB"; rm -f "$OUT/librtr_hip_new.so"; }
trap restore EXIT
cd "$ROOT"
run() {      # run <tag> <build> <bench arguments>
    local tag=$1 build=$2; shift 2
    if [ "$build" = parent ]; then cp "$PARENT" "$LIB"; else cp "$OUT/librtr_hip_new.so" "$LIB"; fi
    timeout -k 10 240 python bench.py "$@" > "$OUT/bench_${tag}_${build}.out" 2> "$OUT/bench_${tag}_${build}.err" || { echo "[$tag] $build : bench.py failed ($?)"; tail -5 "$OUT/bench_${tag}_${build}.err"; return 1; }
    python - "$OUT/bench_${tag}_${build}.out" "$tag" "$build" <<'PY' | tee -a "$OUT/ab.log"
import json, sys
j = json.loads(open(sys.argv[1]).readlines()[-1])
k = j.get("kernels_ms_in_flight_event_brackets") or j.get("kernels_ms") or {}      # ms per frame, event brackets of the launches in flight
print(f"[{sys.argv[2]}] {sys.argv[3]} : ms_per_step {j.get('ms_per_step')} frames_per_launch {j.get('frames_per_launch')} shadow_gen {k.get('shadow_gen')} resolve {k.get('resolve')} kernels {json.dumps(k)} value {j.get('value')}")
PY
}
: > "$OUT/ab.log"
for r in 1 2 3; do
    run steps20_r$r parent --gpus 1 --steps 20 --warmup 5 && run steps20_r$r new --gpus 1 --steps 20 --warmup 5 || exit 1
done
for r in 1 2 3; do
    run default_r$r parent --gpus 1 && run default_r$r new --gpus 1 || exit 1
done
run dump parent --gpus 1 --steps 20 --warmup 5 --dump-outputs "$OUT/dump_parent" && run dump new --gpus 1 --steps 20 --warmup 5 --dump-outputs "$OUT/dump_new" || exit 1
python - "$OUT" <<'PY' | tee -a "$OUT/ab.log"
import sys
import numpy as np
a, b = (np.load(f"{sys.argv[1]}/dump_{w}/framebuffer_rgba8.npy") for w in ("parent", "new"))
print("framebuffer_rgba8 parent vs new", "equal" if a.shape == b.shape and np.array_equal(a, b) else f"DIFFERENT ({int((a != b).sum())} bytes)", a.shape)
PY
rm -rf "$OUT/dump_parent" "$OUT/dump_new"
