#!/bin/bash
# a state's measurements in one call -- the full bench line (default flags, and the driver's --steps 20 --warmup 5), rocprofv3 kernel statistics of
# the resident steps, the PMC passes, the kernels alone.  usage: bash tools/measure_state.sh <tag> [folder for the results, default measure_out]
TAG=${1:-r06a}
cd "$(dirname "$0")/.."; OUT=${2:-measure_out}; mkdir -p "$OUT"
timeout -k 10 900 python bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err; echo "bench rc $?"
timeout -k 10 600 python bench.py --full --steps 20 --warmup 5 > $OUT/${TAG}_bench_driver_flags.json 2> $OUT/${TAG}_bench_driver_flags.err; echo "bench (driver flags) rc $?"
bash tools/gpu_kstats.sh $TAG > $OUT/${TAG}_kstats.txt 2>&1; echo "kstats rc $?"
bash tools/gpu_pmc.sh $TAG > $OUT/${TAG}_pmc.txt 2>&1; echo "pmc rc $?"
bash tools/kb.sh --no-overlap > $OUT/${TAG}_kernels_alone.txt 2>&1; echo "alone rc $?"
python - <<PY
import json
for f in ("$OUT/${TAG}_bench.json", "$OUT/${TAG}_bench_driver_flags.json"):
    d = json.loads(open(f).read().strip().splitlines()[-1])
    print(f, {k: d.get(k) for k in ("value", "value_min", "value_max", "ms_per_step", "dominant_kernel_ms", "sustained_frames_per_s", "step_hbm_bytes", "facade_ms_per_file", "c_call_ms_per_file", "first_call_ms", "decode_only_float32_exact_ms", "decode_only_int16_ms", "parity_checked")}, d["roofline"]["frac"], d["roofline_alu"])
PY
