#!/bin/bash
# Final check of a round (GPU box): the whole -m gpu suite, smoke(), the default bench line with its CPU legs and parity
# gate (--full).  Usage: tools/gpu_final_check.sh OUT_DIR (logs and the bench line are written there).
set -o pipefail
O=${1:?usage: tools/gpu_final_check.sh OUT_DIR}
mkdir -p "$O"
timeout -k 10 900 python -m pytest tests -m gpu -q > "$O/final_gpu_tests.log" 2>&1; rc=$?
tail -5 "$O/final_gpu_tests.log"
[ $rc -eq 0 ] || exit $rc
python -c "import __graft_entry__ as g; g.smoke()" || exit 1
timeout -k 10 400 python3 bench.py --full > "$O/final_bench.json" 2> "$O/final_bench.err"; echo "bench rc=$?"
python3 - "$O/final_bench.json" <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print("ms/step %.4f value %.4g k1 %.4f frac %.3f parity %s cpu %.3g" % (d["ms_per_step"], d["value"], d["roofline"]["kernel_ms"], d["roofline"]["frac"], d["parity"]["ok"], d["cpu_baseline"]["value"]))
PY
