#!/bin/bash
# Round 4, first GPU call: the whole -m gpu suite, the plain `bench.py --gpus 2` self-launch on ONE card (gloo rehearsal:
# throughput meaningless, the flow is what is checked) for cfg3 and cfg5, then the default bench line with its parity gate
# (--full).  Usage: tools/gpu_round4_check.sh OUT_DIR (logs and bench lines are written there).
set -o pipefail
O=${1:?usage: tools/gpu_round4_check.sh OUT_DIR}
mkdir -p "$O"
timeout -k 10 700 python -m pytest tests -m gpu -x -q > "$O/r4_gpu_tests.log" 2>&1 || { tail -30 "$O/r4_gpu_tests.log"; exit 1; }
tail -3 "$O/r4_gpu_tests.log"
NFOPP_DIST_BACKEND=gloo timeout -k 10 300 python3 bench.py --gpus 2 --batch-per-gpu 1024 --cpu-sample 0 --steps 20 --warmup 3 --fit-iters 20 > "$O/r4_bench_2rank_cfg3.json" 2> "$O/r4_bench_2rank_cfg3.err" || { tail -20 "$O/r4_bench_2rank_cfg3.err"; exit 1; }
NFOPP_DIST_BACKEND=gloo timeout -k 10 300 python3 bench.py --gpus 2 --batch-per-gpu 1024 --cpu-sample 0 --steps 10 --warmup 2 --fit-iters 20 --workload cfg5 --spin-up 5 > "$O/r4_bench_2rank_cfg5.json" 2> "$O/r4_bench_2rank_cfg5.err" || { tail -20 "$O/r4_bench_2rank_cfg5.err"; exit 1; }
python3 - "$O" <<'PY'
import json, os, sys
for w in ("cfg3", "cfg5"):
    d = json.loads(open(os.path.join(sys.argv[1], "r4_bench_2rank_%s.json" % w)).read().strip().splitlines()[-1])
    print(w, "n_gpus", d["n_gpus"], "ranks_seen", d["ranks_seen"], d["backend"], "finite", d["config"]["paths_finite"])
PY
timeout -k 10 400 python3 bench.py --full > "$O/r4_bench_cfg3.json" 2> "$O/r4_bench_cfg3.err"; echo "bench rc=$?"
python3 - "$O/r4_bench_cfg3.json" <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print("ms/step", d["ms_per_step"], "value", d["value"], "frac", d["roofline"]["frac"], "k1_ms", d["roofline"]["kernel_ms"])
print("parity ok", d["parity"]["ok"], json.dumps(d["parity"]["short"]["gate"]["checks"]))
PY
