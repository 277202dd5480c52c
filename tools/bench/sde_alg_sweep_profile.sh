# artifacts for profiles/sde_model/alg_sweep_*: the pullback bench JSON (no profiler), then a rocprofv3 --kernel-trace --stats table
# (no counters) of the one-launch sweep's route alone — three warm-ups and three calls per kind — in a run of its own
R=$(cd "$(dirname "$0")/../.." && pwd)
O=${1:-$R/bench_out/sde_alg_sweep}
mkdir -p "$O"
timeout -k 10 300 python3 "$R/tools/bench/sde_alg_sweep_bench.py" "$O/alg_sweep_bench.json" || exit 1
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/prof_sweep" -o sweep -- \
  python3 "$R/tools/bench/sde_alg_sweep_bench.py" --route sweep --reps 3 > "$O/prof_sweep.log" 2>&1 || { tail -5 "$O/prof_sweep.log"; exit 1; }
