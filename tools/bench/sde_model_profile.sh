# artifacts for profiles/sde_model: the bench JSON (no profiler), then rocprofv3 --kernel-trace --hip-trace --stats tables of 20 bare
# training steps of each path (the new step; the path the package offered before it), each in a run of its own
R=$(cd "$(dirname "$0")/../.." && pwd)
O=${1:-$R/bench_out/sde_model}
mkdir -p "$O"
timeout -k 10 300 python3 "$R/tools/bench/sde_model_bench.py" --out "$O/bench.json" || exit 1
for p in ours parent; do
  timeout -k 10 300 rocprofv3 --kernel-trace --hip-trace --stats --output-format csv -d "$O/prof_$p" -o "$p" -- \
    python3 "$R/tools/bench/sde_model_bench.py" --only "$p" --steps 20 > "$O/prof_$p.log" 2>&1 || { tail -5 "$O/prof_$p.log"; exit 1; }
done
