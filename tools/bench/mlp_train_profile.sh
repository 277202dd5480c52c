# per-kernel breakdown of the MLP bench incl. training steps: rocprofv3 --kernel-trace --stats
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
O=$R/bench_out/mlpprof; mkdir -p $O
rocprofv3 --kernel-trace --stats --output-format csv -d $O -o mlp -- python3 $R/bench.py --full --no-conv --no-cpu-baseline --steps 3 --warmup 1 --adjoint-steps 10 > $O.log 2>&1 || exit 1
python3 - <<PY
import csv,re
for r in csv.DictReader(open("$O/mlp_kernel_stats.csv")):
    m=re.search(r"(k_\w+(<[^>]*>)?)",r["Name"])
    n=m.group(1) if m else r["Name"][:40]
    print("  %-40s n=%5s avg=%8.1f us tot=%8.2f ms"%(n,r["Calls"],float(r["AverageNs"])/1e3,float(r["TotalDurationNs"])/1e6))
PY
