cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
O=$R/bench_out/sdeprof; mkdir -p $O
rocprofv3 --kernel-trace --stats --output-format csv -d $O -o sde -- python3 $R/bench.py --full --workload mnist_sde --no-cpu-baseline > $O.log 2>&1 || exit 1
python3 - <<PY
import csv,re
for r in csv.DictReader(open("$O/sde_kernel_stats.csv")):
    m=re.search(r"(k_\w+(<[^>]*>)?)",r["Name"])
    if m: print("  %-30s n=%5s avg=%8.1f us"%(m.group(1),r["Calls"],float(r["AverageNs"])/1e3))
PY
