set -e
cd ${GRAFT_REPO_ROOT:-/root/repo}
export TMPDIR=/tmp
# Usage: tools/final_bench.sh [out dir, default bench_out]: the whole bench (--full) once plain and once under a kernel trace
OUT=${1:-bench_out}
mkdir -p $OUT
python bench.py --full > $OUT/bench_full.json 2> $OUT/bench_full.err
tail -1 $OUT/bench_full.json | python -c "
import json,sys
d=json.loads(sys.stdin.read())
print('value', d['value'], 'frac', d['roofline']['frac'], 'kernel_ms', d['roofline']['kernel_avg_ms'])
for k,v in d['secondary'].items():
    if isinstance(v,dict):
        print(k, {kk:(round(vv,4) if isinstance(vv,float) else vv) for kk,vv in v.items() if kk in ('apply_aij_GDoF_per_s','apply_aij_ms','roofline_frac_hbm','GDoF_per_s','ms','cheby_5_iterations_ms')})
"
mkdir -p $OUT/prof_final
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_final/trace -- python3 bench.py --full --no-check > $OUT/prof_final/bench.json 2> $OUT/prof_final/bench.err
OUT=$OUT python3 - <<PY > $OUT/prof_final/summary.txt
import csv, glob, os
f = glob.glob(os.path.join(os.environ["OUT"], "prof_final/trace/**/*kernel_stats.csv"), recursive=True)[0]
for r in list(csv.DictReader(open(f)))[:60]:
    print("%-110s calls=%s avg_ns=%s pct=%s" % (r["Name"][:110], r["Calls"], r["AverageNs"], r["Percentage"]))
PY
rm -rf $OUT/prof_final/trace
head -5 $OUT/prof_final/summary.txt
