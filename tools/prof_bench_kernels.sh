REPO=${GRAFT_REPO_ROOT:-$(pwd)}
cd /tmp && export TMPDIR=/tmp
# raw trace and bench line under $PROF_OUT (default: $TMPDIR/cull_prof)
export PROF_OUT=${PROF_OUT:-$TMPDIR/cull_prof}
mkdir -p $PROF_OUT
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $PROF_OUT -o t -- python3 $REPO/bench.py --full --no-cpu-baseline --no-api --no-io --no-c4 --no-c5 > $PROF_OUT/bench.log 2>&1
cd $REPO
python3 - <<'PY'
import csv, glob, os, json
out = os.environ["PROF_OUT"]
f = glob.glob(f"{out}/**/*kernel_stats.csv", recursive=True)[0]
for r in csv.DictReader(open(f)):
    n = r["Name"].replace("(anonymous namespace)::", "").replace("void ", "")
    if n.startswith("k_"): print(f"{n[:60]:60s} {r['Calls']:>6s} avg {float(r['AverageNs'])/1e3:9.2f} min {float(r['MinNs'])/1e3:9.2f} max {float(r['MaxNs'])/1e3:9.2f}")
j = json.loads([l for l in open(f"{out}/bench.log") if l.startswith("{")][-1])
print(j["value"], j["ms_per_step"], j["aggregate"]["views_per_s"])
PY
