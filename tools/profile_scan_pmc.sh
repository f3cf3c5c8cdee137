# Pipe / stall counters of the MFMA scan at 64 and 128 queries (rocprofv3, one small counter set per run).
# Run on the GPU box:  gpurun --timeout 900 -- "bash tools/profile_scan_pmc.sh"
# Optional, for a comparison of two builds over one command line:
#   PCV_PMC_SET="A B C D"   one counter set instead of the three below
#   PCV_PMC_BATCHES="64"    the query counts
#   PCV_PMC_ROWS=100000000  rows of the corpus
#   PCV_PMC_BENCH=path      the bench.py to run (a second checkout, built)
#   PCV_PMC_TAG=name        prefix of the output files (default pmc_scan)
R=$GRAFT_REPO_ROOT
cd /tmp && export TMPDIR=/tmp
G=$R/gpurun_out
mkdir -p $G
BENCH=${PCV_PMC_BENCH:-$R/bench.py}
TAG=${PCV_PMC_TAG:-pmc_scan}
ROWS=${PCV_PMC_ROWS:-50000000}
if [ -n "${PCV_PMC_SET:-}" ]; then
  SETS=("$PCV_PMC_SET")
else
  SETS=("SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_INST_CYCLES_VMEM" \
        "SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_INST_LEVEL_LDS SQ_WAIT_INST_LDS" \
        "SQ_VALU_MFMA_BUSY_CYCLES SQ_INST_LEVEL_VMEM SQ_ACTIVE_INST_VALU SQ_WAVES")
fi
i=0
for B in ${PCV_PMC_BATCHES:-64 128}; do
  for set in "${SETS[@]}"; do
    i=$((i+1))
    rm -rf $G/${TAG}_$i
    timeout -k 10 300 rocprofv3 --pmc $set --kernel-trace --output-format csv -d $G/${TAG}_$i -o p -- \
      python3 $BENCH --no-cpu-baseline --no-extra --rows $ROWS --batch $B --steps 2 --warmup 1 > $G/${TAG}_$i.log 2>&1 || { echo "FAILED set $i"; tail -3 $G/${TAG}_$i.log; exit 1; }
  done
done
export PCV_PMC_RUNS=$i PCV_PMC_TAG=$TAG
python3 - <<'PY'
import csv, glob, os, collections
G = os.environ.get("GRAFT_REPO_ROOT", ".") + "/gpurun_out"
tag, runs = os.environ["PCV_PMC_TAG"], int(os.environ["PCV_PMC_RUNS"])
out = open(f"{G}/{tag}_summary.txt", "w")
for i in range(1, runs + 1):
    agg = collections.defaultdict(lambda: collections.defaultdict(float))
    calls = collections.Counter()
    for f in glob.glob(f"{G}/{tag}_{i}/*counter_collection.csv") + glob.glob(f"{G}/{tag}_{i}/*/*counter_collection.csv"):
        for row in csv.DictReader(open(f)):
            k = row["Kernel_Name"]
            if "scan_mfma" not in k: continue
            agg[k][row["Counter_Name"]] += float(row["Counter_Value"])
            calls[(k, row["Counter_Name"])] += 1
    for k, c in agg.items():
        short = k[k.find("scan_mfma"):][:60]
        for name, v in c.items():
            line = f"set {i}  {short:62s} {name:28s} {v / max(1, calls[(k, name)]):.4g} per launch"
            print(line); out.write(line + "\n")
PY
