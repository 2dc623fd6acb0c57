# PMC counters for the ML-step kernels at PMC_P x PMC_L: HBM traffic passes + SQ instruction mix.
# Each counter set in its own rocprofv3 pass (no trace options with --pmc).
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/out}; export OUT
cd /tmp; export TMPDIR=/tmp
P=${PMC_P:-20000}; L=${PMC_L:-2000}
mkdir -p $OUT
[ -n "$PMC_LIST" ] && rocprofv3 -L > $OUT/pmc_list.txt 2>&1
i=0
for set in "FETCH_SIZE" "WRITE_SIZE" "TCC_HIT_sum TCC_MISS_sum" "SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_ACTIVE_INST_VALU" "SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_LDS SQ_INST_CYCLES_VMEM SQ_INSTS_VMEM_WR SQ_LDS_BANK_CONFLICT GRBM_GUI_ACTIVE"; do
  i=$((i+1))
  rm -rf $OUT/pmcany_$i
  timeout 300 rocprofv3 --pmc $set --output-format csv -d $OUT/pmcany_$i -- python3 $R/bench.py --full --steps 3 --warmup 1 --particles $P --landmarks $L --no-cpu-baseline ${PMC_ARGS} > $OUT/pmcany_$i.log 2>&1
  tail -1 $OUT/pmcany_$i.log | cut -c1-200
done
cd $R
python3 - <<'PY'
import csv, glob, collections, json, os
out = {}
for f in sorted(glob.glob(os.environ['OUT'] + '/pmcany_*/**/*counter_collection.csv', recursive=True)):
    acc = collections.defaultdict(lambda: collections.defaultdict(float)); n = collections.Counter()
    for r in csv.DictReader(open(f)):
        k = r['Kernel_Name'][:48]
        acc[k][r['Counter_Name']] += float(r['Counter_Value']); n[(k, r['Counter_Name'])] += 1
    for k, v in acc.items():
        if 'assoc' in k or 'observe' in k or 'settle' in k or 'fused' in k:
            out.setdefault(k, {}).update({a: b / n[(k, a)] for a, b in v.items()})
for k, v in out.items():
    print(k, {a: '%.4g' % b for a, b in v.items()})
json.dump(out, open(os.environ['OUT'] + '/pmc_any.json', 'w'), indent=1)
PY
