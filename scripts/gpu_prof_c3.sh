# kernel trace of the config 3 ML step (100 000 x 2 000)
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/out}; export OUT
cd /tmp; export TMPDIR=/tmp
rm -rf $OUT/prof_c3; mkdir -p $OUT
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_c3 -- python3 $R/bench.py --full --no-cpu-baseline --steps 5 --warmup 2 --particles ${PMC_P:-100000} --landmarks ${PMC_L:-2000} > $OUT/prof_c3.log 2>&1
cd $R
f=$(find $OUT/prof_c3 -name '*kernel_stats.csv' | head -1); [ -n "$f" ] && cp "$f" $OUT/kernel_stats_c3.csv && cut -c1-200 "$f" | head -12
