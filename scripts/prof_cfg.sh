# rocprofv3 kernel stats of one bench config: bash scripts/prof_cfg.sh <config> [extra bench args]
# Output: ${SCC_OUT_DIR:-bench_out}/prof_<config>/, prof_<config>.log, kstats_<config>.csv
set -u
cfg=$1; shift
export TMPDIR=/tmp
cd "$(dirname "$0")/.."
out=${SCC_OUT_DIR:-bench_out}
mkdir -p $out
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $out/prof_$cfg -o run --output-format csv -- \
  python3 bench.py --full --config "$cfg" --no-cpu-baseline --no-pearson --steps 2 --warmup 1 "$@" > $out/prof_$cfg.log 2>&1
rc=$?
f=$(find $out/prof_$cfg -name '*kernel_stats.csv' | head -n 1)
[ -n "$f" ] && cp "$f" $out/kstats_$cfg.csv && head -n 25 "$f"
exit $rc
