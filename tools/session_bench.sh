# tools/session_bench.sh OUTDIR : bench lines of the four configs (bench.py --full: deriv leg, CPU baseline and check)
# into OUTDIR, after the PMC traffic files of the tree are in profiles/
set -o pipefail
out="${1:?usage: tools/session_bench.sh OUTDIR}"
mkdir -p "$out"
for c in 3 2 4 5; do
  python3 bench.py --full --config $c --steps 20 --warmup 3 > "$out/bench_cfg$c.log" 2>&1 || { tail -5 "$out/bench_cfg$c.log"; exit 1; }
  grep '^{"metric' "$out/bench_cfg$c.log" > "$out/bench_cfg$c.json"
done
