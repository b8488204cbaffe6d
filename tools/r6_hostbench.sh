set -e
OUT=${OUT:-bench_out/r6_j}
mkdir -p $OUT
for c in cascade v6 pf6 gpu; do
  timeout -k 10 300 python -u bench.py --full --config $c --host-tuples --steps 5 --warmup 2 --no-cpu-baseline > $OUT/host_$c.json 2> $OUT/host_$c.err
done
