# usage: tools/tiny_ab.sh [out dir]
set -o pipefail
cd ${GRAFT_REPO_ROOT:-/root/repo}
out=$(realpath -m ${1:-bench_out})
mkdir -p $out
lib=blazingmq_amd/lib
base=$(mktemp)
cp $lib/libbmqcrc.so $base
for rep in 1 2; do
for v in base allnt; do
  if [ $v = base ]; then cp $base $lib/libbmqcrc.so; else cp $lib/variant_$v.so $lib/libbmqcrc.so; fi
  for mb in 64 128 512; do
    log=$out/tiny_${v}_${mb}_$rep.log
    timeout -k 10 120 python3 bench.py --full --config 1M_x_256B --msg-bytes $mb --steps 20 --warmup 5 --no-cpu-baseline > $log 2>&1 || { cp $base $lib/libbmqcrc.so; exit 3; }
    echo "$v $mb $(tail -1 $log | python3 -c 'import json,sys; d=json.load(sys.stdin); print(d["value"], d["roofline"]["kernel_avg_us"], d["parity"])')"
  done
done
done
cp $base $lib/libbmqcrc.so
rm -f $base
