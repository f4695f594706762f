# usage: tools/cpu_baseline_check.sh [out dir]
out=${1:-bench_out}/cpu
mkdir -p $out
for i in 1 2; do
  timeout -k 10 300 python3 bench.py --full > $out/bench_$i.log 2>&1 || exit 1
  tail -1 $out/bench_$i.log | python3 -c 'import json,sys; d=json.load(sys.stdin); c=d["cpu_baseline"]; print(d["value"], c["value"], c["window_spread"], c["windows_GiBps"], c["streamed_value"], c["streamed_window_spread"], c["single_thread_value"])'
done
timeout -k 10 300 python3 bench.py --full --config 1M_x_256B > $out/bench_256.log 2>&1 || exit 1
tail -1 $out/bench_256.log | python3 -c 'import json,sys; d=json.load(sys.stdin); c=d["cpu_baseline"]; print(d["value"], c["value"], c["window_spread"], c["windows_GiBps"], c["streamed_value"], c["streamed_window_spread"])'
