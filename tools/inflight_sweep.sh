# bench.py at the driver's step counts with 2, 3 and 4 batches in flight (no CPU baseline)
set -e
(while sleep 50; do date >> gpurun_out/tick.log; done) &
TICK=$!
trap 'kill $TICK' EXIT
# --full for config.batch_latency_ms (one batch alone); written where tools/summarize_profiles.py reads
O=$(python3 -c "import sys; sys.path.insert(0, 'tools'); import summarize_profiles as s; print(s.OUT)")
for n in 2 3 4; do
  timeout -k 10 240 python3 bench.py --steps 20 --warmup 5 --full --no-cpu --inflight $n > "$O/inflight_$n.json" 2> "$O/inflight_$n.err"
done
