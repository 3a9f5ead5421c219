# The round-end visit: full GPU suite, smoke, default bench (tools/final_visit.sh [traffic] adds the PMC traffic profiles).
out=$(mktemp -d)
python -m pytest tests -m gpu -q -x 2>&1 | tail -15 > $out/pytest_gpu.log
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $out/smoke.log 2>&1
python bench.py --full > $out/bench_default.json 2> $out/bench_default.err
python tools/bench_digest.py $out/bench_default.json > $out/bench_digest.txt 2>&1
if [ "$1" = "traffic" ]; then
  python tools/profile_traffic.py --config base_fwd > $out/traffic_fwd.log 2>&1
  python tools/profile_traffic.py --config base_bwd > $out/traffic_bwd.log 2>&1
  python tools/profile_traffic.py --config small4_bwd_bf16 > $out/traffic_small4.log 2>&1
fi
tail -3 $out/pytest_gpu.log; tail -2 $out/smoke.log; cut -c1-160 $out/bench_digest.txt | head -40
echo "logs: $out"
