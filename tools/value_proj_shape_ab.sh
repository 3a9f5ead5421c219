# per-tag time of the hoisted value projections by row-panel shape (BEVMSDA_GEMM_KERNEL: default = the library's rule)
d=$(mktemp)                  # the full record of each run (--detail-json), read back below
trap 'rm -f "$d"' EXIT
for r in 1 2; do
for k in "" panel64 panel128 panelr panelr4; do
  : > "$d"; BEVMSDA_GEMM_KERNEL=$k python bench.py --full --no-cpu-baseline --no-variants --steps 10 --windows 3 --detail-json "$d" 2>/dev/null | tail -1 | python -c "
import json,sys
l=json.loads(sys.stdin.read())
d=json.load(open('$d')); d=d.get('bench_detail',d)
pt=d['gemms']['per_tag']
print('kernel=${k:-default} ms_per_step %.4f' % l['ms_per_step'], {k: round(v['avg_us'],1) for k,v in pt.items()})"
done
done
