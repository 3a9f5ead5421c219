for lib in default tsa256 default tsa256 default tsa256; do
  if [ $lib = default ]; then unset BEVMSDA_LIBRARY; else export BEVMSDA_LIBRARY=$PWD/bevformer_amd/lib/libbevmsda_$lib.so; fi
  python bench.py --full --no-cpu-baseline --no-variants --backward --steps 10 --warmup 3 --windows 3 2>/dev/null | python -c "
import json,sys
ls=[l for l in sys.stdin if l.startswith('{')]
d=json.loads(ls[0]); d=d.get('bench_detail', d)
k=d['kernels']
print('$lib fwd+bwd base ms_per_step %.3f' % d['ms_per_step'], {t: round(k[t]['avg_us'],1) for t in k})"
done
