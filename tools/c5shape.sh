# config-5-shaped block run (5e5 x 5e7 at 1e-4 on one GPU), 1 and 4 blocks per rank; bench.py turns SLP_TALL_SPLIT on for admm_blocks
R="${GRAFT_REPO_ROOT:?}"
cd "$R" || exit 1
O=${1:?usage: bash tools/c5shape.sh OUT   (OUT: output directory, relative to the repo root)}
mkdir -p $O
for g in 1 4; do
  python bench.py --method admm_blocks --blocks-per-rank $g --n 50000000 --m 500000 --density 1e-4 --steps 3 --warmup 1 --full --no-cpu-baseline > $O/bench_blocks_c5shape_split_g$g.json 2> $O/bench_blocks_c5shape_split_g$g.err
  tail -3 $O/bench_blocks_c5shape_split_g$g.err
  python -c "
import json
d=json.load(open('$O/bench_blocks_c5shape_split_g$g.json')); r=d['roofline']; print(d['metric'], d['value'], d['ms_per_step'], r['kernel'][:14], r['frac'], r['ms_per_product'], r['spmv_transposed']['ms_per_product'], d['setup_seconds'], d['config'].get('cg_steps_per_iteration'), d['device_memory'])
"
done
