# rocprofv3 --kernel-trace --stats of the default bench command with --full (config 4, ADMM): the kernel stats of the whole run
# beside the bench line's roofline.      bash tools/profile_bench_c4.sh OUT   (OUT: output directory, relative to the repo root)
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
O=${1:?usage: bash tools/profile_bench_c4.sh OUT}
mkdir -p $R/$O
timeout 900 rocprofv3 --kernel-trace --stats -d $R/$O/prof_bench/stats -o s -- python3 $R/bench.py --steps 10 --full --no-cpu-baseline --no-secondary --no-general > $R/$O/prof_bench_line.json 2> /dev/null
cd $R
f=$(find $O/prof_bench/stats -name "*.db" | head -1)
if [ -n "$f" ]; then timeout 120 python3 tools/summarize_rocprof.py db-stats $f > $O/bench_admm_c4_kernel_stats.csv; fi
rm -rf $O/prof_bench
head -12 $O/bench_admm_c4_kernel_stats.csv | cut -c1-150
python3 -c "
import json; d=json.loads(open('$O/prof_bench_line.json').read().strip().splitlines()[-1]); r=d['roofline']; print(d['value'], r['ms_per_product'], r['frac'])"
