cd /tmp && export TMPDIR=/tmp
R="${GRAFT_REPO_ROOT:?}"
cd "$R" || exit 1
O=${1:?usage: bash tools/refresh_admm_profiles.sh OUT   (OUT: output directory, relative to the repo root)}
mkdir -p $O
timeout 200 python3 bench.py --full > $O/final_admm.json 2> $O/final_admm.err
rocprofv3 --kernel-trace --stats -d $R/$O/prof_admm -o admm -- python3 bench.py --steps 10 --full --no-cpu-baseline > $O/prof_admm_bench.json 2> $O/prof_admm.err
timeout 600 python3 tools/scaling_compute_only.py > $O/scaling.json 2> $O/scaling.err
cut -c1-200 $O/final_admm.json
