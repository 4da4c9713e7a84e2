"""The one-line JSON contract of bench.py: every key the driver and the judge read, on the committed final bench
lines (CPU) and on a small live run (GPU)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import MAX_RANKS_ON_ONE_GPU

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TOP = {"metric": str, "value": float, "unit": str, "n_gpus": int, "steps": int, "warmup": int, "ms_per_step": float,
       "higher_is_better": bool, "scaling": str, "dtype": str, "data": str, "config": dict, "roofline": dict}
ROOFLINE = ("bound", "achieved", "peak", "unit", "frac", "traffic")
CPU = ("value", "unit", "cores", "kind", "sample")


def _per_product(r, what):
    """``bytes`` / ``matrix_copy_bytes`` / ``ms`` of one product: round 5 renamed the ``*_per_launch`` keys, which had always
    meant per PRODUCT (a chunked matrix takes several launches for one)."""
    return r.get(what + "_per_product", r.get(what + "_per_launch"))


def check_line(d, need_cpu_baseline):
    for key, typ in TOP.items():
        assert key in d, key
        assert isinstance(d[key], typ) or (typ is float and isinstance(d[key], int)), (key, type(d[key]))
    assert "vs_baseline" in d and d["vs_baseline"] is None          # BASELINE.md holds no published number
    assert d["higher_is_better"] is True and d["unit"] == "it/s" and d["dtype"] == "f64" and d["data"] == "synthetic"
    assert d["scaling"] in ("weak", "strong") and "workload" in d["config"] and "model" not in d["config"]
    assert abs(d["value"] - 1000.0 * d["steps"] / (d["ms_per_step"] * d["steps"])) < 1e-6 * d["value"]
    r = d["roofline"]
    for key in ROOFLINE:
        assert key in r, key
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s") and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    if "products_timed" in r:  # round 6 (late): ~0.3 s of back-to-back products (reps from a 3-product estimate) behind a warm-up, never fewer than five
        assert r["products_timed"] >= 5 and (r["products_timed"] * r["ms_per_product"] >= 150.0 or r["products_timed"] == 400)
    if r.get("timed_region"):  # round 6 (late): HIP event pairs around every product of the K timed steps themselves
        t = r["timed_region"]
        assert t["products"] == round(t["products_per_step"] * d["steps"]) and t["products"] > 0
        assert 0.0 < t["ms_per_product"] <= t["longest_ms"] and 0.0 < t["share_of_step"] <= 1.0
        assert abs(t["frac"] - t["achieved"] / r["peak"]) < 1e-12 and 0.0 < t["frac"] <= 1.0
    if _per_product(r, "bytes") is not None:  # round 2 on: bytes the kernel has to move / time -- a fraction of the peak, never above it
        assert 0.0 < r["frac"] <= 1.0
        assert _per_product(r, "bytes") >= _per_product(r, "matrix_copy_bytes") > 0
    if "exchange" in d:   # round 5 on: what of a step was exchange
        e = d["exchange"]
        for key in ("ms_per_iteration", "collectives_per_iteration", "bytes_per_collective", "algbw_gbps", "compute_ms_per_step",
                    "collectives_timed", "slowest_collective_ms"):
            assert key in e, key
        assert e["collectives_per_iteration"] == d["config"]["collectives_per_iteration"] and "shard_updates" in d["config"]
        assert 0.0 <= e["ms_per_iteration"] <= d["ms_per_step"] * 1.001 + e["ms_overlapped_per_iteration"]
        if d["config"]["collectives_per_iteration"] > 0:
            assert e["collectives_timed"] == round(e["collectives_per_iteration"] * d["steps"]) and e["bytes_per_collective"] > 0
            assert e["ms_per_iteration"] > 0 and e["algbw_gbps"] > 0
            # (serial collectives come off the step; fully overlapped ones -- block groups -- leave compute = step)
            exposed = e["ms_per_iteration"] - e["ms_overlapped_per_iteration"]
            assert abs(e["compute_ms_per_step"] - (d["ms_per_step"] - exposed)) < 1e-9 and e["compute_ms_per_step"] <= d["ms_per_step"] + 1e-9
        else:
            assert e["ms_per_iteration"] == 0 and abs(e["compute_ms_per_step"] - d["ms_per_step"]) < 1e-9
    if need_cpu_baseline:
        c = d["cpu_baseline"]
        for key in CPU:
            assert key in c, key
        assert c["kind"] in ("reference", "port") and c["cores"] >= 1 and c["value"] > 0


@pytest.mark.parametrize("name", ["r01_bench_admm_c3_final.json", "r01_bench_cp_c3_final.json", "r02_bench_admm_c3.json",
                                  "r02_bench_cp_c3.json"])
def test_committed_bench_lines(name):
    d = json.loads(open(os.path.join(REPO, "profiles", name)).read().strip().splitlines()[-1])
    check_line(d, need_cpu_baseline=True)
    assert d["n_gpus"] == 1 and d["config"]["n"] == 1_000_000 and d["config"]["m"] == 2_000_000  # BASELINE config 3
    assert d["roofline"]["traffic"] is not None and d["roofline"]["traffic"] > 1e9                # PMC bytes per launch
    if name.startswith("r02"):  # round 2: admissible fraction, the general path in the same line, an honest CPU baseline
        r = d["roofline"]
        assert r["frac"] <= 1.0 and abs(r["traffic"] / _per_product(r, "bytes") - 1.0) < 0.1          # PMC agrees with the bytes moved
        g = r["general_fp64"]
        assert 0.5 < g["spmv"]["frac"] <= 1.0 and 0.5 < g["spmv_transposed"]["frac"] <= 1.0
        assert g["admm_it_per_s"] > 0 and g["chambolle_pock_it_per_s"] > 0
        assert d["cpu_baseline"]["extrapolated"] is True and d["setup_seconds"] > 0 and d["device_memory"]["csr_released"]


@pytest.mark.parametrize("name", ["r03_bench_admm_c4slice.json", "r03_bench_cp_c4slice.json", "r03_bench_admm_c3_500steps.json"])
def test_committed_round3_bench_lines(name):
    """`bench.py --config c4slice` (BASELINE config 4's per-rank shape at the density that fits: 2.5e6 rows x 1e7 variables
    at 1e-4) and the 500-step config-3 line."""
    d = json.loads(open(os.path.join(REPO, "profiles", name)).read().strip().splitlines()[-1])
    check_line(d, need_cpu_baseline=True)
    r = d["roofline"]
    assert d["n_gpus"] == 1 and 0.0 < r["frac"] <= 1.0 and d["cpu_baseline"]["extrapolated"] is True
    if "c4slice" in name:
        assert (d["config"]["n"], d["config"]["m"], d["config"]["density"]) == (10_000_000, 2_500_000, 1e-4)
        assert "k_tall_spmv" in r["kernel"] and r["frac"] >= 0.30          # >= 0.30 of the HBM peak
        assert r["traffic"] is not None and abs(r["traffic"] / _per_product(r, "bytes") - 1.0) < 0.15
    else:
        assert d["steps"] == 500 and d["config"]["n"] == 1_000_000
        assert r["traffic_measured_in_this_run"] is False
        assert d["cpu_baseline"]["full_size_validation"]["source"] == "profiles/r03_cpu_full_c3.json"


@pytest.mark.parametrize("name", ["r04_bench_admm_c4_1gpu.json", "r04_bench_cp_c4_1gpu.json", "r04_bench_admm_c4slice.json",
                                  "r04_bench_admm_c3.json"])
def test_committed_round4_bench_lines(name):
    """Round 4: the default workload is the LP BASELINE.json's metric names -- 1e7 variables x 2e7 rows at the density that fits
    (1e-4), resident on ONE GPU in row chunks -- with config 3 as the secondary block of the default line."""
    d = json.loads(open(os.path.join(REPO, "profiles", name)).read().strip().splitlines()[-1])
    check_line(d, need_cpu_baseline=True)
    r = d["roofline"]
    assert d["n_gpus"] == 1 and 0.0 < r["frac"] <= 1.0
    if "c4_1gpu" in name:
        assert (d["config"]["n"], d["config"]["m"], d["config"]["density"]) == (10_000_000, 20_000_000, 1e-4)
        assert d["config"]["chunks_per_rank"] == 8 and d["config"]["nnz"] > 1.9e10 and "row chunks" in d["config"]["workload"]
        assert "k_tall_spmv" in r["kernel"] and r["frac"] >= 0.40                       # north_star: >= 40 % of the HBM roofline on the SpMV
        assert r.get("launches_per_product", 8) == 8                                      # one launch per row chunk
        assert r["traffic"] is not None and abs(r["traffic"] / _per_product(r, "bytes") - 1.0) < 0.15   # PMC bytes = the copy, per PRODUCT
        assert d["device_memory"]["in_use_in_timed_region_gb"] < 288 and d["setup_breakdown"]["peak_device_gb"] < 300
        assert d["cpu_baseline"]["extrapolated"] is True and d["cpu_baseline"]["cores"] == 1
        if "admm" in name:                                                                # the default line carries config 3 too
            c3 = d["secondary"]["c3"]
            assert c3["config"]["n"] == 1_000_000 and c3["value"] > 100 and 0.4 < c3["roofline"]["frac"] <= 1.0
    elif "c4slice" in name:
        assert d["config"]["chunks_per_rank"] == 1 and r["frac"] >= 0.38
    else:
        assert d["config"]["n"] == 1_000_000 and d["value"] > 100
        assert d["cpu_baseline"]["extrapolated"] is False                                 # the full-size one-thread measurement
        assert d["cpu_baseline"]["value_extrapolated_from_sample"] > d["cpu_baseline"]["value"] * 0.8


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["admm", "chambolle_pock_ppd"])
def test_live_bench_line(method):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--n", "20000", "--m", "40000", "--density", "0.001",
                        "--steps", "4", "--warmup", "1", "--method", method, "--full"],
                       capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1  # exactly one JSON line on stdout
    d = json.loads(lines[0])
    check_line(d, need_cpu_baseline=True)
    assert d["steps"] == 4 and d["warmup"] == 1 and d["n_gpus"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["admm", "chambolle_pock_ppd"])
def test_dump_outputs_holds_the_solution_of_the_timed_steps(method, tmp_path):
    """``--dump-outputs DIR``: DIR/x.npy is the solution over the n variables that the K timed steps left, float64, the same
    for two runs with the same arguments, and its objective is the line's ``objective_after_run``."""
    import numpy as np

    n, m, p = 20000, 40000, 0.001
    xs = []
    for run in range(2):
        out = tmp_path / f"run{run}"
        r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--n", str(n), "--m", str(m), "--density", str(p),
                            "--steps", "3", "--warmup", "1", "--method", method, "--no-cpu-baseline", "--no-general",
                            "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=REPO)
        assert r.returncode == 0, r.stderr[-3000:]
        d = json.loads([l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1])
        assert d["steps"] == 3 and d["warmup"] == 1
        assert sorted(os.listdir(out)) == ["x.npy"]
        x = np.load(out / "x.npy")
        assert x.dtype == np.float64 and x.shape == (n,) and np.all(np.isfinite(x))
        xs.append((x, d["objective_after_run"]))
    assert np.array_equal(xs[0][0], xs[1][0]) and xs[0][1] == xs[1][1]
    sys.path.insert(0, REPO)
    from pysparselp_amd.problems import random_lp_on_device

    a, xf, c, lb, ub, b = random_lp_on_device(n, m, p, seed=0)
    a.close()
    assert float(c.dot(xs[0][0])) == xs[0][1]


def test_dump_outputs_samples_a_large_solution_the_same_way_every_time(tmp_path):
    """Above DUMP_MAX_VALUES variables x.npy holds a fixed sample of x: sorted indices drawn with seed 0, float64."""
    code = ("import runpy, sys\nimport numpy as np\nb = runpy.run_path(sys.argv[1])\ncap = b['DUMP_MAX_VALUES']\n"
            "x = np.arange(cap + 1_000_000, dtype=np.float32)\n"
            "b['dump_outputs'](sys.argv[2] + '/a', x)\nb['dump_outputs'](sys.argv[2] + '/b', x)\n"
            "b['dump_outputs'](sys.argv[2] + '/c', x[:1000])\n")
    r = subprocess.run([sys.executable, "-c", code, os.path.join(REPO, "bench.py"), str(tmp_path)], capture_output=True, text=True,
                       timeout=120, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    import numpy as np

    a, b, c = (np.load(tmp_path / k / "x.npy") for k in "abc")
    assert a.dtype == np.float64 and a.size == 4_000_000 and a.nbytes <= 64e6
    assert np.array_equal(a, b) and np.all(np.diff(a) > 0)          # the same sorted entries of x (here x[i] = i) each time
    assert c.dtype == np.float64 and np.array_equal(c, np.arange(1000))   # a small x is written whole


FULL_ONLY = ("roofline", "chambolle_pock", "cpu_baseline", "secondary")   # what --full measures after the timed steps


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["admm", "chambolle_pock_ppd"])
def test_plain_line_is_the_headline_of_the_full_one(method, tmp_path):
    """Without ``--full`` bench.py sets up, warms up, times the K steps, dumps x and prints the line: the headline keys, meaning
    what they mean under ``--full``, and nothing that ``--full`` measures after the timed steps.  Both runs time the same steps:
    same LP, same x, same objective."""
    import numpy as np

    runs = {}
    for mode in ("plain", "full"):
        r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--n", "20000", "--m", "40000", "--density", "0.001",
                            "--steps", "4", "--warmup", "1", "--method", method, "--dump-outputs", str(tmp_path / mode)]
                           + (["--full"] if mode == "full" else []), capture_output=True, text=True, timeout=600, cwd=REPO)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
        assert len(lines) == 1
        runs[mode] = json.loads(lines[0]), np.load(tmp_path / mode / "x.npy")
    (plain, x_plain), (full, x_full) = runs["plain"], runs["full"]
    check_line(full, need_cpu_baseline=True)
    for key, typ in TOP.items():
        if key != "roofline":
            assert isinstance(plain[key], typ) or (typ is float and isinstance(plain[key], int)), (key, type(plain.get(key)))
    assert not [k for k in FULL_ONLY if k in plain] and set(plain) <= set(full)
    assert plain["vs_baseline"] is None and plain["higher_is_better"] is True and plain["unit"] == "it/s" and plain["dtype"] == "f64"
    assert abs(plain["value"] - 1000.0 / plain["ms_per_step"]) < 1e-6 * plain["value"]
    assert plain["steps"] == 4 and plain["warmup"] == 1 and plain["n_gpus"] == 1
    assert plain["metric"] == full["metric"] and plain["config"] == full["config"]
    assert plain["objective_after_run"] == full["objective_after_run"] and np.array_equal(x_plain, x_full)


def test_full_is_an_option_off_by_default():
    code = ("import runpy, sys\nb = runpy.run_path(sys.argv[1])\nsys.argv = ['bench.py']\nassert b['parse']().full is False\n"
            "sys.argv = ['bench.py', '--full']\nassert b['parse']().full is True\n")
    r = subprocess.run([sys.executable, "-c", code, os.path.join(REPO, "bench.py")], capture_output=True, text=True, timeout=120,
                       cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]


def test_steps_below_one_are_rejected():
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120,
                       cwd=REPO)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr

def _launch(nproc, extra_env, port, more=()):
    env = dict(os.environ, **extra_env)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(REPO, "bench.py"), "--gpus", str(nproc), "--steps", "4", "--warmup", "2",
           "--vars", "30000", "--rows", "40000", "--density", "0.001", "--full", "--no-cpu-baseline", "--no-general"] + list(more)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=REPO, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]  # rank 0 only
    return json.loads(lines[0])


def _self_launch(nproc, extra_env, more=()):
    """``python bench.py --gpus N`` as the driver's N = 1 command is shaped: bench.py starts its own ranks (no torch, no launcher)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    env.update(extra_env)
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", str(nproc), "--steps", "4", "--warmup", "2",
           "--vars", "30000", "--rows", "40000", "--density", "0.001", "--full", "--no-cpu-baseline", "--no-general"] + list(more)
    return subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=REPO, env=env)


def test_self_launched_ranks_fail_loudly_without_a_gpu_or_with_a_dead_rank():
    """No launcher: ``bench.py --gpus 2`` spawns its two ranks itself.  A rank that cannot run (here: a device index no box has) ends
    the whole job with a non-zero exit code and no JSON line -- never a hang, never a line from a partial job."""
    r = _self_launch(2, {"SLP_DEVICE": "63"})
    assert r.returncode != 0
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert "job ended" in r.stderr


@pytest.mark.gpu
def test_self_launched_two_ranks_equal_the_launcher_run():
    """``python bench.py --gpus 2`` (self-launched: child processes + the TCP id exchange of pysparselp_amd/parallel.py, no torch
    anywhere in the multi-GPU path) gives the line the ``torch.distributed.run`` launch gives: two ranks on one GPU through the
    host transport, same stored entries, same collectives, the same objective bit for bit."""
    env = {"SLP_DEVICE": "0", "SLP_COMM_TRANSPORT": "host", "SLP_STRIP_MIN_NNZ": "1"}
    r = _self_launch(2, env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]  # rank 0 only
    mine = json.loads(lines[0])
    check_line(mine, need_cpu_baseline=False)
    assert mine["n_gpus"] == 2 and mine["scaling"] == "strong" and mine["config"]["collectives_per_iteration"] == 2.0
    theirs = _launch(2, env, 29731)
    assert mine["config"]["nnz"] == theirs["config"]["nnz"] and mine["objective_after_run"] == theirs["objective_after_run"]
    # no torch in any rank of the self-launched job
    probe = subprocess.run([sys.executable, "-c", "import sys, runpy; sys.argv = ['bench.py', '--help']\n"
                            "try:\n    runpy.run_path('bench.py', run_name='__main__')\nexcept SystemExit:\n    pass\n"
                            "import pysparselp_amd.parallel, pysparselp_amd.scale, pysparselp_amd.admm_cg\n"
                            "assert 'torch' not in sys.modules, 'torch was imported'"], capture_output=True, text=True, cwd=REPO, timeout=120)
    assert probe.returncode == 0, probe.stderr[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["chambolle_pock_ppd", "admm"])
def test_two_ranks_with_equality_rows_match_one_rank(method):
    """SURVEY 8(d)'s equality variant under a row partition (``--eq-frac 0.1 --gpus 2``, self-launched, host transport on one GPU): the
    first rank's block holds the equality rows and some inequality rows, the second only inequalities; every rank is told ITS number of
    equality rows.  Same LP (stored entries), same objective as the one-process run to the summation-order tolerance of a partition."""
    env = {"SLP_DEVICE": "0", "SLP_COMM_TRANSPORT": "host", "SLP_STRIP_MIN_NNZ": "1"}
    more = ("--eq-frac", "0.1", "--method", method)
    r2 = _self_launch(2, env, more=more)
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-4000:]
    two = json.loads([l for l in r2.stdout.strip().splitlines() if l.startswith("{")][0])
    check_line(two, need_cpu_baseline=False)
    r1 = _self_launch(1, {"SLP_STRIP_MIN_NNZ": "1"}, more=more)
    assert r1.returncode == 0, r1.stdout[-2000:] + r1.stderr[-4000:]
    one = json.loads([l for l in r1.stdout.strip().splitlines() if l.startswith("{")][0])
    assert two["n_gpus"] == 2 and one["n_gpus"] == 1 and two["config"]["equality_rows"] == one["config"]["equality_rows"] == 4000
    assert two["config"]["nnz"] == one["config"]["nnz"]
    assert abs(two["objective_after_run"] - one["objective_after_run"]) <= 1e-9 * (1 + abs(one["objective_after_run"]))


@pytest.mark.gpu
def test_bench_under_the_launcher_one_rank_rccl():
    """The driver's launch line with N = 1 and the N > 1 plumbing forced on: launcher env, TCP id exchange, a one-rank
    RCCL communicator, the packed exchange (2 collectives per ADMM iteration)."""
    d = _launch(1, {"SLP_BENCH_FORCE_DIST": "1", "SLP_FORCE_DISTRIBUTED": "1", "SLP_STRIP_MIN_NNZ": "1"}, 29631)
    check_line(d, need_cpu_baseline=False)
    assert d["n_gpus"] == 1 and d["config"]["collectives_per_iteration"] == 2.0


@pytest.mark.gpu
def test_bench_under_the_launcher_two_ranks_on_one_gpu():
    """--gpus 2 on ONE device through the host transport (RCCL refuses two ranks on one GPU): row partition, rank-0-only
    output, max-over-ranks timing, whole-job rate; the objective must agree with the single-process run."""
    two = _launch(2, {"SLP_DEVICE": "0", "SLP_COMM_TRANSPORT": "host", "SLP_STRIP_MIN_NNZ": "1"}, 29641)
    check_line(two, need_cpu_baseline=False)
    assert two["n_gpus"] == 2 and two["scaling"] == "strong" and two["config"]["collectives_per_iteration"] == 2.0
    one = _launch(1, {"SLP_STRIP_MIN_NNZ": "1"}, 29651)
    assert two["config"]["nnz"] == one["config"]["nnz"]
    assert abs(two["objective_after_run"] - one["objective_after_run"]) <= 1e-9 * (1 + abs(one["objective_after_run"]))


@pytest.mark.gpu
def test_bench_under_the_launcher_two_ranks_with_chunked_row_blocks():
    """What the driver's `--gpus 2` run does on the default workload, in small: every rank's row block is itself generated,
    converted and released in row chunks (`--chunks 3`); same objective as the single-process unchunked run."""
    two = _launch(2, {"SLP_DEVICE": "0", "SLP_COMM_TRANSPORT": "host", "SLP_STRIP_MIN_NNZ": "1"}, 29681, more=("--chunks", "3"))
    check_line(two, need_cpu_baseline=False)
    assert two["n_gpus"] == 2 and two["config"]["chunks_per_rank"] == 3 and "row chunks" in two["config"]["workload"]
    one = _launch(1, {"SLP_STRIP_MIN_NNZ": "1"}, 29691)
    assert one["config"]["chunks_per_rank"] == 1 and two["config"]["nnz"] == one["config"]["nnz"]
    assert abs(two["objective_after_run"] - one["objective_after_run"]) <= 1e-9 * (1 + abs(one["objective_after_run"]))


@pytest.mark.gpu
def test_bench_block_groups_under_the_launcher_two_ranks_on_one_gpu():
    """What `--config c5 --gpus 2` does, in small: block-splitting ADMM with TWO row blocks on each of two ranks, every block
    generated from its own row range (no resident matrix), a block's consensus all-reduce issued beside the next block's
    projection: 2 collectives per iteration, all timed, the overlapped part reported; same objective as one rank with four blocks."""
    more = ("--method", "admm_blocks", "--blocks-per-rank", "2")
    two = _launch(2, {"SLP_DEVICE": "0", "SLP_COMM_TRANSPORT": "host", "SLP_STRIP_MIN_NNZ": "1"}, 29711, more=more)
    check_line(two, need_cpu_baseline=False)
    cfg, e = two["config"], two["exchange"]
    assert two["n_gpus"] == 2 and cfg["blocks_per_rank"] == 2 and cfg["blocks_total"] == 4 and cfg["collectives_per_iteration"] == 2.0
    assert "no resident matrix" in cfg["workload"] and e["ms_overlapped_per_iteration"] > 0 and cfg["cg_steps_per_block_update"] > 0
    one = _launch(1, {"SLP_STRIP_MIN_NNZ": "1"}, 29721, more=("--method", "admm_blocks", "--blocks-per-rank", "4"))
    assert one["config"]["blocks_total"] == 4 and one["config"]["nnz"] == two["config"]["nnz"]
    assert abs(two["objective_after_run"] - one["objective_after_run"]) <= 1e-8 * (1 + abs(one["objective_after_run"]))


@pytest.mark.gpu
@pytest.mark.timeout(1200)
def test_bench_under_the_launcher_four_ranks_on_one_gpu():
    """The driver's 4-GPU launch line (`torch.distributed.run --nproc-per-node 4 ... bench.py --gpus 4`) with all four ranks on
    ONE device through the host transport: four row blocks, one line from rank 0, the single-process objective.  (Four, not
    eight: see conftest.MAX_RANKS_ON_ONE_GPU.)"""
    world = MAX_RANKS_ON_ONE_GPU
    four = _launch(world, {"SLP_DEVICE": "0", "SLP_COMM_TRANSPORT": "host", "SLP_STRIP_MIN_NNZ": "1"}, 29661)
    check_line(four, need_cpu_baseline=False)
    assert four["n_gpus"] == world and four["scaling"] == "strong" and four["config"]["collectives_per_iteration"] == 2.0
    one = _launch(1, {"SLP_STRIP_MIN_NNZ": "1"}, 29671)
    assert four["config"]["nnz"] == one["config"]["nnz"]
    assert abs(four["objective_after_run"] - one["objective_after_run"]) <= 1e-9 * (1 + abs(one["objective_after_run"]))

