"""The per-instance stopping test of the batched ADMM solver (ADMMBatchState.set_stop, csrc/slp_admm_batch.hip): what it costs
when it was never armed, what the armed test costs, and what it buys.

    python tools/bench_admm_batch_stop.py OUTDIR [--parts a,b,c] [--parent-repo DIR]
                 [--sets 256:1:tile,256:1:levels,256:8:tile,256:8:levels,256:64:tile,256:64:levels,50:64,50:256]
                 [--price 256:64:tile,256:64:levels,50:64] [--buys 50:64,50:256] [--tol 1e-2] [--check-every 10]
                 [--horizon 3000] [--iters 2000] [--warmup 20] [--repeats 3] [--seconds 0.3]

Writes one JSON line (stdout and OUTDIR/admm_batch_stop.json).  The measuring code is that of tools/bench_cp_batch_gap.py: times
between two HIP events on the library's stream, a warm-up, `repeats` measurements that alternate between the variants compared,
the median with every repeat and the spread ((max - min) / median) beside it.  A set is `potts size:B[:form]`: the Potts n x n LP
of tools/bench_admm_batch.py with B seeded perturbations of the unary costs, in the form the library's rule chooses or in the one
named (SLP_ADMM_BATCH_FORM).

  (a) unarmed   `iterate(k)` on a state that was never armed, instance-iterations/s, against the PARENT commit's library
                (--parent-repo: a built checkout), alternating child processes, parent then this.  The bar is fixed before the
                run: this median >= parent median x (1 - the parent's own spread between its repeats), per set.
  (b) price     one process per set: no test, and the test armed at both tolerances 0 with check_every 1 and 10; how many
                instances stopped (an exact fixed point with an exact residual would) is recorded.  No bar.
  (c) buys      distinct costs at (--tol, --tol), check_every --check-every, --horizon iterations: per-instance stopping
                iterations, the work ratio sum_k t_k / (B max_k t_k), and the wall time of lp_admm_batch_until against
                lp_admm_batch for max_k t_k iterations, both reporting every --plot iterations.  No bar.

Every GPU step of a run belongs under a time limit of its own (timeout -k 10 SECONDS python tools/bench_admm_batch_stop.py ...).
"""
import argparse
import json
import os
import platform
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_cp_many import timed_iterate  # noqa: E402
from bench_cp_many_stop import summary  # noqa: E402


def sets_of(text):
    """`size:B[:form]` items -> (size, B, form or None)."""
    out = []
    for item in text.split(","):
        if item:
            f = item.split(":")
            out.append((int(f[0]), int(f[1]), f[2] if len(f) > 2 else None))
    return out


def key_of(size, batch, form):
    return f"potts{size}:{batch}:{form or 'default'}"


def potts_batch(size, batch, seed):
    """The arguments of ADMMBatchState for `batch` instances of the Potts size x size LP (instance 0 unperturbed)."""
    from pysparselp_amd.problems import potts_lp

    lp, _, pix, _ = potts_lp(size)
    cs = np.tile(lp.costsvector, (batch, 1))
    cs[1:, :pix.size] += 0.3 * np.random.RandomState(seed + batch).randn(batch - 1, pix.size)   # the unary costs come first
    return cs, None, None, lp.a_inequalities, lp.b_lower, lp.b_upper, lp.lower_bounds, lp.upper_bounds


def batch_state(problem, form):
    from bench_admm_batch import batch_state as forced

    return forced(problem[0], problem[1:], form, None)


def pick_k(lib, state, iters, warmup, seconds):
    state.iterate(warmup)
    per_it = timed_iterate(lib, state, 8) / 8   # one measurement near `seconds`
    return int(max(8, min(iters, 1e3 * seconds / max(per_it, 1e-6))))


# ---------------------------------------------------------------------------------------------------- (a) unarmed, per library
def rates_unarmed(args):
    """Instance-iterations/s of `iterate(k)` on a never-armed state for every set: one measurement each, in this process, with the
    package and the library of whichever checkout --repo names."""
    from pysparselp_amd import _lib

    lib = _lib.lib()
    out = {}
    for size, batch, form in sets_of(args.sets):
        st = batch_state(potts_batch(size, batch, args.seed), form)
        k = pick_k(lib, st, args.iters, args.warmup, args.seconds)
        out[key_of(size, batch, form)] = batch * k * 1e3 / timed_iterate(lib, st, k)
        st.close()
    return out


def part_unarmed(args):
    def child(repo):
        cmd = [sys.executable, os.path.abspath(__file__), "--child-unarmed", "--repo", os.path.abspath(repo), "--sets", args.sets,
               "--iters", str(args.iters), "--warmup", str(args.warmup), "--seconds", str(args.seconds), "--seed", str(args.seed)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, check=True, timeout=600)
        rates = json.loads(done.stdout.decode().strip().splitlines()[-1])
        print(f"[unarmed] {os.path.relpath(repo)}: " + ", ".join(f"{key} {v:.0f}" for key, v in rates.items()), file=sys.stderr, flush=True)
        return rates

    runs = {"parent": [], "this": []}
    for _ in range(args.repeats):   # alternating, one process at a time
        if args.parent_repo:
            runs["parent"].append(child(args.parent_repo))
        runs["this"].append(child(REPO))
    points = []
    for key in runs["this"][0]:
        name, batch, form = key.split(":")
        point = {"set": name, "B": int(batch), "form": form, "this_instance_it_per_s": summary([r[key] for r in runs["this"]])}
        if runs["parent"]:
            point["parent_instance_it_per_s"] = summary([r[key] for r in runs["parent"]])
            point["this_over_parent"] = point["this_instance_it_per_s"]["median"] / point["parent_instance_it_per_s"]["median"]
            point["bar"] = 1.0 - point["parent_instance_it_per_s"]["spread"]
            point["inside_bar"] = bool(point["this_over_parent"] >= point["bar"])
        points.append(point)
        print(f"[unarmed] {key}: {point['this_instance_it_per_s']['median']:.0f} instance-it/s, ratio to parent "
              f"{point.get('this_over_parent')}, bar {point.get('bar')}", file=sys.stderr)
    return {"parent_measured": bool(args.parent_repo), "points": points}


# ---------------------------------------------------------------------------------------------------- (b) the price of the test
def part_price(args, lib):
    points = []
    for size, batch, form in sets_of(args.price):
        problem = potts_batch(size, batch, args.seed)
        states = {"off": batch_state(problem, form), "every_1": batch_state(problem, form), "every_10": batch_state(problem, form)}
        states["every_1"].set_stop(0.0, 0.0, 1)
        states["every_10"].set_stop(0.0, 0.0, 10)
        k = pick_k(lib, states["off"], args.iters, args.warmup, args.seconds)
        for key in ("every_1", "every_10"):
            states[key].iterate(args.warmup + 8)
        rate = {key: [] for key in states}
        for _ in range(args.repeats):   # alternating
            for key, st in states.items():
                rate[key].append(batch * k * 1e3 / timed_iterate(lib, st, k))
        point = {"set": f"potts{size}", "B": batch, "form": states["off"].form(), "iterations_per_measurement": k}
        for key, st in states.items():
            point[f"{key}_instance_it_per_s"] = summary(rate[key])
            if key != "off":
                iterations, stopped = st.stop_state()[:2]
                point[f"{key}_stopped"] = int(stopped.sum())
                point[f"{key}_iterations"] = [int(iterations.min()), int(iterations.max())]
                point[f"{key}_over_off"] = point[f"{key}_instance_it_per_s"]["median"] / float(np.median(rate["off"]))
            st.close()
        points.append(point)
        print(f"[price] potts{size} B={batch} {point['form']}: off {np.median(rate['off']):.0f} instance-it/s, check_every 1 "
              f"x{point['every_1_over_off']:.3f} ({point['every_1_stopped']} stopped), 10 x{point['every_10_over_off']:.3f} "
              f"({point['every_10_stopped']} stopped)", file=sys.stderr)
    return {"points": points}


# ---------------------------------------------------------------------------------------------------- (c) what it buys
def part_buys(args):
    from pysparselp_amd import lp_admm_batch, lp_admm_batch_until

    points = []
    for size, batch, form in sets_of(args.buys):
        problem = potts_batch(size, batch, args.seed)
        if form:
            os.environ["SLP_ADMM_BATCH_FORM"] = form
        wall, infos = [], []
        for _ in range(args.repeats):
            start = time.perf_counter()
            _, info = lp_admm_batch_until(*problem, args.tol, args.tol, args.check_every, nb_iter=args.horizon, nb_iter_plot=args.plot)
            wall.append(time.perf_counter() - start)
            infos.append(info)
        info = infos[0]
        assert all(np.array_equal(i["iterations"], info["iterations"]) for i in infos)
        t = info["iterations"].astype(np.float64)
        point = {"set": f"potts{size}", "B": batch, "form": form or "default", "tol": args.tol, "check_every": args.check_every,
                 "horizon": args.horizon, "report_every": args.plot, "stopped": int(info["stopped"].sum()),
                 "stopping_iterations": [int(v) for v in info["iterations"]], "work_ratio": float(t.sum() / (batch * t.max())),
                 "until_wall_s": summary(wall)}
        if info["stopped"].all():
            last = int(t.max())
            plain = []
            for _ in range(args.repeats):
                start = time.perf_counter()
                lp_admm_batch(*problem, nb_iter=last, nb_iter_plot=args.plot)
                plain.append(time.perf_counter() - start)
            point["plain_wall_s_for_the_last_stop"] = summary(plain)
            point["until_over_plain_wall"] = point["until_wall_s"]["median"] / point["plain_wall_s_for_the_last_stop"]["median"]
        else:
            point["note"] = "not every instance stops within the horizon: no comparison of wall times"
        os.environ.pop("SLP_ADMM_BATCH_FORM", None)
        points.append(point)
        print(f"[buys] potts{size} B={batch}: {point['stopped']} stopped, iterations {int(t.min())}..{int(t.max())}, work ratio "
              f"{point['work_ratio']:.3f}, until {point['until_wall_s']['median']:.3f} s, plain "
              f"{point.get('plain_wall_s_for_the_last_stop', {}).get('median')}", file=sys.stderr)
    return {"points": points}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("outdir", nargs="?")
    p.add_argument("--parts", default="a,b,c")
    p.add_argument("--parent-repo", default="")
    p.add_argument("--repo", default="")
    p.add_argument("--sets", default="256:1:tile,256:1:levels,256:8:tile,256:8:levels,256:64:tile,256:64:levels,50:64,50:256")
    p.add_argument("--price", default="256:64:tile,256:64:levels,50:64")
    p.add_argument("--buys", default="50:64,50:256")
    p.add_argument("--tol", type=float, default=1e-2)
    p.add_argument("--check-every", type=int, default=10)
    p.add_argument("--horizon", type=int, default=3000)
    p.add_argument("--plot", type=int, default=100)
    p.add_argument("--iters", type=int, default=2000)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--seconds", type=float, default=0.3)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--child-unarmed", action="store_true")
    args = p.parse_args()
    assert args.repeats >= 1 and args.iters >= 8

    if args.child_unarmed:
        if args.repo:   # ahead of this checkout: the package and the library of that one
            sys.path[:0] = [args.repo]
        print(json.dumps(rates_unarmed(args)))
        return
    assert args.outdir, "OUTDIR is missing"
    parts = args.parts.split(",")
    out = {"method": "lp_admm_batch_until", "box": platform.node(), "device": "AMD Instinct MI355X (gfx950)",
           "iterations": args.iters, "warmup": args.warmup, "repeats": args.repeats}
    if "a" in parts:   # before this process opens the GPU: one process with the device at a time
        out["unarmed_against_parent"] = part_unarmed(args)
    if "b" in parts or "c" in parts:
        from pysparselp_amd import _lib

        lib = _lib.lib()
        if "b" in parts:
            out["price_of_the_test"] = part_price(args, lib)
        if "c" in parts:
            out["what_it_buys"] = part_buys(args)
    line = json.dumps(out)
    print(line)
    os.makedirs(args.outdir, exist_ok=True)
    with open(os.path.join(args.outdir, "admm_batch_stop.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
