"""The certificate as the per-instance stopping test of the batched Chambolle-Pock solver (CPBatchState.set_stop_gap,
csrc/slp_cp_batch.hip): what it costs when it was never armed, what the armed test costs, and what it buys.

    python tools/bench_cp_batch_gap.py OUTDIR [--parts a,b,c] [--parent-repo DIR] [--sets 256:1,256:8,256:64,256:256,50:64]
                                              [--price 256:64,256:256] [--buys 256:64,256:256] [--tol 1e-2] [--check-every 10]
                                              [--horizon 20000] [--iters 2000] [--warmup 200] [--repeats 3] [--seconds 0.3]

Writes one JSON line (stdout and OUTDIR/cp_batch_gap.json).  The measuring code is that of tools/bench_cp_many_gap.py: times
between two HIP events on the library's stream, a warm-up, `repeats` measurements that alternate between the variants compared,
the median with every repeat and the spread ((max - min) / median) beside it.  A set is `potts size:B`: the Potts n x n LP of
tools/bench_cp_batch.py with B seeded perturbations of the unary costs.

  (a) unarmed   `iterate(k)` on a state that was never armed, instance-iterations/s, against the PARENT commit's library
                (--parent-repo: a built checkout), alternating child processes, parent then this.  The bar is fixed before the
                run: this median >= parent median x (1 - the parent's own spread between its repeats), per set.
  (b) price     one process per set: no test, and the certificate armed at both tolerances 0 with check_every 1 and 10.  Two
                cadences give two equations: in units of an unarmed iteration, t1 = 1 + i + c and t10 = 1 + i + c / 10, with i
                what an armed (masked) iteration costs beyond an unarmed one and c what a check costs.  Instances that reach
                gap 0 and violation 0 exactly within --screen iterations would stop: they are passed over, and counted.  No bar.
  (c) buys      distinct costs at (--tol, --tol), check_every --check-every, --horizon iterations: per-instance stopping
                iterations, the work ratio sum_k t_k / (B max_k t_k), per tile of 64 instances the iterations it spent wholly
                stopped (its blocks then retire at their first load), and the wall time of chambolle_pock_ppd_batch_certified
                against chambolle_pock_ppd_batch for max_k t_k iterations, both reporting every --plot iterations.  No bar.
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
    return [tuple(int(v) for v in item.split(":")) for item in text.split(",") if item]


def potts_batch(size, batch, seed):
    """The arguments of CPBatchState for `batch` instances of the Potts size x size LP (instance 0 unperturbed)."""
    from pysparselp_amd.ChambollePockPPD import one_sided_system
    from pysparselp_amd.problems import potts_lp

    lp, _, pix, _ = potts_lp(size)
    ineq, b = one_sided_system(lp.a_inequalities, lp.b_lower, lp.b_upper)
    cs = np.tile(lp.costsvector, (batch, 1))
    cs[1:, :pix.size] += 0.3 * np.random.RandomState(seed + batch).randn(batch - 1, pix.size)   # the unary costs come first
    return cs, ineq, b, lp.lower_bounds, lp.upper_bounds


def batch_state(cs, ineq, b, lb, ub):
    from pysparselp_amd.ChambollePockPPD import CPBatchState

    return CPBatchState(cs, None, None, ineq, b, lb, ub, None, 1, 1)


def pick_k(lib, state, iters, warmup, seconds):
    state.iterate(warmup)
    per_it = timed_iterate(lib, state, 32) / 32   # one measurement near `seconds`
    return int(max(32, min(iters, 1e3 * seconds / max(per_it, 1e-6))))


# ---------------------------------------------------------------------------------------------------- (a) unarmed, per library
def rates_unarmed(args):
    """Instance-iterations/s of `iterate(k)` on a never-armed state for every set: one measurement each, in this process, with the
    package and the library of whichever checkout --repo names."""
    from pysparselp_amd import _lib

    lib = _lib.lib()
    out = {}
    for size, batch in sets_of(args.sets):
        st = batch_state(*potts_batch(size, batch, args.seed))
        k = pick_k(lib, st, args.iters, args.warmup, args.seconds)
        out[f"potts{size}:{batch}"] = batch * k * 1e3 / timed_iterate(lib, st, k)
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
        name, batch = key.split(":")
        point = {"set": name, "B": int(batch), "this_instance_it_per_s": summary([r[key] for r in runs["this"]])}
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
def never_stopping(size, batch, seed, screen):
    """The arguments of `batch` instances, drawn from batch + batch // 4, that do not stop at both tolerances 0 and check_every = 1
    within `screen` iterations, and how many were passed over."""
    cs, ineq, b, lb, ub = potts_batch(size, batch + batch // 4, seed)
    st = batch_state(cs, ineq, b, lb, ub)
    st.set_stop_gap(0.0, 0.0, 1)
    st.iterate(screen)
    stopped = st.gap_state()[1]
    st.close()
    keep = np.nonzero(~stopped)[0][:batch]
    assert keep.size == batch, "too many instances reach gap 0 exactly"
    return (np.ascontiguousarray(cs[keep]), ineq, b, lb, ub), int(stopped[:keep[-1] + 1].sum())


def part_price(args, lib):
    points = []
    for size, batch in sets_of(args.price):
        problem, passed_over = never_stopping(size, batch, args.seed, args.screen)
        states = {"off": batch_state(*problem), "every_1": batch_state(*problem), "every_10": batch_state(*problem)}
        states["every_1"].set_stop_gap(0.0, 0.0, 1)
        states["every_10"].set_stop_gap(0.0, 0.0, 10)
        k = pick_k(lib, states["off"], args.iters, args.warmup, args.seconds)
        for key in ("every_1", "every_10"):
            states[key].iterate(args.warmup + 32)
        rate = {key: [] for key in states}
        for _ in range(args.repeats):   # alternating
            for key, st in states.items():
                rate[key].append(batch * k * 1e3 / timed_iterate(lib, st, k))
        point = {"set": f"potts{size}", "B": batch, "iterations_per_measurement": k, "screen_iterations": args.screen,
                 "passed_over": passed_over}
        for key, st in states.items():
            point[f"{key}_instance_it_per_s"] = summary(rate[key])
            if key != "off":
                iterations, stopped = st.gap_state()[:2]
                point[f"{key}_stopped"] = int(stopped.sum())
                point[f"{key}_iterations"] = [int(iterations.min()), int(iterations.max())]
                point[f"{key}_over_off"] = point[f"{key}_instance_it_per_s"]["median"] / float(np.median(rate["off"]))
            st.close()
        t1, t10 = 1.0 / point["every_1_over_off"], 1.0 / point["every_10_over_off"]   # in units of an unarmed iteration
        point["cost_per_check"] = (t1 - t10) / 0.9
        point["cost_per_iteration"] = t10 - 1.0 - point["cost_per_check"] / 10.0
        points.append(point)
        print(f"[price] potts{size} B={batch}: off {np.median(rate['off']):.0f} instance-it/s, check_every 1 x{point['every_1_over_off']:.3f}, "
              f"10 x{point['every_10_over_off']:.3f}; per iteration {point['cost_per_iteration']:+.4f}, per check "
              f"{point['cost_per_check']:+.4f} of an unarmed iteration", file=sys.stderr)
    return {"points": points}


# ---------------------------------------------------------------------------------------------------- (c) what it buys
def part_buys(args):
    from pysparselp_amd import chambolle_pock_ppd_batch, chambolle_pock_ppd_batch_certified
    from pysparselp_amd.problems import potts_lp

    points = []
    for size, batch in sets_of(args.buys):
        lp, _, _, _ = potts_lp(size)
        cs = potts_batch(size, batch, args.seed)[0]
        common = (None, None, lp.a_inequalities, lp.b_lower, lp.b_upper, lp.lower_bounds, lp.upper_bounds)
        wall, infos = [], []
        for _ in range(args.repeats):
            start = time.perf_counter()
            _, _, info = chambolle_pock_ppd_batch_certified(cs, *common, args.tol, args.tol, args.check_every, nb_max_iter=args.horizon,
                                                            nb_iter_plot=args.plot)
            wall.append(time.perf_counter() - start)
            infos.append(info)
        info = infos[0]
        assert all(np.array_equal(i["iterations"], info["iterations"]) for i in infos)
        t = info["iterations"].astype(np.float64)
        point = {"set": f"potts{size}", "B": batch, "tol": args.tol, "check_every": args.check_every, "horizon": args.horizon,
                 "report_every": args.plot, "stopped": int(info["stopped"].sum()), "stopping_iterations": [int(v) for v in info["iterations"]],
                 "work_ratio": float(t.sum() / (batch * t.max())), "certified_wall_s": summary(wall)}
        if info["stopped"].all():
            last = int(t.max())
            tiles = [info["iterations"][i:i + 64] for i in range(0, batch, 64)]
            point["tile_last_stop"] = [int(v.max()) for v in tiles]
            point["tile_iterations_wholly_stopped"] = [last - int(v.max()) for v in tiles]
            point["tile_launch_share_saved"] = float(sum(last - int(v.max()) for v in tiles) / (len(tiles) * last))
            plain = []
            for _ in range(args.repeats):
                start = time.perf_counter()
                chambolle_pock_ppd_batch(cs, *common, nb_max_iter=last, nb_iter_plot=args.plot)
                plain.append(time.perf_counter() - start)
            point["plain_wall_s_for_the_last_stop"] = summary(plain)
            point["certified_over_plain_wall"] = point["certified_wall_s"]["median"] / point["plain_wall_s_for_the_last_stop"]["median"]
        else:
            point["note"] = "not every instance stops within the horizon: no comparison of wall times"
        points.append(point)
        print(f"[buys] potts{size} B={batch}: {point['stopped']} stopped, iterations {int(t.min())}..{int(t.max())}, work ratio "
              f"{point['work_ratio']:.3f}, certified {point['certified_wall_s']['median']:.3f} s, plain "
              f"{point.get('plain_wall_s_for_the_last_stop', {}).get('median')}", file=sys.stderr)
    return {"points": points}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("outdir", nargs="?")
    p.add_argument("--parts", default="a,b,c")
    p.add_argument("--parent-repo", default="")
    p.add_argument("--repo", default="")
    p.add_argument("--sets", default="256:1,256:8,256:64,256:256,50:64")
    p.add_argument("--price", default="256:64,256:256")
    p.add_argument("--buys", default="256:64,256:256")
    p.add_argument("--tol", type=float, default=1e-2)
    p.add_argument("--check-every", type=int, default=10)
    p.add_argument("--horizon", type=int, default=20000)
    p.add_argument("--plot", type=int, default=100)
    p.add_argument("--screen", type=int, default=3000)
    p.add_argument("--iters", type=int, default=2000)
    p.add_argument("--warmup", type=int, default=200)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--seconds", type=float, default=0.3)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--child-unarmed", action="store_true")
    args = p.parse_args()
    assert args.repeats >= 1 and args.iters >= 32

    if args.child_unarmed:
        if args.repo:   # ahead of this checkout: the package and the library of that one
            sys.path[:0] = [args.repo]
        print(json.dumps(rates_unarmed(args)))
        return
    assert args.outdir, "OUTDIR is missing"
    parts = args.parts.split(",")
    out = {"method": "chambolle_pock_ppd_batch_certified", "box": platform.node(), "device": "AMD Instinct MI355X (gfx950)",
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
    with open(os.path.join(args.outdir, "cp_batch_gap.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
