"""The per-LP stopping test of the Chambolle-Pock list solver (CPManyState.set_stop, csrc/slp_cp_many.hip): what it costs when it
is off, what the test itself costs, and what stopping buys on a mixed list.

    python tools/bench_cp_many_stop.py OUTDIR [--parts a,b,c] [--parent-repo DIR] [--counts-sc105 1,16,256,1024]
                                              [--counts-potts50 1,16,256] [--counts-price 256,1024] [--mixed 256] [--tol 1e-2]
                                              [--check-every 10] [--iters 2000] [--warmup 200] [--repeats 3] [--seconds 0.3]
    python tools/bench_cp_many_stop.py --cpu-check [--tol 1e-2] [--check-every 10] [--mixed 256]      (needs no GPU)

Writes one JSON line (stdout and OUTDIR/cp_many_stop.json).  All times are between two HIP events on the library's stream
(slp_timer_start / slp_timer_stop) except the wall times of part (c); every figure is the median of `repeats` measurements that
alternate between the variants compared, with every repeat and the spread ((max - min) / median) recorded beside it.

  (a) off       `iterate(k)` with the test off, LP-iterations/s over the sets of tools/bench_cp_many.py, against the PARENT
                commit's library on the same box.  Two libraries cannot share a process, so this part alone alternates between
                child processes (one at a time): `repeats` x (parent, this).  --parent-repo names a built checkout of the
                parent commit (its package, its library, its tests/golden); the same measuring code of this file runs on it.
                Without it only this library is measured and the comparison is null.
                Recorded: both rates, the parent's own spread between its repeats, the ratio of the medians.
  (b) price     one process: the SC105 set with the test off, armed with tol = 0 and check_every = 1, and with check_every =
                10 (tol = 0 never stops an LP that reaches no exact fixed point; `stopped` records that none did).  Recorded: the
                three rates and the two ratios armed / off.
  (c) buys      a mixed list of `--mixed` LPs in rotation: the package's Potts LPs of 8 x 8 to 16 x 16, the golden random0..2 and
                SC105.  t_k = the stopping iteration of LP k at (--tol, --check-every); the tolerance is one at which every LP
                of the list stops on the CPU restatement (tests/cp_stop_cpu.py; `--cpu-check` prints the t_k and needs no GPU).
                Wall time of chambolle_pock_ppd_many_until until every LP is stopped against chambolle_pock_ppd_many run for
                max_k t_k iterations -- the count a user needs today for the same result -- and the work ratio
                sum_k t_k / (N max_k t_k), which needs no GPU.
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

from _bench_util import spread  # noqa: E402
from bench_cp_many import perturbed, timed_iterate  # noqa: E402
sys.path.insert(0, os.path.join(REPO, "tests"))


def summary(values):
    return {"median": float(np.median(values)), "repeats": [float(v) for v in values], "spread": spread(values)}


def fixture(name):
    from conftest import load_golden
    from test_oracle_golden import _reduced

    return _reduced(load_golden("lp_" + name))


def many_state(problems):
    from pysparselp_amd.ChambollePockPPD import CPManyState, _many_problem

    return CPManyState([_many_problem(k, p) for k, p in enumerate(problems)])


def pick_k(lib, state, iters, warmup, seconds):
    state.iterate(warmup)
    per_it = timed_iterate(lib, state, 32) / 32   # one measurement near `seconds`
    return int(max(32, min(iters, 1e3 * seconds / max(per_it, 1e-6))))


# ---------------------------------------------------------------------------------------------------- (a) off, per library
def rates_off(args):
    """LP-iterations/s of `iterate(k)` with the test off (the state after create) for every set and count: one measurement
    each, in this process, with the package and the library of whichever checkout --repo names."""
    from pysparselp_amd import _lib

    lib = _lib.lib()
    out = {}
    for name in ("sc105", "potts50"):
        for count in [int(v) for v in getattr(args, "counts_" + name).split(",")]:
            st = many_state(perturbed(fixture(name), count, args.seed + count))
            k = pick_k(lib, st, args.iters, args.warmup, args.seconds)
            out[f"{name}:{count}"] = count * k * 1e3 / timed_iterate(lib, st, k)
            st.close()
    return out


def part_off(args):
    def child(repo):
        cmd = [sys.executable, os.path.abspath(__file__), "--child-rates-off", "--repo", os.path.abspath(repo), "--counts-sc105",
               args.counts_sc105, "--counts-potts50", args.counts_potts50, "--iters", str(args.iters), "--warmup", str(args.warmup),
               "--seconds", str(args.seconds), "--seed", str(args.seed)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, check=True, timeout=600)
        rates = json.loads(done.stdout.decode().strip().splitlines()[-1])
        print(f"[off] {os.path.relpath(repo)}: " + ", ".join(f"{key} {v:.0f}" for key, v in rates.items()), file=sys.stderr, flush=True)
        return rates

    runs = {"parent": [], "this": []}
    for _ in range(args.repeats):   # alternating, one process at a time
        if args.parent_repo:
            runs["parent"].append(child(args.parent_repo))
        runs["this"].append(child(REPO))
    points = []
    for key in runs["this"][0]:
        name, count = key.split(":")
        point = {"set": name, "N": int(count), "this_lp_it_per_s": summary([r[key] for r in runs["this"]])}
        if runs["parent"]:
            point["parent_lp_it_per_s"] = summary([r[key] for r in runs["parent"]])
            point["this_over_parent"] = point["this_lp_it_per_s"]["median"] / point["parent_lp_it_per_s"]["median"]
            point["beyond_parent_spread"] = bool(abs(point["this_over_parent"] - 1.0) > point["parent_lp_it_per_s"]["spread"])
        points.append(point)
        print(f"[off] {key}: {point['this_lp_it_per_s']['median']:.0f} LP-it/s, ratio to parent {point.get('this_over_parent')}", file=sys.stderr)
    return {"parent_measured": bool(args.parent_repo), "points": points}


# ---------------------------------------------------------------------------------------------------- (b) the price of the test
def part_price(args, lib):
    points = []
    for count in [int(v) for v in args.counts_price.split(",")]:
        problems = perturbed(fixture("sc105"), count, args.seed + count)
        states = {"off": many_state(problems), "every_1": many_state(problems), "every_10": many_state(problems)}
        states["every_1"].set_stop(0.0, 1)
        states["every_10"].set_stop(0.0, 10)
        k = pick_k(lib, states["off"], args.iters, args.warmup, args.seconds)
        for key in ("every_1", "every_10"):
            states[key].iterate(args.warmup + 32)
        rate = {key: [] for key in states}
        for _ in range(args.repeats):   # alternating
            for key, st in states.items():
                rate[key].append(count * k * 1e3 / timed_iterate(lib, st, k))
        point = {"set": "sc105", "N": count, "iterations_per_measurement": k}
        for key, st in states.items():
            point[f"{key}_lp_it_per_s"] = summary(rate[key])
            if key != "off":
                iterations, stopped, _ = st.stop_state()
                point[f"{key}_stopped"] = int(stopped.sum())
                point[f"{key}_iterations"] = [int(iterations.min()), int(iterations.max())]
                point[f"{key}_over_off"] = point[f"{key}_lp_it_per_s"]["median"] / float(np.median(rate["off"]))
            st.close()
        points.append(point)
        print(f"[price] N={count}: off {np.median(rate['off']):.0f} LP-it/s, check_every 1 x{point['every_1_over_off']:.3f}, "
              f"10 x{point['every_10_over_off']:.3f}", file=sys.stderr)
    return {"points": points}


# ---------------------------------------------------------------------------------------------------- (c) what stopping buys
def mixed_kinds():
    """The distinct LPs of the mixed list: ``[(name, 8-tuple)]``."""
    import copy

    from pysparselp_amd.problems import potts_lp

    kinds = []
    for size in range(8, 17):
        lp = copy.deepcopy(potts_lp(size)[0])
        lp.remove_fixed_variables()
        kinds.append((f"potts{size}", (lp.costsvector, lp.a_equalities, lp.b_equalities, lp.a_inequalities, lp.b_lower, lp.b_upper,
                                       lp.lower_bounds, lp.upper_bounds)))
    return kinds + [(name, fixture(name)) for name in ("random0", "random1", "random2", "sc105")]


def cpu_stops(kinds, tol, every, horizon):
    """t_k of every distinct LP on the CPU restatement, ``None`` where it does not stop within ``horizon``."""
    import cp_stop_cpu

    out = {}
    for name, p in kinds:
        if p[1] is not None and p[1].shape[0] == 0:
            p = (p[0], None, None) + tuple(p[3:])
        out[name] = cp_stop_cpu.stopping_iteration(cp_stop_cpu.steps_of(*cp_stop_cpu.oracle_iterates(p, horizon)), tol, every)
    return out


def work_ratio(stops, count):
    t = np.array([stops[i % len(stops)] for i in range(count)], dtype=np.float64)
    return float(t.sum() / (count * t.max()))


def part_buys(args):
    from pysparselp_amd import chambolle_pock_ppd_many, chambolle_pock_ppd_many_until

    kinds = mixed_kinds()
    problems = [kinds[i % len(kinds)][1] for i in range(args.mixed)]
    wall = {"until": [], "fixed": []}
    t_max = None
    for rep in range(args.repeats + 1):   # the first round warms both up and fixes max t_k; alternating
        start = time.perf_counter()
        _, _, info = chambolle_pock_ppd_many_until(problems, args.tol, args.check_every, nb_max_iter=args.horizon)
        until = time.perf_counter() - start
        assert info["stopped"].all(), "an LP of the mixed list did not stop: choose another tolerance (--cpu-check)"
        t_max = int(info["iterations"].max())
        start = time.perf_counter()
        chambolle_pock_ppd_many(problems, nb_max_iter=t_max)
        fixed = time.perf_counter() - start
        if rep:
            wall["until"].append(until)
            wall["fixed"].append(fixed)
    stops = [int(v) for v in info["iterations"][:len(kinds)]]
    out = {"N": args.mixed, "tol": args.tol, "check_every": args.check_every, "kinds": [name for name, _ in kinds],
           "stopping_iterations": stops, "max_iterations": t_max, "work_ratio": work_ratio(stops, args.mixed),
           "until_wall_s": summary(wall["until"]), "fixed_wall_s": summary(wall["fixed"])}
    out["fixed_over_until"] = out["fixed_wall_s"]["median"] / out["until_wall_s"]["median"]
    print(f"[buys] N={args.mixed}: until {out['until_wall_s']['median'] * 1e3:.1f} ms, {t_max} iterations for all "
          f"{out['fixed_wall_s']['median'] * 1e3:.1f} ms; work ratio {out['work_ratio']:.3f}", file=sys.stderr)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("outdir", nargs="?")
    p.add_argument("--parts", default="a,b,c")
    p.add_argument("--parent-repo", default="")
    p.add_argument("--repo", default="")
    p.add_argument("--counts-sc105", default="1,16,256,1024")
    p.add_argument("--counts-potts50", default="1,16,256")
    p.add_argument("--counts-price", default="256,1024")
    p.add_argument("--mixed", type=int, default=256)
    p.add_argument("--tol", type=float, default=1e-2)
    p.add_argument("--check-every", type=int, default=10)
    p.add_argument("--horizon", type=int, default=2000)
    p.add_argument("--iters", type=int, default=2000)
    p.add_argument("--warmup", type=int, default=200)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--seconds", type=float, default=0.3)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--cpu-check", action="store_true")
    p.add_argument("--child-rates-off", action="store_true")
    args = p.parse_args()
    assert args.repeats >= 1 and args.iters >= 32

    if args.child_rates_off:
        if args.repo:   # ahead of this checkout: the package, the library and the fixtures of that one
            sys.path[:0] = [args.repo, os.path.join(args.repo, "tests")]
        print(json.dumps(rates_off(args)))
        return
    if args.cpu_check:
        kinds = mixed_kinds()
        stops = cpu_stops(kinds, args.tol, args.check_every, args.horizon)
        reached = all(t is not None for t in stops.values())
        print(json.dumps({"tol": args.tol, "check_every": args.check_every, "horizon": args.horizon, "stopping_iterations": stops,
                          "all_stop": reached, "work_ratio": work_ratio(list(stops.values()), args.mixed) if reached else None}))
        return
    assert args.outdir, "OUTDIR is missing"
    parts = args.parts.split(",")
    out = {"method": "chambolle_pock_ppd_many_until", "box": platform.node(), "device": "AMD Instinct MI355X (gfx950)",
           "iterations": args.iters, "warmup": args.warmup, "repeats": args.repeats}
    if "a" in parts:   # before this process opens the GPU: one process with the device at a time
        out["off_against_parent"] = part_off(args)
    if "b" in parts or "c" in parts:
        from pysparselp_amd import _lib

        lib = _lib.lib()
        if "b" in parts:
            out["price_of_the_test"] = part_price(args, lib)
        if "c" in parts:
            out["what_stopping_buys"] = part_buys(args)
    line = json.dumps(out)
    print(line)
    os.makedirs(args.outdir, exist_ok=True)
    with open(os.path.join(args.outdir, "cp_many_stop.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
