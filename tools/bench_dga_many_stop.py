"""The per-LP stopping test of dual gradient ascent on a list (DeviceDGAMany.set_stop, csrc/slp_dga_many.hip): what it costs when it
is off, what the test itself costs, and what stopping buys on a mixed list.

    python tools/bench_dga_many_stop.py OUTDIR [--parts a,b,c] [--parent-repo DIR] [--counts 1,8,64,256,1024] [--counts-price 256,1024]
                                               [--mixed 256] [--tol 1e-2] [--check-every 10] [--horizon 1000]
                                               [--iters 400] [--warmup 20] [--repeats 3] [--seconds 0.3] [--screen 1500]

Writes one JSON line (stdout and OUTDIR/dga_many_stop.json).  All times are between two HIP events on the library's stream
(slp_timer_start / slp_timer_stop, the draw buffers filled beforehand) except the wall times of part (c); every figure is the median
of `repeats` measurements that alternate between the variants compared, with every repeat and the spread ((max - min) / median)
recorded beside it.

  (a) off       `iterate(k)` with the test off, instance-iterations/s on the Potts lists of tools/bench_dga_many.py, against the
                PARENT commit's library on the same box.  Two libraries cannot share a process, so this part alone alternates
                between child processes (one at a time): `repeats` x (parent, this).  --parent-repo names a built checkout of the
                parent commit (its package, its library); the same measuring code of this file runs on it.  Without it only this
                library is measured and the comparison is null.  The bar, per N: this median >= the parent's median x (1 - the
                parent's own spread between its repeats), the only noise figure the run has (`inside_bar`; `within_1_percent_of_bar`
                marks a point that close to it on either side).
  (b) price     one process: a Potts list with the test off, armed with tolerance 0 at check_every = 1, and at check_every = 10.
                Tolerance 0 still stops an LP that reaches an exact fixed point, and a stopped LP costs nothing: the list is drawn
                from a longer one by a screening run of `--screen` iterations at check_every = 1 that passes those over
                (`screened_out`; `stopped` records that none of the measured LPs did stop).  An armed `iterate` call reads the stop
                records back before it launches (nothing is launched once no LP moves); that is part of the price.  Recorded: the
                three rates and the two ratios armed / off.
  (c) buys      a mixed list of `--mixed` LPs in rotation: the Potts LPs of 8 x 8 to 16 x 16 and the six small golden LPs.  t_k =
                the iterations LP k ran (its stopping iteration; `--horizon` for one that did not stop, `all_stopped` says whether
                any did not).  Wall time of dual_gradient_ascent_many_until against dual_gradient_ascent_many run for max_k t_k
                iterations -- the count a user needs without the test for the same multipliers -- both with their set-up, and the
                work ratio sum_k t_k / (N max_k t_k).
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
from bench_dga_many import LP, potts_list, timed  # noqa: E402
sys.path.insert(0, os.path.join(REPO, "tests"))

GRIDS = [8, 9, 10, 11, 12, 13, 14, 15, 16]
GOLDEN = ("sc50a", "sc105", "potts8", "random0", "random1", "random2")


def summary(values):
    return {"median": float(np.median(values)), "repeats": [float(v) for v in values], "spread": spread(values)}


def many_state(lps):
    from pysparselp_amd.DualGradientAscent import DeviceDGAMany, _dga_many_lp, dga_many_start

    forms = [_dga_many_lp(k, lp) for k, lp in enumerate(lps)]
    y0s, offsets = dga_many_start(forms)
    return DeviceDGAMany(forms, y0s, offsets)


def pick_k(lib, state, iters, warmup, seconds):
    state.iterate(warmup)
    per_it = timed(lib, [state], 8) / 8   # one measurement near `seconds`
    return int(max(8, min(iters, 1e3 * seconds / max(per_it, 1e-6))))


# ---------------------------------------------------------------------------------------------------- (a) off, per library
def rates_off(args):
    """Instance-iterations/s of `iterate(k)` with the test off (the state after create) for every count: one measurement each,
    in this process, with the package and the library of whichever checkout --repo names."""
    from pysparselp_amd import _lib

    lib = _lib.lib()
    out = {}
    for count in [int(v) for v in args.counts.split(",")]:
        st = many_state(potts_list(count, GRIDS))
        k = pick_k(lib, st, args.iters, args.warmup, args.seconds)
        out[str(count)] = count * k * 1e3 / timed(lib, [st], k)
        st.close()
    return out


def part_off(args):
    def child(repo):
        cmd = [sys.executable, os.path.abspath(__file__), "--child-rates-off", "--repo", os.path.abspath(repo), "--counts", args.counts,
               "--iters", str(args.iters), "--warmup", str(args.warmup), "--seconds", str(args.seconds)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, check=True, timeout=600)
        rates = json.loads(done.stdout.decode().strip().splitlines()[-1])
        print(f"[off] {os.path.relpath(repo)}: " + ", ".join(f"N={key} {v:.0f}" for key, v in rates.items()), file=sys.stderr, flush=True)
        return rates

    runs = {"parent": [], "this": []}
    for _ in range(args.repeats):   # alternating, one process at a time
        if args.parent_repo:
            runs["parent"].append(child(args.parent_repo))
        runs["this"].append(child(REPO))
    points = []
    for key in runs["this"][0]:
        point = {"set": "potts 8..16", "N": int(key), "this_instance_it_per_s": summary([r[key] for r in runs["this"]])}
        if runs["parent"]:
            parent = point["parent_instance_it_per_s"] = summary([r[key] for r in runs["parent"]])
            point["this_over_parent"] = point["this_instance_it_per_s"]["median"] / parent["median"]
            point["bar"] = 1.0 - parent["spread"]
            point["inside_bar"] = bool(point["this_over_parent"] >= point["bar"])
            point["within_1_percent_of_bar"] = bool(abs(point["this_over_parent"] - point["bar"]) <= 0.01)
        points.append(point)
        print(f"[off] N={key}: {point['this_instance_it_per_s']['median']:.0f} instance-it/s, ratio to parent {point.get('this_over_parent')}, "
              f"bar {point.get('bar')}", file=sys.stderr)
    return {"parent_measured": bool(args.parent_repo), "points": points}


# ---------------------------------------------------------------------------------------------------- (b) the price of the test
def never_stopping(lps, count, screen):
    """The first `count` of `lps` that reach no exact fixed point (step 0, where even tolerance 0 stops an LP) within `screen`
    iterations, and how many were passed over: an LP that has not stopped at check_every = 1 by then has not stopped at any
    cadence either."""
    st = many_state(lps)
    st.set_stop(0.0, 1)
    st.iterate(screen)
    stopped = st.stop_state()[1]
    st.close()
    keep, passed_over = [], 0
    for lp, gone in zip(lps, stopped):
        if len(keep) == count:
            break
        if gone:
            passed_over += 1
        else:
            keep.append(lp)
    assert len(keep) == count, "too many LPs of the list reach an exact fixed point"
    return keep, passed_over


def part_price(args, lib):
    points = []
    for count in [int(v) for v in args.counts_price.split(",")]:
        lps, screened_out = never_stopping(potts_list(count + count // 4, GRIDS), count, args.screen)
        states = {"off": many_state(lps), "every_1": many_state(lps), "every_10": many_state(lps)}
        states["every_1"].set_stop(0.0, 1)
        states["every_10"].set_stop(0.0, 10)
        k = pick_k(lib, states["off"], args.iters, args.warmup, args.seconds)
        assert args.screen >= 2 * (args.warmup + 8) + args.repeats * k, "--screen is shorter than the measurement"
        for key in ("every_1", "every_10"):
            states[key].iterate(args.warmup + 8)
        rate = {key: [] for key in states}
        for _ in range(args.repeats):   # alternating
            for key, st in states.items():
                rate[key].append(count * k * 1e3 / timed(lib, [st], k))
        point = {"set": "potts 8..16", "N": count, "iterations_per_measurement": k, "screen_iterations": args.screen,
                 "screened_out": screened_out}
        for key, st in states.items():
            point[f"{key}_instance_it_per_s"] = summary(rate[key])
            if key != "off":
                iterations, stopped, _ = st.stop_state()
                point[f"{key}_stopped"] = int(stopped.sum())
                point[f"{key}_iterations"] = [int(iterations.min()), int(iterations.max())]
                point[f"{key}_over_off"] = point[f"{key}_instance_it_per_s"]["median"] / float(np.median(rate["off"]))
            st.close()
        points.append(point)
        print(f"[price] N={count}: off {np.median(rate['off']):.0f} instance-it/s, check_every 1 x{point['every_1_over_off']:.3f}, "
              f"10 x{point['every_10_over_off']:.3f}", file=sys.stderr)
    return {"points": points}


# ---------------------------------------------------------------------------------------------------- (c) what stopping buys
def mixed_kinds():
    """The distinct LPs of the mixed list: ``[(name, LP)]``."""
    from conftest import load_golden
    from test_dga_host import dga_args

    kinds = [(f"potts{size}", lp) for size, lp in zip(GRIDS, potts_list(len(GRIDS), GRIDS))]
    return kinds + [("golden_" + name, LP(*dga_args(load_golden("lp_" + name)))) for name in GOLDEN]


def work_ratio(stops):
    t = np.array(stops, dtype=np.float64)
    return float(t.sum() / (t.size * t.max()))


def part_buys(args):
    from pysparselp_amd import dual_gradient_ascent_many, dual_gradient_ascent_many_until

    kinds = mixed_kinds()
    lps = [kinds[i % len(kinds)][1] for i in range(args.mixed)]
    wall = {"until": [], "fixed": []}
    t_max = None
    for rep in range(args.repeats + 1):   # the first round warms both up and fixes max t_k; alternating
        start = time.perf_counter()
        *_, info = dual_gradient_ascent_many_until(lps, args.tol, args.check_every, nb_max_iter=args.horizon)
        until = time.perf_counter() - start
        t_max = int(info["iterations"].max())
        start = time.perf_counter()
        dual_gradient_ascent_many(lps, nb_max_iter=t_max)
        fixed = time.perf_counter() - start
        if rep:
            wall["until"].append(until)
            wall["fixed"].append(fixed)
    stops = [int(v) for v in info["iterations"]]
    out = {"N": args.mixed, "tol": args.tol, "check_every": args.check_every, "horizon": args.horizon, "kinds": [name for name, _ in kinds],
           "iterations_of_the_kinds": stops[:len(kinds)], "stopped_of_the_kinds": [bool(v) for v in info["stopped"][:len(kinds)]],
           "all_stopped": bool(info["stopped"].all()), "max_iterations": t_max, "work_ratio": work_ratio(stops),
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
    p.add_argument("--counts", default="1,8,64,256,1024")
    p.add_argument("--counts-price", default="256,1024")
    p.add_argument("--mixed", type=int, default=256)
    p.add_argument("--tol", type=float, default=1e-2)
    p.add_argument("--check-every", type=int, default=10)
    p.add_argument("--horizon", type=int, default=1000)
    p.add_argument("--iters", type=int, default=400)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--seconds", type=float, default=0.3)
    p.add_argument("--screen", type=int, default=1500, help="part b: iterations of the screening run for LPs that reach a fixed point")
    p.add_argument("--child-rates-off", action="store_true")
    args = p.parse_args()
    assert args.repeats >= 1 and args.iters >= 8

    if args.child_rates_off:
        if args.repo:   # ahead of this checkout: the package and the library of that one
            sys.path[:0] = [args.repo]
        print(json.dumps(rates_off(args)))
        return
    assert args.outdir, "OUTDIR is missing"
    parts = args.parts.split(",")
    out = {"method": "dual_gradient_ascent_many_until", "box": platform.node(), "device": "AMD Instinct MI355X (gfx950)",
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
    with open(os.path.join(args.outdir, "dga_many_stop.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
