"""The certificate as the per-LP stopping test of the Chambolle-Pock list solver (CPManyState.set_stop_gap, csrc/slp_cp_many.hip):
what it costs when it is off, what the armed test costs, and what it changes against the step test on a mixed list.

    python tools/bench_cp_many_gap.py OUTDIR [--parts a,b,c] [--parent-repo DIR] [--counts-sc105 1,16,256,1024]
                                             [--counts-potts50 1,16,256] [--counts-price 256,1024] [--mixed 256] [--tol 1e-2]
                                             [--check-every 10] [--iters 2000] [--warmup 200] [--repeats 3] [--seconds 0.3]

Writes one JSON line (stdout and OUTDIR/cp_many_gap.json).  The measuring code is that of tools/bench_cp_many_stop.py: times
between two HIP events on the library's stream, a warm-up, `repeats` measurements that alternate between the variants compared,
the median with every repeat and the spread ((max - min) / median) beside it.

  (a) off       `iterate(k)` with no test armed, LP-iterations/s over the sets of tools/bench_cp_many.py, against the PARENT
                commit's library (--parent-repo: a built checkout), alternating child processes, parent then this.  The bar is
                fixed before the run: this median >= parent median x (1 - the parent's own spread between its repeats), per
                set; a set within 1 % of the bar is marked.
  (b) price     one process: the SC105 set with no test, and with the certificate armed at both tolerances 0 and check_every 1
                and 10.  Two cadences give two equations: in units of an unarmed iteration, t1 = 1 + i + c and t10 = 1 + i + c /
                10, with i what an armed iteration costs beyond an unarmed one and c what a check costs.  LPs that reach gap 0
                and violation 0 exactly within --screen iterations would stop: they are passed over, and counted.  No bar.
  (c) changes   the mixed list of bench_cp_many_stop.py part (c).  Per kind of LP: the iteration at which the step test at
                --tol stops it and the certificate of that very iterate (a second state with the certificate armed at tolerance 0
                is walked to that iteration; its record is the device's own evaluation) -- the relative gap
                |primal - bound| / (1 + |primal| + |bound|) and the violation a user gets under the name "converged"; then the
                iteration at which the certificate at (--tol, --tol) stops it within --horizon, and the work ratio
                sum_k t_k / (N max_k t_k) of both (an LP that does not stop counts with the horizon).
"""
import argparse
import json
import os
import platform
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_cp_many import perturbed, timed_iterate  # noqa: E402
from bench_cp_many_stop import fixture, many_state, mixed_kinds, part_off, pick_k, summary  # noqa: E402
sys.path.insert(0, os.path.join(REPO, "tests"))


# ---------------------------------------------------------------------------------------------------- (a) off, against the parent
def part_off_with_bar(args):
    out = part_off(args)
    for point in out["points"]:
        if "parent_lp_it_per_s" in point:
            point["bar"] = 1.0 - point["parent_lp_it_per_s"]["spread"]
            point["inside_bar"] = bool(point["this_over_parent"] >= point["bar"])
            point["within_1_percent_of_the_bar"] = bool(abs(point["this_over_parent"] - point["bar"]) <= 0.01)
            print(f"[off] {point['set']}:{point['N']}: ratio {point['this_over_parent']:.4f}, bar {point['bar']:.4f}", file=sys.stderr)
    return out


# ---------------------------------------------------------------------------------------------------- (b) the price of the test
def never_stopping(problems, count, screen):
    """The first `count` of `problems` that do not stop at both tolerances 0 and check_every = 1 within `screen` iterations, and
    how many were passed over."""
    st = many_state(problems)
    st.set_stop_gap(0.0, 0.0, 1)
    st.iterate(screen)
    stopped = st.gap_state()[1]
    st.close()
    keep, passed_over = [], 0
    for p, gone in zip(problems, stopped):
        if len(keep) == count:
            break
        if gone:
            passed_over += 1
        else:
            keep.append(p)
    assert len(keep) == count, "too many LPs of the set reach gap 0 exactly"
    return keep, passed_over


def part_price(args, lib):
    points = []
    for count in [int(v) for v in args.counts_price.split(",")]:
        drawn = perturbed(fixture("sc105"), count + count // 4, args.seed + count)
        problems, passed_over = never_stopping(drawn, count, args.screen)
        states = {"off": many_state(problems), "every_1": many_state(problems), "every_10": many_state(problems)}
        states["every_1"].set_stop_gap(0.0, 0.0, 1)
        states["every_10"].set_stop_gap(0.0, 0.0, 10)
        k = pick_k(lib, states["off"], args.iters, args.warmup, args.seconds)
        for key in ("every_1", "every_10"):
            states[key].iterate(args.warmup + 32)
        rate = {key: [] for key in states}
        for _ in range(args.repeats):   # alternating
            for key, st in states.items():
                rate[key].append(count * k * 1e3 / timed_iterate(lib, st, k))
        point = {"set": "sc105", "N": count, "iterations_per_measurement": k, "screen_iterations": args.screen, "passed_over": passed_over}
        for key, st in states.items():
            point[f"{key}_lp_it_per_s"] = summary(rate[key])
            if key != "off":
                iterations, stopped = st.gap_state()[:2]
                point[f"{key}_stopped"] = int(stopped.sum())
                point[f"{key}_iterations"] = [int(iterations.min()), int(iterations.max())]
                point[f"{key}_over_off"] = point[f"{key}_lp_it_per_s"]["median"] / float(np.median(rate["off"]))
            st.close()
        t1, t10 = 1.0 / point["every_1_over_off"], 1.0 / point["every_10_over_off"]   # in units of an unarmed iteration
        point["cost_per_check"] = (t1 - t10) / 0.9
        point["cost_per_iteration"] = t10 - 1.0 - point["cost_per_check"] / 10.0
        points.append(point)
        print(f"[price] N={count}: off {np.median(rate['off']):.0f} LP-it/s, check_every 1 x{point['every_1_over_off']:.3f}, 10 "
              f"x{point['every_10_over_off']:.3f}; per iteration {point['cost_per_iteration']:+.4f}, per check {point['cost_per_check']:+.4f} "
              "of an unarmed iteration", file=sys.stderr)
    return {"points": points}


# ---------------------------------------------------------------------------------------------------- (c) what it changes
def relative_gap(primal, bound):
    with np.errstate(invalid="ignore"):
        return np.abs(primal - bound) / (1.0 + np.abs(primal) + np.abs(bound))


def work_ratio(iterations, kinds, count):
    t = np.array([iterations[i % kinds] for i in range(count)], dtype=np.float64)
    return float(t.sum() / (count * t.max()))


def number(v):
    """A float for the JSON line: an infinity or a NaN as a string."""
    v = float(v)
    return v if np.isfinite(v) else str(v)


def part_changes(args):
    from pysparselp_amd import chambolle_pock_ppd_many_certified

    kinds = mixed_kinds()
    names = [name for name, _ in kinds]
    distinct = [p for _, p in kinds]
    # the step test on the distinct LPs, then the certificate of each LP's iterate at its stopping iteration
    st = many_state(distinct)
    st.set_stop(args.tol, args.check_every)
    st.iterate(args.horizon)
    step_iterations, step_stopped, _ = st.stop_state()
    st.close()
    walker = many_state(distinct)
    walker.set_stop_gap(0.0, 0.0, 1)
    at_stop = {}
    done = 0
    for t in sorted(set(int(v) for v in step_iterations)):
        walker.iterate(t - done)
        done = t
        iterations, stopped, primal, bound, violation = walker.gap_state()
        for k in np.nonzero(step_iterations == t)[0]:
            assert iterations[k] == t or stopped[k]
            at_stop[int(k)] = (primal[k], bound[k], violation[k], bool(stopped[k]) and iterations[k] < t)
    walker.close()
    # the certificate as the test, on the whole list
    problems = [distinct[i % len(distinct)] for i in range(args.mixed)]
    _, _, info = chambolle_pock_ppd_many_certified(problems, args.tol, args.tol, args.check_every, nb_max_iter=args.horizon)
    rows = []
    for k, name in enumerate(names):
        primal, bound, violation, early = at_stop[k]
        rows.append({"kind": name, "step_test_iteration": int(step_iterations[k]), "step_test_stopped": bool(step_stopped[k]),
                     "relative_gap_there": number(relative_gap(primal, bound)), "violation_there": number(violation),
                     "primal_there": number(primal), "bound_there": number(bound), "reached_gap_0_before": early,
                     "gap_test_iteration": int(info["iterations"][k]), "gap_test_stopped": bool(info["stopped"][k]),
                     "relative_gap_at_the_end": number(relative_gap(info["primal"][k], info["lower_bound"][k])),
                     "violation_at_the_end": number(info["violation"][k])})
        print(f"[changes] {name}: step test {rows[-1]['step_test_iteration']} (gap {rows[-1]['relative_gap_there']}, violation "
              f"{rows[-1]['violation_there']}); gap test {rows[-1]['gap_test_iteration']} stopped {rows[-1]['gap_test_stopped']}",
              file=sys.stderr)
    return {"N": args.mixed, "tol": args.tol, "check_every": args.check_every, "horizon": args.horizon, "kinds": rows,
            "step_test_work_ratio": work_ratio(step_iterations, len(kinds), args.mixed),
            "gap_test_work_ratio": work_ratio(info["iterations"], len(kinds), args.mixed),
            "gap_test_stopped": int(info["stopped"].sum())}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("outdir")
    p.add_argument("--parts", default="a,b,c")
    p.add_argument("--parent-repo", default="")
    p.add_argument("--counts-sc105", default="1,16,256,1024")
    p.add_argument("--counts-potts50", default="1,16,256")
    p.add_argument("--counts-price", default="256,1024")
    p.add_argument("--mixed", type=int, default=256)
    p.add_argument("--tol", type=float, default=1e-2)
    p.add_argument("--check-every", type=int, default=10)
    p.add_argument("--horizon", type=int, default=2000)
    p.add_argument("--screen", type=int, default=3000)
    p.add_argument("--iters", type=int, default=2000)
    p.add_argument("--warmup", type=int, default=200)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--seconds", type=float, default=0.3)
    p.add_argument("--seed", type=int, default=0)
    args = p.parse_args()
    assert args.repeats >= 1 and args.iters >= 32
    parts = args.parts.split(",")
    out = {"method": "chambolle_pock_ppd_many_certified", "box": platform.node(), "device": "AMD Instinct MI355X (gfx950)",
           "iterations": args.iters, "warmup": args.warmup, "repeats": args.repeats}
    if "a" in parts:   # before this process opens the GPU: one process with the device at a time
        out["off_against_parent"] = part_off_with_bar(args)
    if "b" in parts or "c" in parts:
        from pysparselp_amd import _lib

        lib = _lib.lib()
        if "b" in parts:
            out["price_of_the_test"] = part_price(args, lib)
        if "c" in parts:
            out["what_it_changes"] = part_changes(args)
    line = json.dumps(out)
    print(line)
    os.makedirs(args.outdir, exist_ok=True)
    with open(os.path.join(args.outdir, "cp_many_gap.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
