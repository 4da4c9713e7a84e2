"""What the per-instance stopping test of the batched dual gradient ascent (DeviceDGABatch.set_stop, csrc/slp_dga_batch.hip) costs
and what retiring instances gains, measured on one GPU.

    python tools/bench_dga_batch_stop.py OUTDIR [--potts 50,256] [--batch 64] [--seconds 0.5] [--warmup 50] [--repeats 3]
                                         [--unarmed-only LABEL] [--parent-lines FILE --own-lines FILE [--fold-into RESULT]]

Writes one JSON line (stdout and OUTDIR/dga_batch_stop.json).  Per Potts n x n LP (problems.potts_lp; instance costs = seeded
perturbations of the unary costs, as tools/bench_dga_batch.py) at the batch size given, on the automatic path:

(a) `unarmed`: iterations per second of a state whose test was never armed.  With --unarmed-only LABEL the tool measures nothing
    else, uses nothing but the interface of the batch without a test and writes OUTDIR/dga_batch_unarmed_LABEL.json -- so the
    very same file runs from a checkout of the parent commit (python PARENT/tools/bench_dga_batch_stop.py ...), in a process of
    its own, alternating with this tree's on the same box.  --parent-lines / --own-lines: files of such lines (one per process);
    they are folded into the result as `against_parent`: both rates per process and the run-to-run spread of each side
    (--fold-into RESULT: into an existing result, without measuring anything else).
(b) `armed_cannot_fire`: the same iterations with the test armed but unable to fire, for check_every 1, 10 and 100 and three
    rules: `step` (tol = 0, no cut-offs), `step_and_bound` (tol = 0 with targets = +inf: the bound is evaluated, nothing can meet
    it) and `bound_above` (no step test, cut-offs above every bound).  An unarmed state and a second one, at the same iterates,
    are timed in turn -- unarmed, armed, unarmed -- and the armed run is set against the mean of its two neighbours; `control` is
    the same with the second state's test off, what the two states differ by before any check is paid for, and
    `time_ratio_over_control` the price of the checks.  That no instance stopped is asserted.
(c) `half_retired`: every second instance gets the bound an unstopped run shows after `early` iterations as its cut-off, so it
    retires at the first check from there on; the wall time of `horizon` iterations from the start against the batch without a
    test, fresh states for every repeat, alternating.

Every time is a pair of HIP events (slp_timer_start / _stop) around plain launches after a warm-up, the draw buffer filled
beforehand (tools/_bench_util.py); medians with the spread (max - min) / median.  Reads nothing outside the repository."""
import argparse
import json
import os
import platform
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from _bench_util import spread, timed_between_events  # noqa: E402

EVERY = (1, 10, 100)


def timed(lib, state, k):
    """Milliseconds for `k` iterations between two HIP events; the draws are pushed first."""
    return timed_between_events(lib, [state], k, lambda st, k: st.push_random(np.random.RandomState(17).random_sample(2 * k + 2)))


class Workload:
    def __init__(self, size, batch, seed):
        from pysparselp_amd import _lib
        from pysparselp_amd.device import DeviceMatrix
        from pysparselp_amd.problems import potts_lp

        self.lib = _lib.lib()
        lp, _, pix, _ = potts_lp(size)
        assert lp.b_lower is None or np.max(lp.b_lower) == -np.inf
        a_eq, a_ineq = lp.a_equalities, lp.a_inequalities
        self.m_eq = a_eq.shape[0]
        self.c, self.lb, self.ub = lp.costsvector, lp.lower_bounds, lp.upper_bounds
        self.n = self.c.size
        self.b = np.concatenate((lp.b_equalities if self.m_eq else np.zeros(0), lp.b_upper))
        self.mat = DeviceMatrix.from_blocks(a_eq if self.m_eq else None, a_ineq, self.n)
        self.m = self.mat.shape[0]
        self.batch = batch
        self.costs = np.tile(self.c, (batch, 1))
        self.costs[1:, :pix.size] += 0.3 * np.random.RandomState(seed + batch).randn(batch - 1, pix.size)   # the unary costs come first

    def state(self):
        from pysparselp_amd.DualGradientAscent import DeviceDGABatch

        rs = np.random.RandomState(0)
        y0 = np.concatenate((-rs.rand(self.m_eq), np.abs(rs.rand(self.m - self.m_eq))))
        return DeviceDGABatch(self.mat, self.b, self.costs, self.lb, self.ub, y0, m_eq=self.m_eq, draws=rs.random_sample)

    def iterations_for(self, state, seconds):
        """A multiple of 100 (every cadence divides it) that takes about `seconds`."""
        per = timed(self.lib, state, 10) / 10
        return int(max(100, round(seconds * 1e3 / per / 100.0) * 100))


def unarmed(w, seconds, warmup, repeats):
    st = w.state()
    st.iterate(warmup)
    k = w.iterations_for(st, seconds)
    rate = np.array([1e3 * k / timed(w.lib, st, k) for _ in range(repeats)])
    flags = st.status()[0]
    assert not np.any(flags), flags
    out = {"path": st.path(), "sort": st.sort(), "iterations_per_measurement": k, "it_per_s": float(np.median(rate)),
           "it_per_s_repeats": rate.tolist(), "spread": spread(rate)}
    st.close()
    return out


def armed_cannot_fire(w, seconds, warmup, repeats):
    plain, test = w.state(), w.state()
    plain.iterate(warmup)
    test.iterate(warmup)
    k = w.iterations_for(plain, seconds)
    timed(w.lib, test, 10)   # both states stand at the same iterate
    # `control`: the second state with its test off -- what the two states differ by before any check is paid for
    rules = {"control": (None, None), "step": (0.0, None), "step_and_bound": (0.0, np.full(w.batch, np.inf)),
             "bound_above": (None, np.full(w.batch, 1e300))}
    points, control = [], 1.0
    for name, (tol, targets) in rules.items():
        for every in EVERY if name != "control" else (1,):
            trios = []
            for _ in range(repeats):   # unarmed, armed, unarmed: the armed run against the mean of its two neighbours
                before = timed(w.lib, plain, k)
                test.set_stop(tol, targets, every)
                with_test = timed(w.lib, test, k)
                test.set_stop(None)
                trios.append((before, with_test, timed(w.lib, plain, k)))
                timed(w.lib, test, k)   # the states stay at the same iterate
            stopped = test.stop_state()[1]
            assert not stopped.any(), (name, every, stopped)
            trios = np.array(trios)
            base = 0.5 * (trios[:, 0] + trios[:, 2])
            ratio = trios[:, 1] / base
            if name == "control":
                control = float(np.median(ratio))
            points.append({"rule": name, "check_every": every if name != "control" else None, "iterations_per_measurement": k,
                           "unarmed_it_per_s": float(np.median(1e3 * k / base)), "armed_it_per_s": float(np.median(1e3 * k / trios[:, 1])),
                           "time_ratio_armed_to_unarmed": float(np.median(ratio)), "time_ratio_repeats": ratio.tolist(),
                           "time_ratio_over_control": float(np.median(ratio) / control),
                           "check_in_iterations": float((np.median(ratio) / control - 1.0) * every)})
            print(f"  {name} every {every}: x{points[-1]['time_ratio_armed_to_unarmed']:.4f} (over control x"
                  f"{points[-1]['time_ratio_over_control']:.4f}), a check = {points[-1]['check_in_iterations']:.3f} iterations", file=sys.stderr)
    a, b = plain.status(), test.status()
    assert a[3] == b[3] and np.array_equal(a[1], b[1]) and np.array_equal(plain.y()[1], test.y()[1])   # the test changed no iterate
    plain.close()
    test.close()
    return points


def half_retired(w, horizon, early, every, repeats):
    probe = w.state()
    probe.push_random(np.random.RandomState(17).random_sample(2 * horizon + 2))   # the draws of the timed runs
    probe.iterate(early, refill=False)
    targets = np.full(w.batch, np.inf)
    targets[::2] = probe.report()[::2, 0]
    probe.close()
    times, stops = [], None
    for _ in range(repeats):
        pair = []
        for arm in (False, True):
            st = w.state()
            if arm:
                st.set_stop(None, targets, every)
            pair.append(timed(w.lib, st, horizon))
            if arm:
                iterations, stopped = st.stop_state()[:2]
                assert stopped[::2].all() and not stopped[1::2].any()
                stops = iterations[::2]
            st.close()
        times.append(pair)
    times = np.array(times)
    ratio = times[:, 1] / times[:, 0]
    return {"horizon": horizon, "cut_off_from_iteration": early, "check_every": every, "retired": int(targets[::2].size),
            "of": w.batch, "stopping_iterations_min_max": [int(stops.min()), int(stops.max())],
            "unstopped_ms": float(np.median(times[:, 0])), "half_retired_ms": float(np.median(times[:, 1])),
            "time_ratio": float(np.median(ratio)), "time_ratio_repeats": ratio.tolist(), "spread_unstopped": spread(times[:, 0])}


def fold_parent(parent_file, own_file):
    sides = {}
    for label, path in (("parent", parent_file), ("this_tree", own_file)):
        lines = [json.loads(v) for v in open(path) if v.strip()]
        per = {}
        for line in lines:
            for name, q in line["unarmed"].items():
                per.setdefault(name, []).append(q["it_per_s"])
        sides[label] = per
    out = {}
    for name in sides["parent"]:
        p, o = np.array(sides["parent"][name]), np.array(sides["this_tree"][name])
        out[name] = {"parent_it_per_s_per_process": p.tolist(), "this_tree_it_per_s_per_process": o.tolist(),
                     "parent_median": float(np.median(p)), "this_tree_median": float(np.median(o)),
                     "parent_run_to_run_spread": spread(p), "this_tree_run_to_run_spread": spread(o),
                     "ratio_this_tree_to_parent": float(np.median(o) / np.median(p)),
                     "within_parent_spread": bool(abs(np.median(o) / np.median(p) - 1.0) <= spread(p))}
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("outdir")
    p.add_argument("--potts", default="50,256")
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--seconds", type=float, default=0.5)
    p.add_argument("--warmup", type=int, default=50)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--unarmed-only", default=None, metavar="LABEL")
    p.add_argument("--parent-lines", default=None)
    p.add_argument("--own-lines", default=None)
    p.add_argument("--fold-into", default=None, metavar="FILE")
    args = p.parse_args()
    os.makedirs(args.outdir, exist_ok=True)
    sizes = [int(v) for v in args.potts.split(",")]
    head = {"method": "dual_gradient_ascent_batch", "box": platform.node(), "device": "AMD Instinct MI355X (gfx950)", "B": args.batch,
            "warmup": args.warmup, "repeats": args.repeats}
    if args.unarmed_only is not None:
        out = dict(head, label=args.unarmed_only, unarmed={})
        for size in sizes:
            w = Workload(size, args.batch, args.seed)
            out["unarmed"][f"potts{size}"] = dict(unarmed(w, args.seconds, args.warmup, args.repeats), n=int(w.n), m=int(w.m))
            w.mat.close()
        line = json.dumps(out)
        print(line)
        with open(os.path.join(args.outdir, f"dga_batch_unarmed_{args.unarmed_only}.json"), "a") as f:
            f.write(line + "\n")
        return
    if args.fold_into:   # no measurement: the lines of a later alternation replace `against_parent` of an existing result
        out = json.loads(open(args.fold_into).read())
        out["against_parent"] = fold_parent(args.parent_lines, args.own_lines)
        with open(args.fold_into, "w") as f:
            f.write(json.dumps(out) + "\n")
        return
    out = dict(head, workloads=[])
    for size in sizes:
        w = Workload(size, args.batch, args.seed)
        print(f"[potts{size}] n = {w.n}, m = {w.m}", file=sys.stderr)
        plain = unarmed(w, args.seconds, args.warmup, args.repeats)
        horizon = max(100, int(round(plain["it_per_s"] * 2 * args.seconds / 100.0)) * 100)
        out["workloads"].append({"workload": f"potts{size}", "n": int(w.n), "m": int(w.m), "m_eq": int(w.m_eq), "unarmed": plain,
                                 "armed_cannot_fire": armed_cannot_fire(w, args.seconds, args.warmup, args.repeats),
                                 "half_retired": half_retired(w, horizon, 20, 10, args.repeats)})
        w.mat.close()
    if args.parent_lines and args.own_lines:
        out["against_parent"] = fold_parent(args.parent_lines, args.own_lines)
    line = json.dumps(out)
    print(line)
    with open(os.path.join(args.outdir, "dga_batch_stop.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
