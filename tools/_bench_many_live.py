"""What tools/bench_cp_many_live.py and tools/bench_admm_many_live.py share: the three parts of the compaction measurement of
the Chambolle-Pock and the ADMM list solver, written once over a `solver` -- an object that says how its tool makes a state,
arms its tests, reads its records and builds its lists.  The method is that of tools/bench_dga_many_live.py: one MI355X, one
run; times between two HIP events on the library's stream around the calls (slp_timer_start / _stop), after a warm-up; `repeats`
measurements that alternate between the variants compared; the median with every repeat and the spread ((max - min) / median).

  (a) unchanged  compaction off, against the PARENT commit's library on the same box: the kernel that is never armed and the armed
                 kernels at a tolerance of 0 and check_every = 10 on lists screened for exact fixed points, LP-iterations/s over the
                 solver's sets at the given counts, alternating child processes (parent, this), one at a time.  The bar, fixed
                 before the run, per point: this median >= the parent's median x (1 - the parent's own spread).
  (b) price      one process: a screened list armed at a tolerance of 0 -- nothing ever retires --, compaction on against off, at
                 check_every 1 and 10.  With compaction every call begins with one read-back of the records and every launch is
                 preceded by k_many_live per form.  Recorded: the two rates, their ratio, the cap and the launches per call.  No bar.
  (c) buys       N LPs of two kinds whose stopping iterations differ by about ten times or more; the fast kind stands at the first
                 half of the list, at a random half (seed 0) or at every second place.  Each pattern with compaction on and off, to
                 the horizon: as ONE `iterate` call and as calls of check_every x 10 iterations; in the natural (lds) form and with the
                 form forced to global.  The tool asserts that every LP's record is the same with compaction on and off.  The
                 shipping condition, fixed before the run: in the every-second pattern on the forced global form the compacted run's
                 slowest repeat is below the uncompacted run's fastest, and in every pattern and form the compacted median is at most
                 the uncompacted median x (1 + the uncompacted side's spread).  Also recorded: the grid and the cap of every call.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

from _bench_util import spread


def summary(values):
    return {"median": float(np.median(values)), "repeats": [float(v) for v in values], "spread": spread(values)}


def timed(lib, st, calls):
    """(milliseconds between two HIP events, wall seconds) of `st.iterate(k)` for k in calls; ends synchronised."""
    from pysparselp_amd import _lib

    ms = np.zeros(1)
    start = time.perf_counter()
    _lib.check(lib.slp_timer_start())
    for k in calls:
        st.iterate(k)
    _lib.check(lib.slp_timer_stop(_lib.ptr(ms)))
    return float(ms[0]), time.perf_counter() - start


def pick_k(lib, st, iters, warmup, seconds):
    st.iterate(warmup)
    per_it = timed(lib, st, [32])[0] / 32   # one measurement near `seconds`
    return int(max(32, min(iters, 1e3 * seconds / max(per_it, 1e-6))))


def screened(solver, kernel, problems, count, screen):
    """The first `count` of `problems` that `kernel`'s test at a tolerance of 0 and check_every = 1 does not stop within `screen`
    iterations (an exact fixed point would), and how many of `problems` it does stop."""
    if kernel == "unarmed":
        return problems[:count], 0
    st = solver.state(problems)
    solver.arm(st, kernel, 0.0, 1)
    st.iterate(screen)
    stopped = solver.records(st, kernel)[1]
    st.close()
    keep = [p for p, gone in zip(problems, stopped) if not gone][:count]
    assert len(keep) == count, "too many LPs of the list reach an exact fixed point"
    return keep, int(np.sum(stopped))


# ---------------------------------------------------------------------------------------------------- (a) against the parent
def child_rates(solver, args):
    """LP-iterations/s per set, count and kernel: one measurement each, in this process, with whichever checkout --repo names.
    Uses nothing the parent commit does not have."""
    from pysparselp_amd import _lib

    lib = _lib.lib()
    out = {}
    for name, counts in solver.sets(args):
        for count in counts:
            drawn = solver.draw(name, count + max(2, count // 4), args.seed + count)
            for kernel in solver.kernels:
                problems, _ = screened(solver, kernel, drawn, count, args.screen)
                st = solver.state(problems)
                if kernel != "unarmed":
                    solver.arm(st, kernel, 0.0, 10)
                k = pick_k(lib, st, args.iters, args.warmup, args.seconds)
                out[f"{name}:{count}:{kernel}"] = count * k * 1e3 / timed(lib, st, [k])[0]
                if kernel != "unarmed":
                    assert not solver.records(st, kernel)[1].any()
                st.close()
    return out


def part_unchanged(solver, args, tool, repo):
    def child(where):
        cmd = [sys.executable, tool, "--child-rates", "--repo", os.path.abspath(where), "--counts", args.counts, "--iters", str(args.iters),
               "--warmup", str(args.warmup), "--seconds", str(args.seconds), "--seed", str(args.seed), "--screen", str(args.screen), "unused"]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, check=True, timeout=900)
        return json.loads(done.stdout.decode().strip().splitlines()[-1])

    runs = {"parent": [], "this": []}
    for _ in range(args.repeats):   # alternating, one process at a time
        if args.parent_repo:
            runs["parent"].append(child(args.parent_repo))
        runs["this"].append(child(repo))
    points = []
    for key in runs["this"][0]:
        name, count, kernel = key.split(":")
        point = {"set": name, "N": int(count), "kernel": kernel, "this_lp_it_per_s": summary([r[key] for r in runs["this"]])}
        if runs["parent"]:
            point["parent_lp_it_per_s"] = summary([r[key] for r in runs["parent"]])
            point["this_over_parent"] = point["this_lp_it_per_s"]["median"] / point["parent_lp_it_per_s"]["median"]
            point["bar"] = 1.0 - point["parent_lp_it_per_s"]["spread"]
            point["inside_bar"] = bool(point["this_over_parent"] >= point["bar"])
        points.append(point)
        print(f"[unchanged] {key}: {point['this_lp_it_per_s']['median']:.0f} LP-it/s, ratio to parent {point.get('this_over_parent')}, "
              f"bar {point.get('bar')}", file=sys.stderr)
    return {"parent_measured": bool(args.parent_repo), "points": points,
            "inside_bar": sum(bool(p.get("inside_bar")) for p in points), "of": len(points)}


# ---------------------------------------------------------------------------------------------------- (b) the price of the list
def part_price(solver, args, lib):
    points = []
    name = solver.price_set
    kernel = solver.kernels[-1]
    for count in [int(v) for v in args.counts_price.split(",")]:
        problems, passed_over = screened(solver, kernel, solver.draw(name, count + count // 4, args.seed + count), count, args.screen)
        for every in (1, 10):
            states = {"off": solver.state(problems), "on": solver.state(problems)}
            states["on"].set_compaction(True)
            for st in states.values():
                solver.arm(st, kernel, 0.0, every)
            k = pick_k(lib, states["off"], args.iters, args.warmup, args.seconds)
            states["on"].iterate(args.warmup + 32)
            ms = {key: [] for key in states}
            for _ in range(args.repeats):   # alternating
                for key, st in states.items():
                    ms[key].append(timed(lib, st, [k])[0])
            live = {key: st.live_state() for key, st in states.items()}
            for key, st in states.items():
                assert not solver.records(st, kernel)[1].any() and live[key][0].sum() == count
                st.close()
            assert np.array_equal(live["on"][2], live["off"][2]) and np.array_equal(live["on"][3], live["off"][3])
            off, on = float(np.median(ms["off"])), float(np.median(ms["on"]))
            caps = [int(c) for c, n in zip(live["on"][3], live["on"][2]) if n]
            launches = sum(-(-k // c) for c in caps)
            point = {"set": name, "N": count, "kernel": kernel, "check_every": every, "iterations_per_call": k, "passed_over": passed_over,
                     "cap_per_form": [int(v) for v in live["on"][3]], "grid_per_form": [int(v) for v in live["on"][2]],
                     "iteration_launches_per_call": launches, "list_launches_per_call_on": launches, "record_read_backs_per_call_on": 1,
                     "off_lp_it_per_s": summary([count * k * 1e3 / v for v in ms["off"]]),
                     "on_lp_it_per_s": summary([count * k * 1e3 / v for v in ms["on"]]), "on_over_off": off / on,
                     "price_per_call_us": 1e3 * (on - off)}
            points.append(point)
            print(f"[price] {name} N={count} check_every={every}: off {point['off_lp_it_per_s']['median']:.0f}, on "
                  f"{point['on_lp_it_per_s']['median']:.0f} LP-it/s, x{point['on_over_off']:.4f}; {launches} launches of at most {caps} "
                  f"per call of {k}", file=sys.stderr)
    return {"points": points}


# ---------------------------------------------------------------------------------------------------- (c) what the list buys
def part_buys(solver, args, lib):
    count, every = args.pruned, args.check_every
    call = every * 10
    patterns = {"first_half": np.arange(count) < count // 2, "random_half": np.random.RandomState(0).permutation(count) < count // 2,
                "every_second": np.arange(count) % 2 == 0}
    out = {"N": count, "check_every": every, "call": call, "forms": {}}
    condition = {"every_pattern_and_form_met": True}
    for form in ("lds", "global"):
        solver.force_form("global" if form == "global" else None)
        fast, slow, kernel, tol, horizon = solver.pair(args, form)
        assert horizon % call == 0
        splits = {"one_call": [horizon], f"calls_of_{call}": [call] * (horizon // call)}
        variants = {f"{name}/{'on' if compact else 'off'}/{split}": (half, compact, calls)
                    for split, calls in splits.items() for name, half in patterns.items() for compact in (False, True)}
        events, wall, seen, calls_seen = {key: [] for key in variants}, {key: [] for key in variants}, {}, {}
        made = {name: [fast[1] if f else slow[1] for f in half] for name, half in patterns.items()}
        for rep in range(args.repeats + 1):   # the first round warms up and reads the grid and the cap after every call; alternating
            for key, (half, compact, calls) in variants.items():
                st = solver.state(made[key.split("/")[0]])
                if compact:
                    st.set_compaction(True)
                solver.arm(st, kernel, tol, every)
                if rep == 0:
                    forms = sorted({st.form(k) for k in range(st.count)})
                    assert forms == [form], (forms, form)
                    calls_seen[key] = []
                    for k in calls:
                        st.iterate(k)
                        live, _, launched, cap = st.live_state()
                        calls_seen[key].append([int(launched.sum()), int(cap.max()), int(live.sum())])
                else:
                    ms, took = timed(lib, st, calls)
                    events[key].append(ms)
                    wall[key].append(took)
                seen[key] = [np.asarray(v) for v in solver.records(st, kernel)]
                st.close()
        stops = seen["first_half/off/one_call"]
        res = {"kernel": kernel, "tolerance": tol, "horizon": horizon, "fast_kind": fast[0], "slow_kind": slow[0],
               "shapes_n_m": {k[0]: solver.shape(k[1]) for k in (fast, slow)}, "stopping_iterations_fast": sorted({int(v) for v in stops[0][patterns["first_half"]]}),
               "stopping_iterations_slow": sorted({int(v) for v in stops[0][~patterns["first_half"]]}),
               "stopped": int(stops[1].sum()), "work_ratio": float(stops[0].sum() / (count * horizon)), "variants": {}}
        for name in patterns:   # every LP's record is the same with compaction on and off, and however the run is split
            for split in splits:
                a, b = seen[f"{name}/off/{split}"], seen[f"{name}/on/{split}"]
                assert all(np.array_equal(u, v, equal_nan=u.dtype.kind == "f") for u, v in zip(a, b)), (form, name, split)
        for key in variants:
            res["variants"][key] = {"events_ms": summary(events[key]), "wall_s": summary(wall[key]),
                                    "grid_cap_live_after_each_call": calls_seen[key] if len(calls_seen[key]) <= 4 else
                                    calls_seen[key][:3] + [calls_seen[key][-1]]}
        res["on_over_off"] = {}
        for name in patterns:
            for split in splits:
                on, off = events[f"{name}/on/{split}"], events[f"{name}/off/{split}"]
                ratio, allowed = float(np.median(on) / np.median(off)), 1.0 + spread(off)
                res["on_over_off"][f"{name}/{split}"] = {"ratio": ratio, "allowed": allowed, "met": bool(ratio <= allowed),
                                                         "slowest_on_ms": max(on), "fastest_off_ms": min(off)}
                condition["every_pattern_and_form_met"] = condition["every_pattern_and_form_met"] and bool(ratio <= allowed)
                print(f"[buys] {form} {name}/{split}: off {np.median(off):.2f} ms, on {np.median(on):.2f} ms, x{ratio:.3f} (allowed "
                      f"{allowed:.3f})", file=sys.stderr)
        out["forms"][form] = res
    solver.force_form(None)
    wide = out["forms"]["global"]["on_over_off"]
    condition["every_second_on_the_wide_form_met"] = all(v["slowest_on_ms"] < v["fastest_off_ms"] for key, v in wide.items()
                                                         if key.startswith("every_second/"))
    condition["met"] = condition["every_second_on_the_wide_form_met"] and condition["every_pattern_and_form_met"]
    out["condition"] = condition
    print("[buys] condition " + ("met" if condition["met"] else "NOT met") + f": {condition}", file=sys.stderr)
    return out


def add_arguments(p):
    p.add_argument("outdir")
    p.add_argument("--parts", default="a,b,c")
    p.add_argument("--parent-repo", default="")
    p.add_argument("--repo", default="")
    p.add_argument("--child-rates", action="store_true")
    p.add_argument("--counts", default="1,16,256,1024")
    p.add_argument("--counts-price", default="256,1024")
    p.add_argument("--pruned", type=int, default=1024)
    p.add_argument("--check-every", type=int, default=10)
    p.add_argument("--screen", type=int, default=3000)
    p.add_argument("--iters", type=int, default=2000)
    p.add_argument("--warmup", type=int, default=200)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--seconds", type=float, default=0.3)
    p.add_argument("--seed", type=int, default=0)


def run(solver, p, tool, repo, method, filename):
    args = p.parse_args()
    if args.child_rates:
        if args.repo:   # ahead of this checkout: the package, the library and the fixtures of that one
            sys.path[:0] = [args.repo, os.path.join(args.repo, "tests")]
        print(json.dumps(child_rates(solver, args)))
        return
    assert args.repeats >= 1 and args.iters >= 32
    parts = args.parts.split(",")
    import platform

    out = {"method": method, "box": platform.node(), "device": "AMD Instinct MI355X (gfx950)", "iterations": args.iters,
           "warmup": args.warmup, "repeats": args.repeats}
    if "a" in parts:   # before this process opens the GPU: one process with the device at a time
        out["unchanged_against_parent"] = part_unchanged(solver, args, tool, repo)
    if "b" in parts or "c" in parts:
        from pysparselp_amd import _lib

        lib = _lib.lib()
        if "b" in parts:
            out["price_of_the_list"] = part_price(solver, args, lib)
        if "c" in parts:
            out["what_compaction_buys"] = part_buys(solver, args, lib)
    line = json.dumps(out)
    print(line)
    os.makedirs(args.outdir, exist_ok=True)
    with open(os.path.join(args.outdir, filename), "w") as f:
        f.write(line + "\n")
