"""Compaction for dual gradient ascent on a list (DeviceDGAMany.set_compaction, csrc/slp_many.h k_many_live, csrc/slp_dga_many.hip
k_dgm_iterate<., ., true>): that the kernels without it are the parent's, what the list of the live LPs costs when nothing retires,
and what it buys when LPs retire here and there.

    python tools/bench_dga_many_live.py OUTDIR [--parts a,b,c] [--parent-repo DIR] [--counts 1,8,64,256,1024]
                                               [--counts-price 256,1024] [--pruned 1024] [--prune-at 20] [--check-every 10]
                                               [--horizon 200] [--call 20] [--iters 400] [--warmup 20] [--repeats 3]
                                               [--seconds 0.3] [--screen 1500]

Writes one JSON line (stdout and OUTDIR/dga_many_live.json).  It follows tools/bench_dga_many_bound.py, whose part (a) it runs as
it is and whose helpers it imports: the Potts lists of tools/bench_dga_many.py, times between two HIP events on the library's
stream with the draw buffers filled beforehand, a warm-up, `repeats` measurements that alternate between the variants compared,
the median with every repeat and the spread ((max - min) / median) beside it.

  (a) unchanged  compaction off: the kernel that is never armed, <false, false, false>, and the kernel armed with the step alone,
                 <true, false, false>, instance-iterations/s against the PARENT commit's library on the same box, alternating child
                 processes (parent, this), one at a time.  --parent-repo names a built checkout of the parent; without it the
                 comparison is null.  The bar, fixed before the run, per N and kernel: this median >= the parent's median x
                 (1 - the parent's own spread between its repeats).
  (b) price      one process: a Potts list armed with no tolerance and cut-offs of 1e300 -- nothing ever retires --, compaction on
                 against off, at check_every = 1 and 10.  With compaction every launch is preceded by k_many_live and reads its LP
                 through the list.  Recorded: the two rates, their ratio, the cap, and the price per launch in iterations,
                 (time on - time off) / launches / (time off / iterations).  No bar.
  (c) buys       `--pruned` Potts LPs, half of them with the bound an unstopped run shows after `--prune-at` iterations as cut-off,
                 so that they are retired at that check: the first half of the list, a random half (seed 0), every second LP.
                 Each pattern with compaction on and off, and the list without cut-offs, to `--horizon` iterations: as ONE
                 `iterate` call -- the grid and the cap of a call are fixed when it begins, so compaction changes only which
                 workgroups the live LPs have -- and as calls of `--call` iterations, where every call after the retirement
                 launches only the live LPs and takes their cap.  Wall time (host clock around the calls and a synchronising
                 read, the states created and the draws pushed beforehand, as the table this one repeats) and the time between
                 two HIP events around the same calls.  The shipping condition, fixed before the run, on the wall times of the one
                 call and of the split calls alike: with every second LP retired the compacted run's slowest repeat is below the
                 uncompacted run's fastest; with the first half retired the compacted median is not above the uncompacted median
                 by more than the uncompacted run's spread.  Also recorded: each ratio to the list without cut-offs beside the
                 work ratio, and the cap every call used.
"""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_dga_many import fill, potts_list, timed  # noqa: E402
from bench_dga_many_bound import part_unchanged  # noqa: E402
from bench_dga_many_stop import GRIDS, many_state, pick_k, summary  # noqa: E402


# ---------------------------------------------------------------------------------------------------- (b) the price of the list
def part_price(args, lib):
    points = []
    for count in [int(v) for v in args.counts_price.split(",")]:
        lps = potts_list(count, GRIDS)
        for every in (1, 10):
            states = {"off": many_state(lps), "on": many_state(lps)}
            states["on"].set_compaction(True)
            for st in states.values():
                st.set_cutoff(None, every, 1e300)
            k = pick_k(lib, states["off"], args.iters, args.warmup, args.seconds)
            states["on"].iterate(args.warmup + 8)
            ms = {key: [] for key in states}
            for _ in range(args.repeats):   # alternating
                for key, st in states.items():
                    ms[key].append(timed(lib, [st], k))
            cap = {key: st.live_state()[3] for key, st in states.items()}
            launched = {key: st.live_state()[2] for key, st in states.items()}
            assert cap["on"] == cap["off"] and launched == {"off": count, "on": count}, (cap, launched)
            for st in states.values():
                full = st.stop_state_full()
                assert not full[1].any() and np.all(np.isfinite(full[3]))   # every check evaluated a bound, none fired
                st.close()
            off, on = float(np.median(ms["off"])), float(np.median(ms["on"]))
            launches = -(-k // cap["on"])
            point = {"set": "potts 8..16", "N": count, "check_every": every, "iterations_per_measurement": k, "cap": cap["on"],
                     "launches_per_measurement": launches,
                     "off_instance_it_per_s": summary([count * k * 1e3 / v for v in ms["off"]]),
                     "on_instance_it_per_s": summary([count * k * 1e3 / v for v in ms["on"]]),
                     "on_over_off": off / on, "price_per_launch_in_iterations": (on - off) / launches / (off / k),
                     "price_per_launch_us": 1e3 * (on - off) / launches}
            points.append(point)
            print(f"[price] N={count} check_every={every}: off {point['off_instance_it_per_s']['median']:.0f}, on "
                  f"{point['on_instance_it_per_s']['median']:.0f} instance-it/s, x{point['on_over_off']:.4f}; {launches} launches of at most "
                  f"{cap['on']}: {point['price_per_launch_in_iterations']:.3f} it = {point['price_per_launch_us']:.1f} us per launch",
                  file=sys.stderr)
    return {"points": points}


# ---------------------------------------------------------------------------------------------------- (c) what the list buys
def part_buys(args, lib):
    from pysparselp_amd import _lib

    count, every, horizon, call = args.pruned, args.check_every, args.horizon, args.call
    assert args.prune_at % every == 0 and horizon % every == 0 and horizon > args.prune_at and horizon % call == 0
    lps = potts_list(count, GRIDS)
    st = many_state(lps)
    st.iterate(args.prune_at)
    bound = st.report()[:, 0]
    st.close()
    halves = {"first_half": np.arange(count) < count // 2, "random_half": np.random.RandomState(0).permutation(count) < count // 2,
              "every_second": np.arange(count) % 2 == 0}
    splits = {"one_call": [horizon], f"calls_of_{call}": [call] * (horizon // call)}

    def ready(targets, compact):
        st = many_state(lps)
        if compact:
            st.set_compaction(True)
        if targets is not None:
            st.set_cutoff(None, every, targets)
        fill(st, horizon)
        return st

    def run(st, calls):
        """(wall seconds, milliseconds between two HIP events, the stop state)."""
        ms = np.zeros(1)
        start = time.perf_counter()
        _lib.check(lib.slp_timer_start())
        for k in calls:
            st.iterate(k, refill=False)
        _lib.check(lib.slp_timer_stop(_lib.ptr(ms)))
        full = st.stop_state_full()   # synchronises
        return time.perf_counter() - start, float(ms[0]), full

    def caps_of(targets, compact, calls):
        """The cap and the grid of every call of a run, read after each call (a run of its own, not timed)."""
        st = ready(targets, compact)
        out = []
        for k in calls:
            st.iterate(k, refill=False)
            _, _, launched, cap = st.live_state()
            out.append([int(launched), int(cap)])
        st.close()
        return out

    variants = {}
    for split, calls in splits.items():
        variants[f"no_cut_offs/{split}"] = (None, False, calls)
        for name, half in halves.items():
            for compact in (False, True):
                variants[f"{name}/{'on' if compact else 'off'}/{split}"] = (np.where(half, bound, np.inf), compact, calls)
    wall, events, seen = {key: [] for key in variants}, {key: [] for key in variants}, {}
    for rep in range(args.repeats + 1):   # the first round warms up; alternating
        for key, (targets, compact, calls) in variants.items():
            st = ready(targets, compact)
            took, ms, seen[key] = run(st, calls)
            st.close()
            if rep:
                wall[key].append(took)
                events[key].append(ms)
    out = {"set": "potts 8..16", "N": count, "check_every": every, "horizon": horizon, "prune_at": args.prune_at, "call": call,
           "work_ratio": (count // 2 * args.prune_at + (count - count // 2) * horizon) / (count * horizon), "variants": {}}
    for key, (targets, compact, calls) in variants.items():
        base = f"no_cut_offs/{key.split('/')[-1]}"
        full = seen[key]
        point = {"wall_s": summary(wall[key]), "events_ms": summary(events[key]),
                 "wall_over_no_cut_offs": float(np.median(wall[key]) / np.median(wall[base])),
                 "events_over_no_cut_offs": float(np.median(events[key]) / np.median(events[base])),
                 "retired": int(full[1].sum()), "retired_at": sorted({int(v) for v in full[0][full[1]]}),
                 "launched_and_cap_per_call": caps_of(targets, compact, calls)}
        out["variants"][key] = point
    # every LP's record is the same with compaction on and off
    for name in halves:
        for split in splits:
            a, b = seen[f"{name}/off/{split}"], seen[f"{name}/on/{split}"]
            assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a, b)), (name, split)
    out["condition"] = {}
    for split in splits:
        on, off = wall[f"every_second/on/{split}"], wall[f"every_second/off/{split}"]
        first_on, first_off = wall[f"first_half/on/{split}"], wall[f"first_half/off/{split}"]
        slack = (max(first_off) - min(first_off)) / float(np.median(first_off))
        cond = {"every_second_slowest_on_s": max(on), "every_second_fastest_off_s": min(off), "every_second_met": bool(max(on) < min(off)),
                "first_half_on_over_off": float(np.median(first_on) / np.median(first_off)), "first_half_allowed": 1.0 + slack,
                "first_half_met": bool(np.median(first_on) <= np.median(first_off) * (1.0 + slack))}
        cond["met"] = cond["every_second_met"] and cond["first_half_met"]
        out["condition"][split] = cond
        print(f"[buys] {split}: " + ", ".join(
            f"{name} off x{out['variants'][f'{name}/off/{split}']['wall_over_no_cut_offs']:.3f} on "
            f"x{out['variants'][f'{name}/on/{split}']['wall_over_no_cut_offs']:.3f}" for name in halves)
            + f" of no cut-offs {np.median(wall[f'no_cut_offs/{split}']) * 1e3:.1f} ms (work ratio {out['work_ratio']:.3f}); condition "
            + ("met" if cond["met"] else "NOT met"), file=sys.stderr)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("outdir")
    p.add_argument("--parts", default="a,b,c")
    p.add_argument("--parent-repo", default="")
    p.add_argument("--counts", default="1,8,64,256,1024")
    p.add_argument("--counts-price", default="256,1024")
    p.add_argument("--pruned", type=int, default=1024)
    p.add_argument("--prune-at", type=int, default=20)
    p.add_argument("--check-every", type=int, default=10)
    p.add_argument("--horizon", type=int, default=200)
    p.add_argument("--call", type=int, default=20, help="part c: the iterations of a call in the run split over calls")
    p.add_argument("--iters", type=int, default=400)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--seconds", type=float, default=0.3)
    p.add_argument("--screen", type=int, default=1500, help="part a: iterations of the screening run for LPs that reach a fixed point")
    args = p.parse_args()
    assert args.repeats >= 1 and args.iters >= 8
    parts = args.parts.split(",")
    out = {"method": "dual_gradient_ascent_many_compact", "box": platform.node(), "device": "AMD Instinct MI355X (gfx950)",
           "iterations": args.iters, "warmup": args.warmup, "repeats": args.repeats}
    if "a" in parts:   # before this process opens the GPU: one process with the device at a time
        out["unchanged_against_parent"] = part_unchanged(args)
    if "b" in parts or "c" in parts:
        from pysparselp_amd import _lib

        lib = _lib.lib()
        if "b" in parts:
            out["price_of_the_list"] = part_price(args, lib)
        if "c" in parts:
            out["what_compaction_buys"] = part_buys(args, lib)
    line = json.dumps(out)
    print(line)
    os.makedirs(args.outdir, exist_ok=True)
    with open(os.path.join(args.outdir, "dga_many_live.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
