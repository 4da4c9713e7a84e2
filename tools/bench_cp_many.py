"""Chambolle-Pock on a set of LPs, one workgroup per LP (CPManyState, csrc/slp_cp_many.hip), measured against the two ways the
same library already solves such a set.

    python tools/bench_cp_many.py OUTDIR [--sets sc105,potts50] [--counts-sc105 1,16,256,1024] [--counts-potts50 1,16,256]
                                         [--iters 2000] [--warmup 200] [--repeats 3] [--seconds 0.3]

Writes one JSON line (stdout and OUTDIR/cp_many.json).  A set is N copies of a golden fixture's reduced LP with seeded
perturbations of the matrix values and the costs: SC105 (2 n + m = 311 doubles: the LDS form) and Potts-50 (24 600 doubles: the
global form).  Per set and N, `repeats` times in turn, in one process, after a warm-up, each between two HIP events on the
library's stream (slp_timer_start / slp_timer_stop) around `iterate(k)` -- the call a solve makes between two reports:

  (a) single    the single solver (CPState, default order and format: graph replay of 16 iterations) on one LP after another;
                measured on min(N, 4) of the LPs, LP-iterations/s = 1 / the mean time of one LP's iteration;
  (b) concat    the block-diagonal concatenation of the N LPs handed to the single solver as ONE LP (bit-identical per block);
  (c) many      this feature.

k is `iters`, lowered per contender so that one measurement stays near `seconds` (recorded).  Recorded per point:
LP-iterations/s of each contender (median and every repeat), the spread of the repeats ((max - min) / median), the forms that ran,
and slp_cp_many_bench's milliseconds per iteration of the whole set (plain launches of k iterations: whole, primal half, dual half).

`holds_at_256`: on the SC105 set at N = 256 the slowest repeat of (c) lies above the fastest repeat of both (a) and (b).
`concat_wins_from`: the smallest measured N from which (b)'s median is above (c)'s at every larger measured N, or null.
"""
import argparse
import ctypes
import json
import os
import platform
import sys

import numpy as np
import scipy.sparse

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from _bench_util import spread  # noqa: E402
sys.path.insert(0, os.path.join(REPO, "tests"))


def perturbed(problem, count, seed):
    """``count`` LPs: the fixture itself, then seeded perturbations of its matrix values and costs."""
    c, a_eq, beq, a_ineq, bl, bu, lb, ub = problem
    rs = np.random.RandomState(seed)
    out = [problem]
    for _ in range(count - 1):
        ae, ai = scipy.sparse.csr_matrix(a_eq), scipy.sparse.csr_matrix(a_ineq)
        ae.data = ae.data * (1 + 0.1 * rs.randn(ae.nnz))
        ai.data = ai.data * (1 + 0.1 * rs.randn(ai.nnz))
        out.append((c * (1 + 0.2 * rs.randn(c.size)) + 0.05 * np.mean(np.abs(c)) * rs.randn(c.size), ae, beq, ai, bl, bu, lb, ub))
    return out


def single_state(problem):
    from pysparselp_amd.ChambollePockPPD import CPState, one_sided_system

    c, a_eq, beq, a_ineq, bl, bu, lb, ub = problem
    if a_eq is not None and a_eq.shape[0] == 0:
        a_eq, beq = None, None
    ineq, b_ineq = (None, None) if (a_ineq is None or a_ineq.shape[0] == 0) else one_sided_system(a_ineq, bl, bu)
    return CPState(c, a_eq, beq, ineq, b_ineq, lb, ub, None, 1, 1)


def concatenated(problems):
    """The set as ONE LP: block-diagonal matrices, concatenated vectors."""
    cat = lambda pos: np.concatenate([np.asarray(p[pos], dtype=np.float64) for p in problems])  # noqa: E731
    diag = lambda pos: scipy.sparse.block_diag([p[pos] for p in problems], format="csr")  # noqa: E731
    bl = None if problems[0][4] is None else cat(4)
    return cat(0), diag(1), cat(2), diag(3), bl, cat(5), cat(6), cat(7)


def timed_iterate(lib, state, k):
    """Milliseconds the GPU spent on ``state.iterate(k)`` (HIP events on the library's stream)."""
    from pysparselp_amd import _lib

    ms = ctypes.c_double(0.0)
    _lib.check(lib.slp_timer_start())
    state.iterate(k)
    _lib.check(lib.slp_timer_stop(ctypes.byref(ms)))
    return ms.value


def measure(lib, name, problem, counts, iters, warmup, repeats, seconds, seed):
    from pysparselp_amd.ChambollePockPPD import CPManyState, _many_problem

    points = []
    for count in counts:
        problems = perturbed(problem, count, seed + count)
        many = CPManyState([_many_problem(k, p) for k, p in enumerate(problems)])
        forms = sorted(set(many.form(k) for k in range(count)))
        singles = [single_state(p) for p in problems[:min(count, 4)]]
        concat = single_state(concatenated(problems))
        ks = {}
        for key, states in (("many", [many]), ("concat", [concat]), ("single", singles)):
            for st in states:
                st.iterate(warmup)
            per_it = timed_iterate(lib, states[0], 32) / 32   # one measurement near `seconds`
            ks[key] = int(max(32, min(iters, 1e3 * seconds / max(per_it, 1e-6))))
        rate = {"single": [], "concat": [], "many": []}
        for _ in range(repeats):   # alternating
            rate["many"].append(count * ks["many"] * 1e3 / timed_iterate(lib, many, ks["many"]))
            rate["single"].append(1e3 / np.mean([timed_iterate(lib, st, ks["single"]) / ks["single"] for st in singles]))
            rate["concat"].append(count * ks["concat"] * 1e3 / timed_iterate(lib, concat, ks["concat"]))
        ms = many.bench(ks["many"])
        many.close()
        concat.close()
        for st in singles:
            st.close()
        point = {"N": count, "forms": forms, "iterations_per_measurement": ks,
                 "ms_per_iteration_many": float(ms[0]), "ms_primal_half": float(ms[1]), "ms_dual_half": float(ms[2])}
        for key, v in rate.items():
            point[f"{key}_lp_it_per_s"] = float(np.median(v))
            point[f"{key}_repeats"] = [float(x) for x in v]
            point[f"{key}_spread"] = spread(v)
        point["many_beats_both_beyond_spread"] = bool(min(rate["many"]) > max(max(rate["single"]), max(rate["concat"])))
        point["ratio_to_single"] = point["many_lp_it_per_s"] / point["single_lp_it_per_s"]
        point["ratio_to_concat"] = point["many_lp_it_per_s"] / point["concat_lp_it_per_s"]
        points.append(point)
        print(f"[{name}] N={count} ({'/'.join(forms)}): many {point['many_lp_it_per_s']:.0f}, single {point['single_lp_it_per_s']:.0f}, "
              f"concat {point['concat_lp_it_per_s']:.0f} LP-it/s; {ms[0] * 1e3:.1f} us per iteration of the set", file=sys.stderr)
    wins = None
    for q in reversed(points):
        if q["concat_lp_it_per_s"] > q["many_lp_it_per_s"]:
            wins = q["N"]
        else:
            break
    c = problem[0]
    return {"set": name, "n": int(c.size), "m_eq": int(problem[1].shape[0]), "m_ineq": int(problem[3].shape[0]),
            "doubles_2n_plus_m": int(2 * c.size + problem[1].shape[0] + problem[3].shape[0]), "points": points, "concat_wins_from": wins}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("outdir")
    p.add_argument("--sets", default="sc105,potts50")
    p.add_argument("--counts-sc105", default="1,16,256,1024")
    p.add_argument("--counts-potts50", default="1,16,256")
    p.add_argument("--iters", type=int, default=2000)
    p.add_argument("--warmup", type=int, default=200)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--seconds", type=float, default=0.3)
    p.add_argument("--seed", type=int, default=0)
    args = p.parse_args()
    assert args.repeats >= 1 and args.iters >= 32

    from conftest import load_golden
    from test_oracle_golden import _reduced
    from pysparselp_amd import _lib
    from pysparselp_amd.ChambollePockPPD import many_lds_limit

    lib = _lib.lib()
    out = {"method": "chambolle_pock_ppd_many", "box": platform.node(), "device": "AMD Instinct MI355X (gfx950)",
           "iterations": args.iters, "warmup": args.warmup, "repeats": args.repeats, "lds_limit_doubles": many_lds_limit(), "sets": []}
    for name in args.sets.split(","):
        counts = [int(v) for v in getattr(args, "counts_" + name).split(",")]
        w = measure(lib, name, _reduced(load_golden("lp_" + name)), counts, args.iters, args.warmup, args.repeats, args.seconds, args.seed)
        if name == "sc105":
            at = [q for q in w["points"] if q["N"] == 256]
            if at:
                w["holds_at_256"] = at[0]["many_beats_both_beyond_spread"]
        out["sets"].append(w)
    line = json.dumps(out)
    print(line)
    os.makedirs(args.outdir, exist_ok=True)
    with open(os.path.join(args.outdir, "cp_many.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
