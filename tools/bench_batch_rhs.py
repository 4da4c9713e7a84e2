"""Right-hand sides per instance for the batched dual gradient ascent and the batched ADMM solver: what the capability costs.

    python tools/bench_batch_rhs.py OUTDIR [--parent NAME] [--rounds 3] [--repeats 3] [--batch 64]

Writes one JSON line (stdout and OUTDIR/batch_rhs.json).  The lists are those of tools/bench_dga_batch.py (Potts-256 on the general
search with the global sort, Potts-50 on the fused search) and of tools/bench_admm_batch.py (Potts-256, both forms, and its
30 000 x 20 000 random LP with 10 % equality rows in the library's own form), B = 64.  The Potts LPs have no equality rows, so
under ADMM only their ``b_upper`` can be batched (``ub`` becomes tiled, ``b`` stays shared); the random LP batches ``beq`` and
``b_upper``: the tiled ``b``, the kernels that address it and the B products A^T b_k of ``set_rhs``.

1. States that never call ``set_rhs``, this library against the parent commit's.  Two libraries cannot share a process, so child
   processes alternate (parent, this) ``rounds`` times; ``--parent NAME`` names the parent's build, pysparselp_amd/libslp_hip_NAME.so
   (loaded through SLP_LIB_VARIANT).  To produce it: check the parent commit out beside this tree (``git worktree add DIR HEAD~1``),
   ``make -C DIR/pysparselp_amd/csrc``, and copy DIR/pysparselp_amd/libslp_hip.so to pysparselp_amd/libslp_hip_NAME.so (git ignores
   it).  The parent's child runs this tree's Python on that library -- the Python layer of a state that never calls ``set_rhs`` is
   unchanged -- without binding the two entry points the parent lacks.  A child times every point with HIP events, the median of
   ``repeats``.  Condition, fixed beforehand: median(this) / median(parent) of the instance-iterations/s >= 1 - the parent's own
   spread between its rounds.
2. Batched against shared right-hand sides, in ONE process of this library, alternating repeats: the ratio of the
   instance-iterations/s, and the time of ``set_rhs`` itself (wall clock around the synchronising call, the median of ``repeats``).
Reads nothing outside the repository."""
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

from _bench_util import spread, timed_between_events  # noqa: E402

DGA_POINTS = (("potts256", 256, "general", "global"), ("potts50", 50, "fused", None))
ADMM_POINTS = (("potts256", 256, "tile"), ("potts256", 256, "levels"), ("random_30000x20000_d0.0005", None, None))
RANDOM_LP = dict(rows=30000, cols=20000, density=5e-4)   # tools/bench_admm_batch.py's random workload: 10 % equality rows


def potts_costs(lp, npix, batch, seed):
    costs = np.tile(lp.costsvector, (batch, 1))
    costs[1:, :npix] += 0.3 * np.random.RandomState(seed + batch).randn(batch - 1, npix)   # the unary costs come first
    return costs


def moved(b, batch, seed, direction=0):
    """Row 0 is ``b``; row k >= 1 moves every finite entry by 0.1 (1 + |b|) randn (upwards only with direction > 0)."""
    out = np.tile(np.asarray(b, dtype=np.float64), (batch, 1))
    move = 0.1 * (1 + np.abs(np.where(np.isfinite(b), b, 0.0))) * np.random.RandomState(seed).randn(batch - 1, np.size(b))
    out[1:] = np.where(np.isfinite(b), b + (np.abs(move) if direction > 0 else move), b)
    return out


def dga_ms(lib, state, k):
    return timed_between_events(lib, [state], k, lambda st, k: st.push_random(np.random.RandomState(17).random_sample(2 * k + 2))) / k


def child(batch, repeats, with_rhs, seed=0):
    """Every point of both lists in this process's library; with_rhs: also a state with batched right-hand sides, alternating."""
    from pysparselp_amd import _lib

    if not with_rhs:   # the parent's library has no set_rhs to bind
        _lib._EXT_BATCH_RHS_SIGNATURES.clear()
    from pysparselp_amd import ADMMBatchState
    from pysparselp_amd.DualGradientAscent import DeviceDGABatch
    from pysparselp_amd.device import DeviceMatrix
    from pysparselp_amd.problems import potts_lp

    lib = _lib.lib()
    points = []
    lps = {}
    for name, size, path, sort in DGA_POINTS:
        lp, _, pix, _ = lps.setdefault(size, potts_lp(size))
        a_eq, a_ineq = lp.a_equalities, lp.a_inequalities
        m_eq = a_eq.shape[0]
        b = np.concatenate((lp.b_equalities if m_eq else np.zeros(0), lp.b_upper))
        mat = DeviceMatrix.from_blocks(a_eq if m_eq else None, a_ineq, lp.costsvector.size)
        costs = potts_costs(lp, pix.size, batch, seed)

        def state():
            rs = np.random.RandomState(0)
            y0 = np.concatenate((-rs.rand(m_eq), np.abs(rs.rand(mat.shape[0] - m_eq))))
            os.environ.pop("SLP_DGA_BATCH_SORT", None)
            if sort:
                os.environ["SLP_DGA_BATCH_SORT"] = sort
            st = DeviceDGABatch(mat, b, costs, lp.lower_bounds, lp.upper_bounds, y0, m_eq=m_eq, draws=rs.random_sample, path=path)
            os.environ.pop("SLP_DGA_BATCH_SORT", None)
            return st

        shared = state()
        states, set_ms = [shared], []
        if with_rhs:
            rows = np.ascontiguousarray(np.concatenate((moved(b[:m_eq], batch, 5), moved(b[m_eq:], batch, 6, +1)), axis=1))
            own = state()
            for _ in range(repeats):
                t0 = time.perf_counter()
                own.set_rhs(rows)
                set_ms.append(1e3 * (time.perf_counter() - t0))
            states.append(own)
        for st in states:
            st.iterate(20)
        k = int(min(2000, max(10, 500.0 / dga_ms(lib, shared, 5))))
        ms = [[] for _ in states]
        for _ in range(repeats):   # alternating
            for i, st in enumerate(states):
                ms[i].append(dga_ms(lib, st, k))
        for st in states:
            assert not np.any(st.status()[0])
            st.close()
        mat.close()
        q = {"solver": "dga", "workload": name, "path": path + ("-" + sort if sort else ""), "B": batch, "iterations_per_measurement": k,
             "shared_instance_it_per_s": (batch * 1e3 / np.array(ms[0])).tolist()}
        if with_rhs:
            q.update(batched_instance_it_per_s=(batch * 1e3 / np.array(ms[1])).tolist(), set_rhs_ms=set_ms)
        points.append(q)
    for name, size, form in ADMM_POINTS:
        if size is None:   # the random LP: equality rows, so beq is batched too
            from pysparselp_amd.problems import random_lp_on_device

            r = RANDOM_LP
            m_eq = r["rows"] // 10
            a, _, c, lb, ub, b = random_lp_on_device(r["cols"], r["rows"], r["density"], seed=seed, m_eq=m_eq)
            host = a.download().tocsr()
            a.close()
            cs = np.tile(c, (batch, 1))
            cs[1:] += 0.2 * float(np.mean(np.abs(c))) * np.random.RandomState(seed + batch).randn(batch - 1, c.size)
            lp_args = (host[:m_eq], b[:m_eq], host[m_eq:], None, b[m_eq:], lb, ub)
            sides = dict(beq=moved(b[:m_eq], batch, 8), b_upper=moved(b[m_eq:], batch, 9, +1))
        else:
            lp, _, pix, _ = lps.setdefault(size, potts_lp(size))
            cs = potts_costs(lp, pix.size, batch, seed)
            lp_args = (None, None, lp.a_inequalities, lp.b_lower, lp.b_upper, lp.lower_bounds, lp.upper_bounds)
            sides = dict(b_upper=moved(lp.b_upper, batch, 7, +1))
        os.environ.pop("SLP_ADMM_BATCH_FORM", None)
        if form:
            os.environ["SLP_ADMM_BATCH_FORM"] = form

        def state():
            return ADMMBatchState(cs, *lp_args)

        shared = state()
        states, set_ms = [shared], []
        if with_rhs:
            own = state()
            for _ in range(repeats):
                t0 = time.perf_counter()
                own.set_rhs(**sides)
                set_ms.append(1e3 * (time.perf_counter() - t0))
            states.append(own)
        for st in states:
            st.iterate(3)
        k = int(min(2000, max(3, 400.0 / shared.bench(3))))
        ms = [[] for _ in states]
        for _ in range(repeats):   # alternating
            for i, st in enumerate(states):
                ms[i].append(st.bench(k))
        used = shared.form()
        assert form in (None, used)
        for st in states:
            st.close()
        os.environ.pop("SLP_ADMM_BATCH_FORM", None)
        q = {"solver": "admm", "workload": name, "path": used, "B": batch, "iterations_per_measurement": k,
             "shared_instance_it_per_s": (batch * 1e3 / np.array(ms[0])).tolist()}
        if with_rhs:
            q.update(batched_instance_it_per_s=(batch * 1e3 / np.array(ms[1])).tolist(), set_rhs_ms=set_ms, batched_sides=sorted(sides))
        points.append(q)
    print("POINTS " + json.dumps(points))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("outdir")
    p.add_argument("--parent", default=None, help="pysparselp_amd/libslp_hip_<NAME>.so: the parent commit's build")
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--child", default=None, choices=("parent", "this"))
    args = p.parse_args()
    if args.child:
        child(args.batch, args.repeats, with_rhs=args.child == "this")
        return

    def run(which):
        env = dict(os.environ)
        env.pop("SLP_LIB_VARIANT", None)
        if which == "parent":
            env["SLP_LIB_VARIANT"] = args.parent
        out = subprocess.run([sys.executable, os.path.abspath(__file__), args.outdir, "--child", which, "--repeats", str(args.repeats),
                              "--batch", str(args.batch)], env=env, check=True, capture_output=True, text=True, timeout=600)
        line = [v for v in out.stdout.splitlines() if v.startswith("POINTS ")][-1]
        print(f"[{which}] done", file=sys.stderr)
        return json.loads(line[len("POINTS "):])

    rounds = {"parent": [], "this": []}
    for _ in range(args.rounds):
        for which in (("parent", "this") if args.parent else ("this",)):
            rounds[which].append(run(which))
    points = []
    for i, first in enumerate(rounds["this"][0]):
        q = {key: first[key] for key in ("solver", "workload", "path", "B")}
        this = np.array([np.median(r[i]["shared_instance_it_per_s"]) for r in rounds["this"]])
        q.update(this_shared_instance_it_per_s=float(np.median(this)), this_rounds=this.tolist(), this_spread=spread(this))
        if rounds["parent"]:
            par = np.array([np.median(r[i]["shared_instance_it_per_s"]) for r in rounds["parent"]])
            ratio = float(np.median(this) / np.median(par))
            q.update(parent_shared_instance_it_per_s=float(np.median(par)), parent_rounds=par.tolist(), parent_spread=spread(par),
                     this_over_parent=ratio, condition_met=bool(ratio >= 1.0 - spread(par)))
        shared = np.concatenate([r[i]["shared_instance_it_per_s"] for r in rounds["this"]])
        own = np.concatenate([r[i]["batched_instance_it_per_s"] for r in rounds["this"]])
        q.update(batched_instance_it_per_s=float(np.median(own)), batched_repeats=own.tolist(), shared_repeats=shared.tolist(),
                 batched_over_shared=float(np.median(own) / np.median(shared)),
                 set_rhs_ms=float(np.median(np.concatenate([r[i]["set_rhs_ms"] for r in rounds["this"]]))),
                 set_rhs_ms_repeats=np.concatenate([r[i]["set_rhs_ms"] for r in rounds["this"]]).tolist())
        if "batched_sides" in first:
            q["batched_sides"] = first["batched_sides"]
        points.append(q)
        print(json.dumps(q), file=sys.stderr)
    out = {"tool": "tools/bench_batch_rhs.py", "box": platform.node(), "device": "AMD Instinct MI355X (gfx950)", "rounds": args.rounds,
           "repeats": args.repeats, "condition": "this / parent >= 1 - the parent's spread between its rounds (states that never call set_rhs)",
           "condition_met": (all(q["condition_met"] for q in points) if rounds["parent"] else None), "points": points}
    line = json.dumps(out)
    print(line)
    os.makedirs(args.outdir, exist_ok=True)
    with open(os.path.join(args.outdir, "batch_rhs.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
