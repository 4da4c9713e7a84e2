"""Dual gradient ascent on a list of LPs (DeviceDGAMany, csrc/slp_dga_many.hip: one workgroup per LP, whole iterations inside a
launch) measured against the same LPs through the single-instance solver one after another (DeviceDGA, csrc/slp_dga.hip, on its
own automatic path), in ONE process and ONE run.

    python tools/bench_dga_many.py OUTDIR [--counts 1,8,64,256,1024] [--grids 8,9,...,16] [--warmup 20] [--repeats 3]

Writes one JSON line (stdout and OUTDIR/dga_many.json).  The LPs are Potts LPs of the package's own builder (problems.potts_lp),
grids 8 x 8 to 16 x 16 in rotation, the unary costs of LP k perturbed with seed k (distinct costs).  Per N: the list form's
instance-iterations per second (N x iterations of the list / time), the partner's (the N single solvers iterated one after
another, the same number of iterations each), their ratio, and as a second line the ceiling a shared matrix gives: the batched
solver (DeviceDGABatch, fused search) on the 12 x 12 LP with N costs.  Every rate is a pair of HIP events (slp_timer_start /
_stop) around the timed iterations, after a warm-up, the draw buffers filled beforehand so that nothing is read back in between;
`repeats` measurements alternate between the list form, the partner and the batch; the median is reported with all repeats.
Shipping condition `many_above_single_at_256`: at N = 256 the list form's slowest repeat is above the partner's fastest.
Reads nothing outside the repository."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from _bench_util import timed_between_events  # noqa: E402


class LP:
    def __init__(self, c, a_eq, b_eq, a_ineq, b_upper, lb, ub):
        self.costsvector, self.a_equalities, self.b_equalities = c, a_eq, b_eq
        self.a_inequalities, self.b_upper, self.b_lower = a_ineq, b_upper, None
        self.lower_bounds, self.upper_bounds = lb, ub


def potts_list(count, grids):
    from pysparselp_amd.problems import potts_lp

    base = {}
    out = []
    for k in range(count):
        size = grids[k % len(grids)]
        if size not in base:
            lp, _, pix, _ = potts_lp(size)
            assert lp.b_lower is None or np.max(lp.b_lower) == -np.inf
            base[size] = (lp, pix.size)
        lp, npix = base[size]
        c = np.array(lp.costsvector, dtype=np.float64)
        c[:npix] += 0.3 * np.random.RandomState(1000 + k).randn(npix)   # the unary costs come first
        out.append(LP(c, lp.a_equalities, lp.b_equalities, lp.a_inequalities, lp.b_upper, lp.lower_bounds, lp.upper_bounds))
    return out


def fill(state, k):
    """Two draws per iteration to come behind the furthest position, so that `k` iterations read nothing back."""
    left = state.status()[2]
    if left < 2 * k:
        state.push_random(state._draws(2 * k - left))


def timed(lib, states, k):
    """Milliseconds for `k` iterations of every state, one state after another, between two HIP events."""
    return timed_between_events(lib, states, k, fill)


def iterations_for(lib, states, target_ms, cap):
    return int(min(cap, max(5, target_ms / max(timed(lib, states, 5) / 5, 1e-6))))


def measure(count, grids, warmup, repeats, target_ms):
    from pysparselp_amd import _lib
    from pysparselp_amd.DualGradientAscent import DeviceDGA, DeviceDGABatch, DeviceDGAMany, _dga_many_lp, dga_many_start
    from pysparselp_amd.device import DeviceMatrix

    lib = _lib.lib()
    lps = potts_list(count, grids)
    forms = [_dga_many_lp(k, lp) for k, lp in enumerate(lps)]
    y0s, offsets = dga_many_start(forms)
    many = DeviceDGAMany(forms, y0s, offsets)
    singles, mats = [], []
    for lp, y0 in zip(lps, y0s):
        m_eq = lp.a_equalities.shape[0]
        mat = DeviceMatrix.from_blocks(lp.a_equalities if m_eq else None, lp.a_inequalities, lp.costsvector.size)
        rs = np.random.RandomState(0)
        rs.random_sample(y0.size)   # the start's draws
        b = np.concatenate((lp.b_equalities if m_eq else np.zeros(0), lp.b_upper))
        singles.append(DeviceDGA(mat, b, lp.costsvector, lp.lower_bounds, lp.upper_bounds, y0, m_eq=m_eq, draws=rs.random_sample))
        mats.append(mat)
    # the ceiling of a shared matrix: N costs over the LP of the middle grid
    mid = potts_list(len(grids), grids)[len(grids) // 2]
    m_eq = mid.a_equalities.shape[0]
    bmat = DeviceMatrix.from_blocks(mid.a_equalities if m_eq else None, mid.a_inequalities, mid.costsvector.size)
    rs = np.random.RandomState(0)
    m = bmat.shape[0]
    y0 = np.concatenate((-rs.rand(m_eq), np.abs(rs.rand(m - m_eq))))
    costs = np.tile(mid.costsvector, (count, 1))
    costs[1:] += 0.01 * np.random.RandomState(5).randn(count - 1, costs.shape[1])
    batch = DeviceDGABatch(bmat, np.concatenate((mid.b_equalities if m_eq else np.zeros(0), mid.b_upper)), costs, mid.lower_bounds,
                           mid.upper_bounds, y0, m_eq=m_eq, draws=rs.random_sample, path="fused")
    sets = {"many": [many], "single": singles, "batch": [batch]}
    for states in sets.values():
        for st in states:
            st.iterate(warmup)
    k = {name: iterations_for(lib, states, target_ms, 2000) for name, states in sets.items()}
    ms = {name: [] for name in sets}
    for _ in range(repeats):   # alternating
        for name, states in sets.items():
            ms[name].append(timed(lib, states, k[name]))
    many.timing(True)
    fill(many, k["many"])
    many.iterate(k["many"], refill=False)
    many.timing(False)
    split = {name: v / k["many"] for name, v in many.timing_read().items()}
    assert not np.any(many.status()[0]), many.status()[0]
    rate = {name: count * k[name] * 1e3 / np.array(v) for name, v in ms.items()}   # instance-iterations per second
    point = {"N": count, "n_min": int(min(f[0].size for f in forms)), "n_max": int(max(f[0].size for f in forms)),
             "iterations_per_launch_cap": many.kmax(), "iterations_per_measurement": k,
             "many_instance_it_per_s": float(np.median(rate["many"])), "many_repeats": rate["many"].tolist(),
             "single_instance_it_per_s": float(np.median(rate["single"])), "single_repeats": rate["single"].tolist(),
             "batch_shared_matrix_instance_it_per_s": float(np.median(rate["batch"])), "batch_repeats": rate["batch"].tolist(),
             "ratio_to_single": float(np.median(rate["many"]) / np.median(rate["single"])),
             "many_slowest_above_single_fastest": bool(rate["many"].min() > rate["single"].max()),
             "many_ms_per_iteration_by_stage": split}
    for states in sets.values():
        for st in states:
            st.close()
    for mat in mats + [bmat]:
        mat.close()
    print(f"N={count}: list {point['many_instance_it_per_s']:.0f}, one after another {point['single_instance_it_per_s']:.0f}, shared matrix "
          f"{point['batch_shared_matrix_instance_it_per_s']:.0f} instance-it/s; x {point['ratio_to_single']:.2f}", file=sys.stderr)
    return point


def main():
    p = argparse.ArgumentParser()
    p.add_argument("outdir")
    p.add_argument("--counts", default="1,8,64,256,1024")
    p.add_argument("--grids", default="8,9,10,11,12,13,14,15,16")
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--target-ms", type=float, default=400.0)
    args = p.parse_args()
    assert args.repeats >= 1
    grids = [int(v) for v in args.grids.split(",")]
    out = {"method": "dual_gradient_ascent_many", "device": "AMD Instinct MI355X (gfx950)", "grids": grids, "warmup": args.warmup,
           "repeats": args.repeats, "points": []}
    for count in (int(v) for v in args.counts.split(",")):
        out["points"].append(measure(count, grids, args.warmup, args.repeats, args.target_ms))
    at256 = [q for q in out["points"] if q["N"] == 256]
    if at256:
        out["many_above_single_at_256"] = bool(at256[0]["many_slowest_above_single_fastest"])
    line = json.dumps(out)
    print(line)
    os.makedirs(args.outdir, exist_ok=True)
    with open(os.path.join(args.outdir, "dga_many.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
