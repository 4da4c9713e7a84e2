"""Batched ADMM (ADMMBatchState, csrc/slp_admm_batch.hip) measured against the single-instance solver of the same library.

    timeout -k 10 900 python tools/bench_admm_batch.py OUTDIR [--workload potts|random|both] [--potts 256]
                                          [--rows 30000 --cols 20000 --density 5e-4] [--batches 1,8,16,64,128,256]
                                          [--random-batches 1,8,64,256] [--target-ms 400] [--warmup 3] [--repeats 3]

Writes one JSON line (stdout and OUTDIR/admm_batch.json).  Per workload, batch size B and configuration -- the form and tile
width the library's rule chooses ("default"), and forced ones (SLP_ADMM_BATCH_FORM, SLP_ADMM_BATCH_TILE): both forms, the tile
form at widths 1, 4 and 16 -- `repeats` times in turn, in ONE process: the batched solver (slp_admm_batch_bench: HIP events around
k iterations, after a warm-up) and the unchanged single-instance solver on instance 0 of the same LP (slp_admm_bench, default
plan: bands on Potts).  k is chosen per point so that one measurement takes about `target-ms`.  Recorded per point: ms per batched
iteration, instance-iterations/s = B x 1000 / ms (median and every repeat), the single-instance it/s of the same turns, the ratio
of the medians and the spread of the repeats ((max - min) / median).

Workload 1: the Potts n x n LP (problems.potts_lp), instance costs = seeded perturbations of the unary costs.
Workload 2: the synthetic random LP (problems.random_lp_on_device, the device restatement of the generator behind the golden
random fixtures, 10 % equality rows) at rows x cols: small enough for M to be formed and planned in seconds.

`holds_at_64`: on Potts at B = 64, default configuration, the slowest batched repeat's instance-iterations/s exceeds the fastest
repeat of the single-instance solver in the same run.

Every GPU step of a run belongs under a time limit of its own, as in the usage line above.
"""
import argparse
import json
import os
import platform
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from _bench_util import spread  # noqa: E402


def batch_state(cs, lp_args, form, width):
    """ADMMBatchState with the form / tile width forced through the environment (None: the library's rule)."""
    from pysparselp_amd import ADMMBatchState

    names = {"SLP_ADMM_BATCH_FORM": form, "SLP_ADMM_BATCH_TILE": None if width is None else str(width)}
    saved = {k: os.environ.get(k) for k in names}
    for k, v in names.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        return ADMMBatchState(cs, *lp_args)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def configurations(batch, both_wide):
    cfg = [("default", None, None), ("tile", "tile", 1), ("levels", "levels", None)]
    if batch >= 4 and both_wide:
        cfg.append(("tile", "tile", 4))
    if batch >= 16 and both_wide:
        cfg.append(("tile", "tile", 16))
    return cfg


def measure(name, c, lp_args, batches, perturb, seed, target_ms, warmup, repeats, both_wide):
    from pysparselp_amd import ORDER_AUTO
    from pysparselp_amd.ADMM import ADMMState

    a_eq, beq, a_ineq, bl, bu, lb, ub = lp_args
    single = ADMMState.from_lp(c, a_eq, beq, a_ineq, bl, bu, lb, ub, None, 2, 3, True, order=ORDER_AUTO)
    single.iterate(warmup)
    ks = int(min(2000, max(5, target_ms / single.bench(5))))
    points = []
    for batch in batches:
        cs = np.tile(c, (batch, 1))
        cs[1:] += perturb(np.random.RandomState(seed + batch), batch - 1)
        for label, form, width in configurations(batch, both_wide):
            st = batch_state(cs, lp_args, form, width)
            st.iterate(warmup)
            k = int(min(2000, max(3, target_ms / st.bench(3))))
            ms_b, ms_s = [], []
            for _ in range(repeats):   # alternating
                ms_b.append(st.bench(k))
                ms_s.append(single.bench(ks))
            used_form, levels = st.form(), st.num_levels()
            st.close()
            inst, one = batch * 1e3 / np.array(ms_b), 1e3 / np.array(ms_s)
            points.append({
                "B": batch, "configuration": label, "form": used_form, "forced_tile_width": width, "levels": levels,
                "iterations_per_measurement": k, "single_iterations_per_measurement": ks,
                "ms_per_batched_iteration": float(np.median(ms_b)), "instance_it_per_s": float(np.median(inst)),
                "instance_it_per_s_repeats": inst.tolist(), "batched_spread": spread(inst),
                "single_it_per_s": float(np.median(one)), "single_repeats": one.tolist(), "single_spread": spread(one),
                "ratio_to_single": float(np.median(inst) / np.median(one)),
                "beats_single_beyond_spread": bool(inst.min() > one.max()),
            })
            q = points[-1]
            print(f"[{name}] B={batch} {label}/{used_form}/w={width}: {q['ms_per_batched_iteration']:.3f} ms, "
                  f"{q['instance_it_per_s']:.0f} instance-it/s, single {q['single_it_per_s']:.0f} it/s, x{q['ratio_to_single']:.2f}", file=sys.stderr)
    out = {"workload": name, "n": int(c.size), "m_eq": 0 if a_eq is None else int(a_eq.shape[0]), "m_ineq": int(a_ineq.shape[0]),
           "single_bands": single.num_bands(), "single_levels": single.num_levels(), "points": points}
    single.close()
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("outdir")
    p.add_argument("--workload", default="both", choices=("potts", "random", "both"))
    p.add_argument("--potts", type=int, default=256)
    p.add_argument("--rows", type=int, default=30000)
    p.add_argument("--cols", type=int, default=20000)
    p.add_argument("--density", type=float, default=5e-4)
    p.add_argument("--batches", default="1,8,16,64,128,256")
    p.add_argument("--random-batches", default="1,8,64,256")
    p.add_argument("--target-ms", type=float, default=400.0)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--seed", type=int, default=0)
    args = p.parse_args()
    assert args.repeats >= 1

    from pysparselp_amd import _lib
    from pysparselp_amd.problems import potts_lp, random_lp_on_device

    _lib.lib()
    out = {"method": "lp_admm_batch", "box": platform.node(), "device": "AMD Instinct MI355X (gfx950)", "target_ms": args.target_ms,
           "warmup": args.warmup, "repeats": args.repeats, "workloads": []}
    if args.workload in ("potts", "both"):
        lp, _, pix, _ = potts_lp(args.potts)
        npix = pix.size

        def perturb(rs, count, n=lp.nb_variables):
            d = np.zeros((count, n))
            d[:, :npix] = 0.3 * rs.randn(count, npix)   # the unary costs (the pixel variables come first)
            return d

        w = measure(f"potts{args.potts}", lp.costsvector, (None, None, lp.a_inequalities, lp.b_lower, lp.b_upper, lp.lower_bounds,
                                                          lp.upper_bounds), [int(v) for v in args.batches.split(",")], perturb, args.seed,
                    args.target_ms, args.warmup, args.repeats, both_wide=True)
        at64 = [q for q in w["points"] if q["B"] == 64 and q["configuration"] == "default"]
        if at64:
            w["holds_at_64"] = at64[0]["beats_single_beyond_spread"]
        out["workloads"].append(w)
    if args.workload in ("random", "both"):
        m_eq = args.rows // 10
        a, _, c, lb, ub, b = random_lp_on_device(args.cols, args.rows, args.density, seed=args.seed, m_eq=m_eq)
        host = a.download().tocsr()
        a.close()
        scale = float(np.mean(np.abs(c)))
        lp_args = (host[:m_eq], b[:m_eq], host[m_eq:], None, b[m_eq:], lb, ub)
        w = measure(f"random_{args.rows}x{args.cols}_d{args.density:g}", c, lp_args, [int(v) for v in args.random_batches.split(",")],
                    lambda rs, count: 0.2 * scale * rs.randn(count, c.size), args.seed, args.target_ms, args.warmup, args.repeats,
                    both_wide=False)
        out["workloads"].append(w)
    line = json.dumps(out)
    print(line)
    os.makedirs(args.outdir, exist_ok=True)
    with open(os.path.join(args.outdir, "admm_batch.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
