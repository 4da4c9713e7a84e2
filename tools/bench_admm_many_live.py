"""Compaction for the ADMM list solver (ADMMManyState.set_compaction, csrc/slp_many.h k_many_live, csrc/slp_admm_many.hip
k_admmm_iterate<., true, true>): that the kernels without it are the parent's, what the live lists cost when nothing retires, and
what they buy when LPs retire here and there.

    python tools/bench_admm_many_live.py OUTDIR [--parts a,b,c] [--parent-repo DIR] [--counts 1,16,256,1024] [--counts-price 256,1024]
                                                [--pruned 1024] [--check-every 10] [--iters 2000] [--warmup 200] [--repeats 3]
                                                [--seconds 0.3] [--screen 3000]

Writes one JSON line (stdout and OUTDIR/admm_many_live.json).  The three parts and the method are tools/_bench_many_live.py's.
Here: the Potts lists of tools/bench_admm_many.py (grids 8 x 8 to 16 x 16 in rotation); the kernels of part (a) are the one never
armed and the one with the residual and step test; part (c) stops at 1e-4 / 1e-4, where the CPU restatement
(tests/admm_stop_cpu.py) stops Potts 9 x 9 after 150 iterations and Potts 14 x 14 after 2430: that pair to 1500 iterations, in the
lds form and with the form forced to global.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _bench_many_live as live  # noqa: E402
from bench_admm_many import potts_list  # noqa: E402
from bench_admm_many_stop import GRIDS, many_state  # noqa: E402


class Solver:
    kernels = ("unarmed", "stop")
    price_set = "potts 8..16"
    state = staticmethod(many_state)

    @staticmethod
    def sets(args):
        return [("potts 8..16", [int(v) for v in args.counts.split(",")])]

    @staticmethod
    def draw(name, count, seed):
        return potts_list(count, GRIDS)

    @staticmethod
    def arm(st, kernel, tol, every):
        st.set_stop(tol, tol, every)

    @staticmethod
    def records(st, kernel):
        return st.stop_state()

    @staticmethod
    def force_form(form):
        if form is None:
            os.environ.pop("SLP_ADMM_MANY_FORM", None)
        else:
            os.environ["SLP_ADMM_MANY_FORM"] = form

    @staticmethod
    def shape(problem):
        return [int(problem[0].size), int((0 if problem[1] is None else problem[1].shape[0]) + problem[3].shape[0])]

    @staticmethod
    def pair(args, form):
        kinds = dict(zip((f"potts{g}" for g in GRIDS), potts_list(len(GRIDS), GRIDS)))
        return ("potts9", kinds["potts9"]), ("potts14", kinds["potts14"]), "stop", 1e-4, 1500


def main():
    p = argparse.ArgumentParser()
    live.add_arguments(p)
    live.run(Solver, p, os.path.abspath(__file__), REPO, "lp_admm_many, compact", "admm_many_live.json")


if __name__ == "__main__":
    main()
