"""Compaction for the Chambolle-Pock list solver (CPManyState.set_compaction, csrc/slp_many.h k_many_live, csrc/slp_cp_many.hip
k_cpm_iterate<., true, true> and k_cpm_iterate_gap<., true>): that the kernels without it are the parent's, what the live lists
cost when nothing retires, and what they buy when LPs retire here and there.

    python tools/bench_cp_many_live.py OUTDIR [--parts a,b,c] [--parent-repo DIR] [--counts 1,16,256,1024] [--counts-price 256,1024]
                                              [--pruned 1024] [--check-every 10] [--iters 2000] [--warmup 200] [--repeats 3]
                                              [--seconds 0.3] [--screen 3000]

Writes one JSON line (stdout and OUTDIR/cp_many_live.json).  The three parts and the method are tools/_bench_many_live.py's.
Here: the sets of tools/bench_cp_many.py (SC105 and Potts-50, perturbed; Potts-50 up to N = 256); the kernels of part (a) are the
one never armed, the step test and the certificate; part (b) arms the certificate on the SC105 set; part (c) stops on the
certificate at 1e-2 / 1e-2 (profiles/cp_many_gap.json part (c) gives the stopping iterations): in the lds form random0 (50)
against Potts 10 x 10 (530) -- workgroups of 512 lanes -- to 600 iterations, and with the form forced to global Potts 8 x 8 (60)
against Potts 16 x 16 (970) -- workgroups of 1024 lanes, one of them resident per compute unit -- to 1000.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _bench_many_live as live  # noqa: E402
from bench_cp_many import perturbed  # noqa: E402
from bench_cp_many_stop import fixture, many_state, mixed_kinds  # noqa: E402


class Solver:
    kernels = ("unarmed", "step", "gap")
    price_set = "sc105"
    state = staticmethod(many_state)

    @staticmethod
    def sets(args):
        counts = [int(v) for v in args.counts.split(",")]
        return [("sc105", counts), ("potts50", [c for c in counts if c <= 256])]

    @staticmethod
    def draw(name, count, seed):
        return perturbed(fixture(name), count, seed)

    @staticmethod
    def arm(st, kernel, tol, every):
        if kernel == "gap":
            st.set_stop_gap(tol, tol, every)
        else:
            st.set_stop(tol, every)

    @staticmethod
    def records(st, kernel):
        return st.gap_state() if kernel == "gap" else st.stop_state()

    @staticmethod
    def force_form(form):
        if form is None:
            os.environ.pop("SLP_CP_MANY_FORM", None)
        else:
            os.environ["SLP_CP_MANY_FORM"] = form

    @staticmethod
    def shape(problem):
        return [int(problem[0].size), int((0 if problem[1] is None else problem[1].shape[0]) + problem[3].shape[0])]

    @staticmethod
    def pair(args, form):
        kinds = dict(mixed_kinds())
        fast, slow, horizon = ("random0", "potts10", 600) if form == "lds" else ("potts8", "potts16", 1000)
        return (fast, kinds[fast]), (slow, kinds[slow]), "gap", 1e-2, horizon


def main():
    p = argparse.ArgumentParser()
    live.add_arguments(p)
    live.run(Solver, p, os.path.abspath(__file__), REPO, "chambolle_pock_ppd_many, compact", "cp_many_live.json")


if __name__ == "__main__":
    main()
