"""The lists of LPs dual gradient ascent on a list (``dual_gradient_ascent_many``, csrc/slp_dga_many.hip) is tested on:
tests/test_dga_many_host.py without a GPU, tests/test_gpu_dga_many.py on one.  Built from the fixtures and batches of
tests/dga_batch_cases.py; computed once per process, do not modify."""
from conftest import load_golden
from dga_batch_cases import BATCH_CASES, batch_case
from test_dga_host import dga_args

_CACHE = {}


class LP:
    """The attributes dual_gradient_ascent reads."""

    def __init__(self, c, a_eq, b_eq, a_ineq, b_upper, lb, ub, b_lower=None):
        self.costsvector, self.a_equalities, self.b_equalities = c, a_eq, b_eq
        self.a_inequalities, self.b_upper, self.b_lower = a_ineq, b_upper, b_lower
        self.lower_bounds, self.upper_bounds = lb, ub


def mixed_list():
    """Twelve ``(case, cost index, args)``: the four batch fixtures in rotation (176 x 224 with inequalities only, 60 x (10 + 80)
    twice, 48 x (20 + 30)), cost indices 0 .. 5 in rotation; ``args`` as ``dga_cpu`` takes them."""
    if "mixed" not in _CACHE:
        out = []
        for k in range(12):
            case, cost = BATCH_CASES[k % 4], k % 6
            args, six = batch_case(case)
            out.append((case, cost, (six[cost],) + tuple(args[1:])))
        _CACHE["mixed"] = out
    return _CACHE["mixed"]


def extra_list():
    """Four ``(name, args)`` beyond the mixed list: SC105, an equality-only LP (the equality rows of SC50A), an inequality-only LP
    (SC50A's inequality rows over a 0-row equality block) and Potts-50 (n = 7400: npad 8192, the LDS maximum; 9800 rows)."""
    if "extra" not in _CACHE:
        c, a_eq, b_eq, a_ineq, b_upper, lb, ub = dga_args(load_golden("lp_sc50a"))
        _CACHE["extra"] = [
            ("sc105", dga_args(load_golden("lp_sc105"))),
            ("equalities_only", (c, a_eq, b_eq, None, None, lb, ub)),
            ("inequalities_only", (c, a_eq[:0].tocsr(), b_eq[:0], a_ineq, b_upper, lb, ub)),
            ("potts50", dga_args(load_golden("lp_potts50"))),
        ]
    return _CACHE["extra"]


def rows_of(args):
    """``(m_eq, m_ineq)`` of an LP given as ``dga_cpu`` takes it."""
    return (0 if args[1] is None else args[1].shape[0]), (0 if args[3] is None else args[3].shape[0])
