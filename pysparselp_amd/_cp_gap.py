"""The certificate of the single Chambolle-Pock solver (``slp_cp``; include/slp_hip_ext_cp_gap.h) as methods of its two wrappers,
``ChambollePockPPD.CPState`` and ``scale.DeviceCP`` (``self._l`` the library, ``self._h`` the handle), and the certificate of a
box vertex on the host for an LP without rows."""
import ctypes

import numpy as np

from . import _lib
from . import _many


def check_gap(tol_gap, tol_feas, check_every):
    """``(tol_gap, tol_feas, check_every)`` as two floats and an int, or ``ValueError``; touches no library."""
    tol_gap, check_every = _many.check_stop(tol_gap, check_every, "tol_gap")
    tol_feas, _ = _many.check_stop(tol_feas, check_every, "tol_feas")
    return tol_gap, tol_feas, check_every


class CPGapMethods:
    def certificate(self):
        """``(primal, bound, violation)`` of the current iterate ``(x_t, y_t)``, between whole iterations, for the LP the solver
        holds (``K = [A_eq; A_ineq]`` one-sided): ``primal = c.x_t``, the lower bound ``sum_j min(d_j lb_j, d_j ub_j) - y_t.b`` with
        ``d = c + K^T y_t`` in the bits of the next primal half (terms with ``d_j == 0`` or ``y_r == 0`` left out; ``-inf`` where a
        free variable has ``d_j`` of the wrong sign) and ``violation = max(max|A_eq x_t - b_eq|, max(A_ineq x_t - b_ineq), 0)``.
        Changes neither the iterate nor the armed test.  Under a communicator every rank calls it and gets the same numbers."""
        out = np.zeros(3)
        _lib.check(self._l.slp_cp_certificate(self._h, _lib.ptr(out)))
        return float(out[0]), float(out[1]), float(out[2])

    def set_stop_gap(self, tol_gap, tol_feas, check_every=1):
        """Arms the certificate as the stopping test (``slp_cp_set_stop_gap``).  The state counts its whole iterations ``t`` from 1
        over its life, those before the arming included; ``primal_step`` then ``dual_step`` is one.  ``iterate`` is cut at every
        ``t`` with ``t % check_every == 0``, where the certificate is evaluated and read back (one synchronising read per check);
        the state stops iff ``violation <= tol_feas`` and ``|primal - bound| <= tol_gap * (1 + |primal| + |bound|)`` with a finite
        left-hand side.  A stopped state does not move -- ``iterate``, ``primal_step`` and ``dual_step`` do nothing -- until this is
        called again; its ``x``, ``y`` after ``t`` iterations are bit for bit the unarmed state's.  ``tol_gap=None`` disarms."""
        if tol_gap is None:
            tol_gap, tol_feas, check_every = -1.0, 0.0, 1
        else:
            tol_gap, tol_feas, check_every = check_gap(tol_gap, tol_feas, check_every)
        _lib.check(self._l.slp_cp_set_stop_gap(self._h, tol_gap, tol_feas, check_every))

    def gap_state(self):
        """``(iterations, stopped, primal, bound, violation)``: the whole iterations completed, whether the state is stopped, and
        the numbers of the last certificate a check evaluated (``+inf``, ``-inf``, ``+inf`` before the first)."""
        iterations, stopped = ctypes.c_int64(0), ctypes.c_int32(0)
        numbers = np.zeros(3)
        base = numbers.ctypes.data
        _lib.check(self._l.slp_cp_gap_state(self._h, ctypes.addressof(iterations), ctypes.addressof(stopped), base, base + 8, base + 16))
        return int(iterations.value), bool(stopped.value), float(numbers[0]), float(numbers[1]), float(numbers[2])


def vertex_certificate(c, x):
    """``info`` of an LP without rows at its box vertex ``x``: optimal, so primal and bound are its value."""
    value = float(np.dot(c, x))
    return dict(iterations=0, stopped=True, primal=value, lower_bound=value, violation=0.0)
