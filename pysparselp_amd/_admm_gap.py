"""The certificate of the two single ADMM solvers (``slp_admm`` and ``slp_admm_cg``; include/slp_hip_ext_admm_gap.h) as methods
of their wrappers: ``ADMM.ADMMState`` and ``admm_cg._CGBase`` (through it ``ADMMCGState``, ``ADMMCGLPState`` and ``DeviceADMM``).
``self._l`` is the library, ``self._h`` the handle, ``_gap_prefix`` the entry points' prefix.  The argument checks are
``_cp_gap.check_gap``: a ``ValueError`` before any library is touched."""
import ctypes

import numpy as np

from . import _lib
from ._cp_gap import check_gap


class ADMMGapMethods:
    _gap_prefix = "slp_admm"

    def _gap_fn(self, name):
        return getattr(self._l, f"{self._gap_prefix}_{name}")

    def certificate(self):
        """``(primal, bound, violation)`` of the current iterate ``(x_t, lam_t)``, between whole iterations, for the STANDARD FORM
        the solver holds (``A`` with its slack columns, ``b``, ``c``, ``lb``, ``ub`` after the row normalisations of the set-up):
        ``primal = c.x_t``; the lower bound ``sum_j min(d_j lb_j, d_j ub_j) - yhat.b`` with ``d = c + A^T yhat``, where ``yhat`` is
        ``lam_t`` with the multiplier of a row set to 0 when it would push a slack column towards a side it has no bound on (terms
        with ``d_j == 0`` or ``yhat_i == 0`` left out; ``-inf`` where an original variable has an infinite bound on the side ``d_j``
        pushes to); ``violation = max(max|A x_t - b|, max(lb - x_t), max(x_t - ub), 0)`` in the solver's row-normalised units, those
        of ``report()[1]``, not the caller's.  It is about ``x``, the vector the drivers return, not the projected ``xp``.  Changes
        neither the iterate nor the armed test.  Under a communicator every rank calls it and gets the same numbers."""
        out = np.zeros(3)
        _lib.check(self._gap_fn("certificate")(self._h, _lib.ptr(out)))
        return float(out[0]), float(out[1]), float(out[2])

    def set_stop_gap(self, tol_gap, tol_feas, check_every=1):
        """Arms the certificate as the stopping test.  The state counts its whole iterations ``t`` from 1 over its life, those
        before the arming included; the x-step half then ``multiplier_step`` is one, and ``x_t`` is ``lp_admm(nb_iter=t - 1)``.
        ``iterate`` is cut at every ``t`` with ``t % check_every == 0``, where the certificate is evaluated and read back (one
        synchronising read per check); the state stops iff ``violation <= tol_feas`` (standard form, row-normalised units) and
        ``|primal - bound| <= tol_gap * (1 + |primal| + |bound|)`` with a finite left-hand side.  A stopped state does not move --
        ``iterate`` and the two half steps do nothing -- until this is called again; its ``x``, ``xp``, ``lam`` after ``t``
        iterations are bit for bit the unarmed state's.  ``tol_gap=None`` disarms.  Not between the two halves of an iteration."""
        if tol_gap is None:
            tol_gap, tol_feas, check_every = -1.0, 0.0, 1
        else:
            tol_gap, tol_feas, check_every = check_gap(tol_gap, tol_feas, check_every)
        _lib.check(self._gap_fn("set_stop_gap")(self._h, tol_gap, tol_feas, check_every))

    def gap_state(self):
        """``(iterations, stopped, primal, bound, violation)``: the whole iterations completed, whether the state is stopped, and
        the numbers of the last certificate a check evaluated (``+inf``, ``-inf``, ``+inf`` before the first)."""
        iterations, stopped = ctypes.c_int64(0), ctypes.c_int32(0)
        numbers = np.zeros(3)
        base = numbers.ctypes.data
        _lib.check(self._gap_fn("gap_state")(self._h, ctypes.addressof(iterations), ctypes.addressof(stopped), base, base + 8, base + 16))
        return int(iterations.value), bool(stopped.value), float(numbers[0]), float(numbers[1]), float(numbers[2])


def gap_info(state):
    """``info`` of a certified run from the state's record: the keys of ``chambolle_pock_ppd_certified``."""
    iterations, stopped, primal, bound, violation = state.gap_state()
    return dict(iterations=iterations, stopped=stopped, primal=primal, lower_bound=bound, violation=violation)
