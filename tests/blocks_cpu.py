"""numpy / scipy reference of the matrix-free projection solvers of csrc/slp_blocks.hip (``DeviceBlocks``, ``DeviceADMM2``): no GPU,
no library call.

The LP is held as the device holds it: one CSR matrix ``a`` (m x n) whose first ``m_eq`` rows are equalities ``a_i x = b_upper_i`` and
whose other rows are ``b_lower_i <= a_i x <= b_upper_i`` with an implicit slack each (standard form ``[A_eq 0; A_in -I]``,
``b = [b_eq; 0]``, tools.py:88-127).  Both solvers project a point ``(v, vs)`` onto ``{A_eq x = b_eq, A_in x - s = 0}`` once per
iteration; the device does it by conjugate gradients on

    dual form     (A A^T + [0; I]) nu = A v - [0; vs] - b ,   x = v - A^T nu ,  s = vs + nu_in
    primal form   (I + A^T A) x      = v + A^T vs ,           s = A x                         (m_eq = 0 only)

``ExactProjector`` / ``project_exact`` solve the same system densely (Cholesky of the system assembled in float64, two rounds of
iterative refinement with the residual in ``np.longdouble``), so the side the system lives on has to stay small (``DENSE_LIMIT``);
the other side may have any length.  It solves the system in the form the device would take (``device_primal``), so that the norm
of the right-hand side and the smallest eigenvalue it reports are those of the device's system: the test turns the device's
residual bar into a bound on the error of ``x`` with them (``projection_bound``).

``admm2_exact`` and ``blocks_exact`` restate the two outer loops (ADMM.py:320-474 as tests/test_admm2_host.py::admm2_matrix_free
states it, with a starting point; ADMMBlocks.py:264-307 with the whole matrix as one block) around a projection callable
``project(v, vs) -> (x, s)``: the exact one by default, or ``CgProjector`` -- the conjugate gradients of ``admm2_matrix_free``, warm
started -- where the dense side would be too large."""
import collections

import numpy as np
import scipy.linalg
import scipy.sparse

DENSE_LIMIT = 400
GAMMA, ALPHA = 0.7, 1.95

Projection = collections.namedtuple("Projection", "x s nu rhs_norm sigma_max lambda_min lambda_max")


def device_primal(m, n, m_eq, forced=None):
    """The form ``rb_primal_form`` (csrc/slp_blocks.hip) takes: ``forced`` is the value of SLP_BLOCKS_PRIMAL or None."""
    return m_eq == 0 and m > 0 and (str(forced)[0] == "1" if forced is not None else m >= n)


class _Products:
    """``A x`` and ``A^T y`` in np.longdouble: per row the products in storage order, summed by ``np.add.reduceat`` over the rows that
    have entries."""

    def __init__(self, a):
        self.a = scipy.sparse.csr_matrix(a)
        self.t = scipy.sparse.csr_matrix(self.a.T)
        self.parts = []
        for mat in (self.a, self.t):
            ptr = mat.indptr.astype(np.int64)
            full = np.nonzero(np.diff(ptr))[0]
            self.parts.append((mat.shape[0], full, ptr[full], mat.indices.astype(np.int64), mat.data.astype(np.longdouble)))

    def _apply(self, which, x):
        rows, full, starts, idx, val = self.parts[which]
        y = np.zeros(rows, dtype=np.longdouble)
        if full.size:
            y[full] = np.add.reduceat(val * np.asarray(x, dtype=np.longdouble)[idx], starts)
        return y

    def mv(self, x):
        return self._apply(0, x)

    def rmv(self, y):
        return self._apply(1, y)


class ExactProjector:
    """The projection onto ``{A_eq x = b_eq, A_in x - s = 0}`` by a dense solve; ``b`` has length m (``[b_eq; 0]``).  ``primal``: the
    form of the system (default: the one the device takes unforced)."""

    def __init__(self, a, m_eq, b, primal=None):
        self.a = scipy.sparse.csr_matrix(a)
        self.m, self.n = self.a.shape
        self.m_eq = int(m_eq)
        self.b = np.asarray(b, dtype=np.float64)
        assert self.b.size == self.m and 0 <= self.m_eq <= self.m
        self.primal = device_primal(self.m, self.n, self.m_eq) if primal is None else bool(primal)
        assert not self.primal or (self.m_eq == 0 and not self.b.any())
        self.side = self.n if self.primal else self.m
        assert 0 < self.side <= DENSE_LIMIT, f"dense side {self.side} above {DENSE_LIMIT}"
        self.ld = _Products(self.a)
        self.ineq = (np.arange(self.m) >= self.m_eq).astype(np.float64)
        if self.primal:
            self.system = np.eye(self.n) + (self.a.T @ self.a).toarray()
        else:
            self.system = (self.a @ self.a.T).toarray() + np.diag(self.ineq)
        ev = scipy.linalg.eigvalsh(self.system)
        self.lambda_min, self.lambda_max = float(ev[0]), float(ev[-1])
        gram = (self.a @ self.a.T if self.m <= self.n else self.a.T @ self.a).toarray()
        self.sigma_max = float(np.sqrt(max(scipy.linalg.eigvalsh(gram)[-1], 0.0)))
        self.chol = None
        if self.lambda_min > 0.0:
            try:
                self.chol = scipy.linalg.cho_factor(self.system)
            except np.linalg.LinAlgError:   # positive only by the rounding of the eigenvalues
                pass

    @property
    def condition(self):
        return self.lambda_max / self.lambda_min if self.chol is not None else np.inf

    def _apply_ld(self, y):
        if self.primal:
            return y + self.ld.rmv(self.ld.mv(y))
        return self.ld.mv(self.ld.rmv(y)) + self.ineq.astype(np.longdouble) * y

    def project(self, v, vs):
        """``vs`` over the inequality rows (length m - m_eq)."""
        assert self.chol is not None, "singular projection system"
        v, vs = np.asarray(v, dtype=np.longdouble), np.asarray(vs, dtype=np.longdouble)
        assert v.size == self.n and vs.size == self.m - self.m_eq
        vs_all = np.concatenate((np.zeros(self.m_eq, dtype=np.longdouble), vs))
        rhs = v + self.ld.rmv(vs_all) if self.primal else self.ld.mv(v) - vs_all - self.b.astype(np.longdouble)
        sol = scipy.linalg.cho_solve(self.chol, rhs.astype(np.float64)).astype(np.longdouble)
        for _ in range(2):
            sol = sol + scipy.linalg.cho_solve(self.chol, (rhs - self._apply_ld(sol)).astype(np.float64))
        if self.primal:   # (m_eq = 0: every row has a slack)
            x = sol
            s = self.ld.mv(x)
            nu = s - vs_all
        else:
            nu = sol
            x = v - self.ld.rmv(nu)
            s = (vs_all + nu)[self.m_eq:]
        return Projection(x.astype(np.float64), s.astype(np.float64), nu.astype(np.float64), float(np.sqrt(np.sum(rhs * rhs))),
                          self.sigma_max, self.lambda_min, self.lambda_max)

    def __call__(self, v, vs):
        p = self.project(v, vs)
        return p.x, p.s


def project_exact(a, m_eq, b, v, vs, primal=None):
    """Euclidean projection of ``(v, vs)`` onto ``{A_eq x = b_eq, A_in x - s = 0}``: a ``Projection`` of ``x``, ``s`` (over the
    inequality rows), the multiplier ``nu`` (``x = v - A^T nu``), and of the system in the device's form the norm of its right-hand
    side, its extreme eigenvalues, and ``sigma_max(A)``."""
    return ExactProjector(a, m_eq, b, primal).project(v, vs)


def projection_bound(p, a, tol, alpha=ALPHA):
    """Bound on ``|x_dev - x_ref|_2`` after ONE iteration from zero multipliers, from the reference's own quantities: the device's
    projection meets ``|rhs - S sol| <= 2 tol |rhs|`` (the bar the suite asserts through ``projection_residual``), which is an error
    of at most ``2 tol |rhs| / lambda_min`` in ``sol`` and ``sigma_max`` times that in ``x = v - A^T nu``; a factor 4 for the
    reference's own rounding of ``rhs`` and the elementwise steps; plus the rounding of the closing product ``A^T nu`` summed in any
    order (``oracle.row_error_bound``).  The iterate is ``alpha x + (1 - alpha) xp``: times ``alpha``; a clamp does not increase it."""
    from oracle import oracle

    at = scipy.sparse.csr_matrix(scipy.sparse.csr_matrix(a).T)
    closing = float(np.linalg.norm(oracle.row_error_bound(at, p.nu)))
    return alpha * (4.0 * (2.0 * tol * p.rhs_norm) * p.sigma_max / p.lambda_min + closing)


class CgProjector:
    """The projection of tests/test_admm2_host.py::admm2_matrix_free: conjugate gradients on the dual form from the previous
    multiplier, stopping test ``|r|^2 <= tol^2 |rhs|^2`` before every step.  ``steps`` counts the steps of all calls."""

    def __init__(self, a, m_eq, b, tol=1e-13, max_steps=500):
        self.a = scipy.sparse.csr_matrix(a)
        self.at = scipy.sparse.csr_matrix(self.a.T)
        self.m_eq, self.b, self.tol, self.max_steps = int(m_eq), np.asarray(b, dtype=np.float64), tol, max_steps
        self.ineq = (np.arange(self.a.shape[0]) >= self.m_eq).astype(np.float64)
        self.nu = np.zeros(self.a.shape[0])
        self.steps = 0

    def apply(self, p):
        return self.a @ (self.at @ p) + self.ineq * p

    def __call__(self, v, vs):
        rhs = self.a @ v - np.concatenate((np.zeros(self.m_eq), vs)) - self.b
        nu = self.nu
        r = rhs - self.apply(nu)
        d, rs, bar = r.copy(), r @ r, self.tol * self.tol * (rhs @ rhs)
        for _ in range(self.max_steps):
            if not rs > bar:
                break
            q = self.apply(d)
            step = rs / (d @ q)
            nu, r = nu + step * d, r - step * q
            rs, rs_old = r @ r, rs
            d = r + (rs / rs_old) * d
            self.steps += 1
        self.nu = nu
        return v - self.at @ nu, vs + nu[self.m_eq:]


def _rows(a, m_eq, b_lower, b_upper):
    a = scipy.sparse.csr_matrix(a)
    m = a.shape[0]
    b_upper = np.asarray(b_upper, dtype=np.float64)
    assert b_upper.size == m
    b = np.concatenate((b_upper[:m_eq], np.zeros(m - m_eq)))
    slo = np.full(m - m_eq, -np.inf) if b_lower is None else np.asarray(b_lower, dtype=np.float64)[m_eq:]
    return a, b, slo, b_upper[m_eq:]


def admm2_exact(a, m_eq, b_lower, b_upper, c, lb, ub, nb_iter, x0=None, project=None, primal=None, gamma=GAMMA, alpha=ALPHA):
    """``nb_iter`` iterations of lp_admm2 (ADMM.py:320-474) from ``x0`` (zeros when None; the slacks start from ``A x0``, clamped,
    tools.py:123-124): ``(x after every iteration, energy of every iteration)`` -- the energy of ADMM.py:396-402, lambda before its
    update.  ``project``: the projection callable (default: the exact one in the form ``primal``)."""
    a, b, slo, shi = _rows(a, m_eq, b_lower, b_upper)
    c, lb, ub = (np.asarray(t, dtype=np.float64) for t in (c, lb, ub))
    if project is None:
        project = ExactProjector(a, m_eq, b, primal)
    x = np.zeros(c.size) if x0 is None else np.asarray(x0, dtype=np.float64)
    xp, xps = np.clip(x, lb, ub), np.clip((a @ x)[m_eq:], slo, shi)
    lam, lams = np.zeros(c.size), np.zeros(xps.size)
    xs_out, energies = [], []
    for _ in range(nb_iter):
        v, vs = (-c + gamma * xp - lam) / gamma, xps - lams / gamma
        xh, sh = project(v, vs)
        x = alpha * xh + (1 - alpha) * xp
        xs = alpha * sh + (1 - alpha) * xps
        xp, xps = np.clip(x + lam / gamma, lb, ub), np.clip(xs + lams / gamma, slo, shi)
        energies.append(float(c @ x + 0.5 * gamma * (np.sum((x - xp) ** 2) + np.sum((xs - xps) ** 2)) + lam @ (x - xp) + lams @ (xs - xps)))
        xs_out.append(x)
        lam, lams = lam + gamma * (x - xp), lams + gamma * (xs - xps)
    return xs_out, energies


def blocks_exact(a, m_eq, b_lower, b_upper, c, lb, ub, nb_iter, project=None, primal=None, gamma=GAMMA, alpha=ALPHA):
    """``nb_iter`` iterations of lp_admm_block_decomposition (ADMMBlocks.py:264-307) from x0 = 0 with all rows as ONE block, as
    ``DeviceBlocks`` runs it on one rank: ``(xp after every iteration, energy after every iteration)`` (:246-253, the multipliers
    after their update).  A column without entries has no copy in the block: the consensus keeps its ``xp`` in the sum (:290-299),
    so it moves by ``-c / gamma`` per iteration until it meets a bound, and it has no multiplier and no energy term."""
    a, b, slo, shi = _rows(a, m_eq, b_lower, b_upper)
    c, lb, ub = (np.asarray(t, dtype=np.float64) for t in (c, lb, ub))
    if project is None:
        project = ExactProjector(a, m_eq, b, primal)
    used = np.zeros(c.size, dtype=bool)
    used[a.indices] = True
    xp, xps = np.clip(np.zeros(c.size), lb, ub), np.clip(np.zeros(slo.size), slo, shi)
    lam, lams = np.zeros(c.size), np.zeros(xps.size)
    xp_out, energies = [], []
    for _ in range(nb_iter):
        v, vs = xp - lam / gamma, xps - lams / gamma
        xh, sh = project(v, vs)
        x = alpha * xh + (1 - alpha) * xp
        xs = alpha * sh + (1 - alpha) * xps
        xp = np.clip(np.where(used, x + lam / gamma, xp) - c / gamma, lb, ub)   # one copy at most: no division
        xps = np.clip(xs + lams / gamma, slo, shi)
        lam = np.where(used, lam + gamma * (x - xp), lam)
        lams = lams + gamma * (xs - xps)
        d, ds = np.where(used, x - xp, 0.0), xs - xps
        energies.append(float(c @ xp + 0.5 * gamma * (np.sum(d ** 2) + np.sum(ds ** 2)) + lam @ d + lams @ ds))
        xp_out.append(xp)
    return xp_out, energies
