"""What the batched forms (B LPs over one matrix) and the list forms (LPs with matrices of their own) of the solvers share on the
host: shape checks and the small array helpers of their assembled systems.  Private; numpy only, and nothing here loads the
library -- every refusal below comes before a caller touches the GPU."""
import numpy as np

from . import _lib


def shared_or_batched(name, v, batch, size):
    """``v`` as a contiguous float64 array of shape ``(size,)`` (shared by the instances) or ``(batch, size)`` (one row per
    instance); returns ``(array, is_batched)``."""
    v = np.asarray(v, dtype=np.float64)
    if v.shape == (size,):
        return _lib.f64(v), False
    if v.shape == (batch, size):
        return _lib.f64(v), True
    raise ValueError(f"{name} has shape {v.shape}: expected ({size},) shared by the instances, or (B, {size}) with B = {batch}")


def check_costs(costs, n):
    """``costs`` as a float64 array of shape ``(B, n)`` with ``B >= 1``; returns ``(costs, B)``."""
    costs = np.asarray(costs, dtype=np.float64)
    if costs.ndim != 2 or costs.shape[1] != n:
        raise ValueError(f"costs has shape {costs.shape}: expected (B, {n}), one row per instance")
    if costs.shape[0] < 1:
        raise ValueError("an empty batch: costs needs at least one row (B >= 1)")
    return costs, costs.shape[0]


def check_targets(targets, batch):
    """The cut-offs of a per-instance bound test as a contiguous float64 array of shape ``(batch,)``: ``targets`` is a real scalar
    (the same cut-off for every instance) or has shape ``(batch,)``; ``+inf`` means that an instance has none, a NaN or ``-inf`` is
    refused.  None stays None (no bound test)."""
    if targets is None:
        return None
    try:
        t = np.asarray(targets)
        if t.dtype == bool or t.dtype.kind not in "iuf":
            raise TypeError
        t = t.astype(np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"targets must be a real number or an array of {batch} real numbers, not {targets!r}") from None
    if t.shape not in ((), (batch,)):
        raise ValueError(f"targets has shape {t.shape}: expected a scalar or ({batch},), one cut-off per instance")
    if np.any(np.isnan(t)) or np.any(t == -np.inf):
        raise ValueError("targets holds a NaN or -inf: a cut-off is a number or +inf (no cut-off for that instance)")
    return _lib.f64(np.broadcast_to(t, (batch,)).copy())


def check_rhs(name, v, batch, rows, finite=False):
    """A right-hand side of ``set_rhs``: ``shared_or_batched(name, v, batch, rows)`` without a NaN and, with ``finite``, without an
    infinite entry in a batched one (the ``ValueError`` names the first such instance)."""
    v, batched = shared_or_batched(name, v, batch, rows)
    if np.any(np.isnan(v)):
        raise ValueError(f"{name} has a NaN")
    if finite and batched and not np.all(np.isfinite(v)):
        k = int(np.nonzero(~np.all(np.isfinite(v), axis=1))[0][0])
        raise ValueError(f"instance {k} has an entry of {name} that is not finite")
    return v, batched


def check_rhs_order(b_lower, b_upper, batch):
    """``b_lower <= b_upper`` row by row, each of shape ``(rows,)`` or ``(batch, rows)`` (either may be None): the ``ValueError``
    names the first instance with a crossed row."""
    if b_lower is None or b_upper is None:
        return
    rows = np.shape(b_lower)[-1]
    crossed = np.broadcast_to(b_lower, (batch, rows)) > np.broadcast_to(b_upper, (batch, rows))
    if np.any(crossed):
        k = int(np.nonzero(np.any(crossed, axis=1))[0][0])
        raise ValueError(f"instance {k} has b_lower > b_upper on row {int(np.nonzero(crossed[k])[0][0])}")


def require_one_sided(b_lower, prefix=""):
    """Dual gradient ascent takes ``a x <= b_upper`` only (the reference's assert, DualGradientAscent.py:82)."""
    if b_lower is not None and np.size(b_lower) > 0 and np.max(b_lower) != -np.inf:
        raise ValueError(f"{prefix}dual_gradient_ascent needs one-sided inequalities: b_lower must be None or all -inf")


def box_vertex(c, lb, ub):
    """The solution of an LP without constraint rows (reference ChambollePockPPD.py:147-151): ``lb`` where the cost is positive,
    ``ub`` where it is negative, 0 elsewhere.  ``lb`` and ``ub`` broadcast against ``c``."""
    lb, ub = np.broadcast_to(lb, c.shape), np.broadcast_to(ub, c.shape)
    x = np.zeros(c.shape)
    x[c > 0] = lb[c > 0]
    x[c < 0] = ub[c < 0]
    return x


def split_by(flat, sizes):
    """``flat`` cut into consecutive copies of the given sizes."""
    return [v.copy() for v in np.split(flat, np.cumsum(sizes)[:-1])]


def first_offsets(sizes):
    """Where each of consecutive pieces of the given sizes begins."""
    return np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.int64)


def concat(parts, dtype):
    """The parts (possibly none) one after another, contiguous, as ``dtype``."""
    return np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(0), dtype=dtype)
