"""numpy restatement of dual gradient ascent with the exact dual line search (reference DualGradientAscent.py:36-245).

``order`` picks how the line search sorts and sums:

``"reference"``  the reference's own operations: sparse row times CSR, ``np.argsort``, ``np.cumsum``, sparse dot;
``"blocked"``    a stable sort by (alpha, column), both running sums formed in blocks of ``block`` elements (in order inside a
                 block, the block sums in order, an element = its block's offset + its sum inside the block) and a pairwise g.b;
``"device"``     the sums exactly as csrc/slp_dga.hip forms them: 4 elements per thread, Hillis-Steele over 64 lanes, 4 waves
                 per 1024-element tile, the tile sums scanned the same way; g.b over tiles of 256 rows.

The step is a discontinuous function of the sums, so the three agree bit for bit only as long as no rounding difference
lands on a decision: tests/golden/make_dga_golden.py records, per case, how far that holds (``<case>_horizon``).
"""
import numpy as np
import scipy.sparse


def _tree(v):
    """Sum of a power-of-two number of terms by adding the upper half onto the lower half, repeatedly."""
    v = np.array(v, dtype=np.float64)
    while v.size > 1:
        h = v.size // 2
        v = v[:h] + v[h:]
    return v[0]


def _pairwise_dot(g, b):
    terms = np.where(g != 0, g * np.where(g != 0, b, 0.0), 0.0)
    size = 1
    while size < terms.size:
        size *= 2
    return _tree(np.concatenate((terms, np.zeros(size - terms.size))))


def _device_dot(g, b, parts=256, tile=256):
    """k_dga_grad / k_dga_begin: tiles of 256 rows (64-lane trees, the 4 waves in order), a workgroup's tiles in order, then
    the 256 workgroups as one more tile."""
    terms = np.where(g != 0, g * np.where(g != 0, b, 0.0), 0.0)
    tiles = -(-terms.size // tile)
    terms = np.concatenate((terms, np.zeros(tiles * tile - terms.size))).reshape(tiles, 4, 64)
    w = terms.copy()
    for off in (32, 16, 8, 4, 2, 1):
        w = w[:, :, :off] + w[:, :, off:2 * off]
    w = w[:, :, 0]
    tile_sums = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    per = -(-tiles // parts)
    part = np.zeros(parts)
    for p in range(parts):
        acc = 0.0
        for s in tile_sums[p * per:(p + 1) * per]:
            acc += s
        part[p] = acc
    w = part.reshape(4, 64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w[:, :off] + w[:, off:2 * off]
    w = w[:, 0]
    return ((w[0] + w[1]) + w[2]) + w[3]


def _blocked_cumsum(v, block):
    n = v.size
    pad = -(-n // block) * block
    w = np.concatenate((v, np.zeros(pad - n))).reshape(-1, block)
    inside = np.cumsum(w, axis=1)
    offsets = np.concatenate(([0.0], np.cumsum(inside[:, -1])[:-1]))
    return (offsets[:, None] + inside).reshape(-1)[:n]


def _group_excl(tot):
    """group_excl_scan over rows of 256 thread totals: (exclusive prefix per thread, total per row)."""
    t = tot.reshape(-1, 4, 64)
    inc = t.copy()
    for off in (1, 2, 4, 8, 16, 32):
        nxt = inc.copy()
        nxt[:, :, off:] = inc[:, :, :-off] + inc[:, :, off:]
        inc = nxt
    ex = np.concatenate((np.zeros(inc.shape[:2] + (1,)), inc[:, :, :-1]), axis=2)
    wsum = inc[:, :, -1]
    woff = np.zeros_like(wsum)
    for i in range(1, 4):
        woff[:, i] = woff[:, i - 1] + wsum[:, i - 1]
    total = ((0.0 + wsum[:, 0]) + wsum[:, 1]) + wsum[:, 2] + wsum[:, 3]
    return (woff[:, :, None] + ex).reshape(-1, 256), total


def _device_cumsum(v):
    nb = v.size
    tiles = -(-nb // 1024)
    w = np.concatenate((v, np.zeros(tiles * 1024 - nb))).reshape(tiles, 256, 4)
    tot = ((w[:, :, 0] + w[:, :, 1]) + w[:, :, 2]) + w[:, :, 3]
    ex, tile_tot = _group_excl(tot)
    # scan_tile_sums: thread i owns `per` consecutive tiles
    per = -(-tiles // 256)
    padded = np.concatenate((tile_tot, np.zeros(256 * per - tiles))).reshape(256, per)
    s = np.zeros(256)
    for i in range(per):
        s = s + padded[:, i]
    tex, _ = _group_excl(s.reshape(1, 256))
    off = np.zeros((256, per))
    run = tex[0].copy()
    for i in range(per):
        off[:, i] = run
        run = run + padded[:, i]
    off = off.reshape(-1)[:tiles]
    run = off[:, None] + ex
    out = np.zeros_like(w)
    for e in range(4):
        run = run + w[:, :, e]
        out[:, :, e] = run
    return out.reshape(-1)[:nb]


class Ties:
    """The uniform draws of the tie rule: one private MT19937 stream, counted."""

    def __init__(self, seed=0):
        self.rs = np.random.RandomState(seed)
        self.count = 0
        self.last = np.nan

    def draw(self):
        self.count += 1
        self.last = self.rs.rand()
        return self.last


def exact_dual_line_search(direction, a, b, c_bar, upper_bounds, lower_bounds, ties, order="reference", block=64):
    """The step along ``direction`` (dense, m values) that maximises the dual; ``a`` CSR of the m rows."""
    if order == "reference":
        row = scipy.sparse.csr_matrix(direction)
        d_a = row * a
        idx, d = d_a.indices, d_a.data
        gb = row.dot(b)
        alphas = -c_bar[idx] / d
        perm = np.argsort(alphas)
    else:
        full = direction * a   # per column: the rows in order, zeros of the direction add +-0.0
        idx = np.nonzero(full)[0]
        d = full[idx]
        gb = _pairwise_dot(direction, b) if order == "blocked" else _device_dot(direction, b)
        alphas = -c_bar[idx] / d
        perm = np.argsort(alphas + 0.0, kind="stable")
    if alphas.size == 0:
        raise ValueError("exact_dual_line_search: the direction meets no column (empty breakpoint set)")
    du, dl = d * upper_bounds[idx], d * lower_bounds[idx]
    low, high = np.minimum(du[perm], dl[perm]), np.maximum(du[perm], dl[perm])
    if order == "reference":
        back, fwd = np.cumsum(high[::-1])[::-1], np.cumsum(low)
    elif order == "blocked":
        back, fwd = _blocked_cumsum(high[::-1], block)[::-1], _blocked_cumsum(low, block)
    else:
        back, fwd = _device_cumsum(high[::-1])[::-1], _device_cumsum(low)
    deriv = -gb * np.ones(alphas.size + 1)
    deriv[:-1] += back
    deriv[1:] += fwd
    k = np.searchsorted(-deriv, 0)
    if k > alphas.size:
        raise ValueError("exact_dual_line_search: the derivative never changes sign")
    if deriv[k] == 0 and k < perm.size:
        r = ties.draw()
        return r * alphas[perm[k]] + (1 - r) * alphas[perm[k - 1]]
    return alphas[perm[k - 1]]


def dual_argmin(c, a_eq, a_ineq, lb, ub, y_eq, y_ineq):
    c_bar = c.copy()
    if a_eq is not None:
        c_bar += y_eq * a_eq
    if a_ineq is not None:
        c_bar += y_ineq * a_ineq
    x = np.zeros(c.size)
    x[c_bar > 0] = lb[c_bar > 0]
    x[c_bar < 0] = ub[c_bar < 0]
    x[c_bar == 0] = 0.5 * (lb + ub)[c_bar == 0]
    return c_bar, x


def dual_energy(c, a_eq, b_eq, a_ineq, b_upper, lb, ub, y_eq, y_ineq):
    c_bar, _ = dual_argmin(c, a_eq, a_ineq, lb, ub, y_eq, y_ineq)
    with np.errstate(invalid="ignore"):
        e = np.sum(np.minimum(c_bar * ub, c_bar * lb)[c_bar != 0])
    if a_eq is not None:
        e -= y_eq.dot(b_eq)
    if a_ineq is not None:
        e -= y_ineq.dot(b_upper)
    return e


def _device_parts(terms, parts=256, lanes=256):
    """The ``parts`` partial results of dga_energy_x_body / dga_energy_y_body over one term per column / row: term ``j`` is lane
    ``j % lanes`` of workgroup ``j // lanes`` (the grid-stride loop, at most one term per lane: ``acc = 0.0 + term``), a workgroup's
    sum is block_reduce -- the 64-lane tree per wave, the four waves added in order.  Only the workgroups that hold a term are
    formed: the others' lanes hold +0.0 and so do their sums, exactly."""
    assert terms.ndim == 1 and terms.size <= parts * lanes and lanes == 4 * 64
    used = -(-terms.size // lanes)
    w = 0.0 + np.concatenate((terms, np.zeros(used * lanes - terms.size))).reshape(used, 4, 64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w[:, :, :off] + w[:, :, off:2 * off]
    w = w[:, :, 0]
    return np.concatenate((((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3], np.zeros(parts - used)))


def device_energy(c, a_eq, b_eq, a_ineq, b_upper, lb, ub, y_eq, y_ineq):
    """``dual_energy`` in the device's order of sums (k_dgab_energy_x / k_dgab_energy_y + dga_bound_finish in
    csrc/slp_dga_shared.h, the same text as the bound of the batch's stopping test): the column terms ``min(c_bar ub, c_bar lb)``
    where ``c_bar != 0``, else 0; the row terms ``y_i b_i`` where ``y_i != 0``, else 0, over all rows, equalities first; each vector
    dealt to 256 workgroups of 256 lanes (``_device_parts``); the 256 partial results of each pass summed in order from 0.0, and
    ``e - yb``.  ``n, m <= 65536``: a lane holds at most one term, so neither the loop's order nor an FMA contraction can matter."""
    c_bar, _ = dual_argmin(c, a_eq, a_ineq, lb, ub, y_eq, y_ineq)
    y = np.asarray(y_eq, dtype=np.float64) if a_eq is not None else np.zeros(0)
    b = np.asarray(b_eq, dtype=np.float64) if a_eq is not None else np.zeros(0)
    if a_ineq is not None:
        y, b = np.concatenate((y, y_ineq)), np.concatenate((b, b_upper))
    assert c_bar.size <= 65536 and y.size <= 65536 and y.size == b.size
    with np.errstate(invalid="ignore"):
        u, low = c_bar * ub, c_bar * lb
        cols = np.where(c_bar != 0, np.where(u < low, u, low), 0.0)   # (u < l) ? u : l
        rows = np.where(y != 0, y * b, 0.0)
        e = yb = 0.0
        for pe, py in zip(_device_parts(cols), _device_parts(rows)):
            e += pe
            yb += py
        return float(e - yb)


def dga_cpu(c, a_eq, b_eq, a_ineq, b_upper, lb, ub, nb_max_iter, order="reference", block=64, keep=None, y_eq=None, y_ineq=None,
            on_search=None):
    """Runs ``nb_max_iter`` iterations; returns ``{it: (x, y_eq, y_ineq, draws)}`` for ``it`` in ``keep`` (default: the last one):
    x of the top of iteration ``it``, the multipliers after it and the tie draws taken so far -- what the reference returns
    after ``it + 1`` iterations.  Key -1: the start (a dual-infeasible start returns only that).  ``a_eq``: CSR, may have no
    rows; ``a_ineq``: CSR or None.  ``on_search(it, kind, direction, c_bar, step, draw)`` sees every line search (``draw``: the
    uniform draw its tie took, else NaN)."""
    ties = Ties(0)
    y_eq = -ties.rs.rand(a_eq.shape[0]) if y_eq is None else y_eq.copy()
    if y_ineq is None:
        if a_ineq is not None:
            y_ineq = np.abs(ties.rs.rand(a_ineq.shape[0]))
    else:
        y_ineq = y_ineq.copy()
    keep = {nb_max_iter - 1} if keep is None else set(keep)
    _, x = dual_argmin(c, a_eq, a_ineq, lb, ub, y_eq, y_ineq)
    out = {-1: (x, y_eq.copy(), None if y_ineq is None else y_ineq.copy(), 0)}
    if dual_energy(c, a_eq, b_eq, a_ineq, b_upper, lb, ub, y_eq, y_ineq) == -np.inf:
        return out
    for it in range(nb_max_iter):
        c_bar, x = dual_argmin(c, a_eq, a_ineq, lb, ub, y_eq, y_ineq)
        if a_ineq is not None:
            g = a_ineq * x - b_upper
            held = y_ineq <= 0
            g[held] = np.maximum(g[held], 0)
            if np.any(g < 0):
                before = ties.count
                t = exact_dual_line_search(g, a_ineq, b_upper, c_bar, ub, lb, ties, order, block)
                if on_search is not None:
                    on_search(it, "ineq", g, c_bar, t, ties.last if ties.count > before else np.nan)
                assert t >= 0
                t = min(t, np.min(y_ineq[g < 0] / -g[g < 0]))
                y_ineq = np.maximum(y_ineq + t * g, 0)
        if a_eq.shape[0] > 0:
            g = a_eq * x - b_eq
            if np.any(g):
                before = ties.count
                t = exact_dual_line_search(g, a_eq, b_eq, c_bar, ub, lb, ties, order, block)
                if on_search is not None:
                    on_search(it, "eq", g, c_bar, t, ties.last if ties.count > before else np.nan)
                assert t >= 0
                y_eq = y_eq + t * g
        if it in keep:
            out[it] = (x, y_eq.copy(), None if y_ineq is None else y_ineq.copy(), ties.count)
    return out
