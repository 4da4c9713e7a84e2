"""Device-side set-up of a host scipy LP for the reference's entry points (``lp_admm(xstep="cg")``, ``chambolle_pock_ppd``,
``SparseLP.solve``) with ``setup="device"``.

The reference prepares these solvers on the host: ``precondition_constraints`` three times and
``convert_to_standard_form_with_bounds`` for the conjugate-gradient ADMM (ADMM.py:73-101), the one-sided stacking
``[A_eq; K_ineq]`` for Chambolle-Pock (ChambollePockPPD.py:74-88,145-233) and, in ``SparseLP.solve``, ``copy.deepcopy`` and
``remove_fixed_variables`` (SparseLP.py:1244-1248).  Here the two constraint blocks are uploaded as the caller holds them and
everything else runs on the device (``slp_matrix_create_stacked``, ``slp_admm_cg_create_lp``, ``DeviceCP``).

When the stacked matrix and its product copies would not fit the device, it is built from row chunks instead
(``ChunkedDeviceMatrix``: the equality rows' chunks first, then the inequality rows', cut at ``m_eq``).  ``SLP_SETUP_CHUNK_ENTRIES``
in the environment forces chunks of about that many stored entries (tests, or a device shared with other work).
"""
import os

import numpy as np

from . import _lib
from .device import ChunkedDeviceMatrix, DeviceMatrix
from .tools import CsrArrays

DICT_MAX = 2048             # most distinct stored values of a value-dictionary copy (csrc/slp_strip.hip: kDictMax)
BYTES_PER_ENTRY = 48        # CSR in both orientations (12 B per entry each) and fp64 product copies of both (12 B each)
DEFAULT_CHUNK_ENTRIES = 2_500_000_000
MULTI_GPU = "partition the rows over several GPUs instead (parallel.init_comm_from_env: every rank holds a block of the rows)"


def choose(setup, nnz):
    """``"auto"`` -> ``"device"`` at ``SparseLP.DEVICE_SETUP_ENTRIES`` stored entries or more, else ``"host"``."""
    if setup not in ("auto", "host", "device"):
        raise ValueError(f"setup must be 'auto', 'host' or 'device', not {setup!r}")
    if setup == "auto":
        from . import SparseLP

        return "device" if nnz >= SparseLP.DEVICE_SETUP_ENTRIES else "host"
    return setup


def nnz_of(*blocks):
    return sum(int(b.indptr[-1]) for b in blocks if b is not None and b.shape[0] > 0)


def rows_of(a, r0, r1):
    """Rows ``r0 .. r1`` of a host CSR block as ``CsrArrays`` (views of the indices and values, row offsets rebased); ``None``
    when the range is empty."""
    if a is None or r1 <= r0:
        return None
    k0, k1 = int(a.indptr[r0]), int(a.indptr[r1])
    return CsrArrays(np.asarray(a.indptr[r0:r1 + 1], dtype=np.int64) - k0, a.indices[k0:k1], a.data[k0:k1], (r1 - r0, a.shape[1]))


def local_blocks(a_eq, a_ineq):
    """This rank's rows of the stacked ``[A_eq; A_ineq]`` under the active communicator (``parallel.local_rows``: equal stored
    entries per rank), as ``((e0, e1), (i0, i1))`` row ranges of the two blocks; the whole blocks without a communicator."""
    from .parallel import comm_world, local_rows

    m_eq = 0 if a_eq is None else a_eq.shape[0]
    m_in = 0 if a_ineq is None else a_ineq.shape[0]
    if comm_world()[0] <= 1:
        return (0, m_eq), (0, m_in)
    parts = [np.zeros(1, dtype=np.int64)]
    if a_eq is not None:
        parts.append(np.asarray(a_eq.indptr[1:], dtype=np.int64))
    if a_ineq is not None:
        parts.append(np.asarray(a_ineq.indptr[1:], dtype=np.int64) + (int(a_eq.indptr[-1]) if a_eq is not None else 0))
    r0, r1, _ = local_rows(np.concatenate(parts), m_eq)
    return (min(r0, m_eq), min(r1, m_eq)), (max(r0, m_eq) - m_eq, max(r1, m_eq) - m_eq)


def chunk_entries(nnz, nrow, ncol):
    """Stored entries per chunk when the LP must be built from chunks, else ``None``: ``SLP_SETUP_CHUNK_ENTRIES`` when set,
    otherwise chunks of ``DEFAULT_CHUNK_ENTRIES`` once ``BYTES_PER_ENTRY`` per entry plus the row and column pointers exceed
    nine tenths of the device's free memory (``slp_device_memory``)."""
    env = os.environ.get("SLP_SETUP_CHUNK_ENTRIES")
    if env:
        return int(float(env))
    free, total = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64)
    _lib.check(_lib.lib().slp_device_memory(_lib.ptr(free), _lib.ptr(total)))
    need = BYTES_PER_ENTRY * nnz + 8 * (nrow + ncol + 2)
    return DEFAULT_CHUNK_ENTRIES if need > 0.9 * float(free[0]) else None


def few_distinct_values(blocks, limit=DICT_MAX):
    """Whether the stored values of all ``blocks`` together take at most ``limit`` distinct values (stops early)."""
    seen = np.zeros(0)
    for blk in blocks:
        if blk is None:
            continue
        for k0 in range(0, blk.data.size, 1 << 26):
            seen = np.union1d(seen, blk.data[k0:k0 + (1 << 26)])
            if seen.size > limit:
                return False
    return True


def upload(eq, ineq, ncol, entries=None, keep=None, shift=None):
    """The device matrix ``[eq; ineq]`` (``CsrArrays`` row blocks, either may be ``None``): one stacked CSR, or with ``entries``
    a ``ChunkedDeviceMatrix`` of chunks of about that many stored entries, the equality rows' chunks first (cut at ``m_eq``, which
    must then be even).  ``keep`` (boolean mask over the columns): every chunk's columns are compacted on the device before it is
    appended, with ``A @ shift`` returned beside the matrix (``remove_fixed_variables`` chunk by chunk; chunked form only)."""
    if entries is None:
        assert keep is None
        return DeviceMatrix.from_blocks(eq, ineq, ncol), None
    m_eq = 0 if eq is None else eq.shape[0]
    m = m_eq + (0 if ineq is None else ineq.shape[0])
    if 0 < m_eq < m and m_eq % 2:
        raise ValueError(f"a chunked matrix is cut at the {m_eq} equality rows, and every chunk but the last needs an even row "
                         f"count; {MULTI_GPU}")
    cuts = []
    for blk in (eq, ineq):
        if blk is not None and blk.shape[0] > 0:
            c = ChunkedDeviceMatrix.balanced_cuts(blk.indptr, int(entries))
            cuts += [(blk, r0, r1) for r0, r1 in zip(c, c[1:])]
    ncol_out = ncol if keep is None else int(np.count_nonzero(keep))
    g = ChunkedDeviceMatrix(ncol_out, expect_chunks=len(cuts), expect_rows=m)
    a_shift = [] if keep is not None else None
    try:
        for blk, r0, r1 in cuts:
            chunk = DeviceMatrix.from_csr(rows_of(blk, r0, r1))
            if keep is not None:
                reduced, part = chunk.remove_columns(keep, shift)
                chunk.close()
                chunk = reduced
                a_shift.append(part)
            g.append(chunk)
    except BaseException:
        g.close()
        raise
    return g, (None if a_shift is None else np.concatenate(a_shift))
