"""The pipeline of the tall-cell product kernel (csrc/slp_tall_spmv.hip): the ring of item registers (depth DI = 4 packets, headers
2 DI ahead), the ring of x-tile pieces with a depth DT of its own (``kTallTileDepth`` <= DI, csrc/slp_tall.h), and the first four
items of the NEXT packet decoded -- their values read from the segment's table -- in front of that packet's barrier
(``kTallAhead``).  Every comparison is bit for bit against the oracle's sequential sums (oracle/slp_oracle.c); no tolerance
anywhere.  Both value kinds (value-dictionary items: policy 0, kernel 6; fp64 entries: policy 1, kernel 7), both orientations,
both packet forms (``SLP_TALL_RECORDS`` 0 and 1).

Streams around the ring sizes.  1 024 x 1 024 k in blocks of 1 024 rows on strips of 1 024 columns: A is ONE stream of k cells,
A^T k streams of one cell.  A tile that is loaded for the wrong packet, or stored from a ring slot that was already refilled,
shows where the stream is as long as a ring, one longer, or one shorter: k = 1, 2, DT, DT + 1, DI - 1, DI, DI + 1, 2 DI, 2 DI + 1
for every DT in 2 .. 4 that the kernel's lab builds know -- 1, 2, 3, 4, 5, 8, 9.

Lists of 4-5 with a partial fifth slot, continuation packets, packets without a tile: the shapes of tests/test_gpu_tall_frame.py
(4 096 x 8 192 at 0.5e-3 / 0.6e-3 in blocks of 2 048 rows, and with rows of 9-40 entries) -- a continuation packet has no barrier
in front of it and takes the items read ahead all the same; the second group of four is read where it always was.

Tile edges: n = 3 * 4096 + 321 and n = 700 at the widths 1 024, 3 072 and 4 096.

Segments with tables of their own.  A chunked matrix of 3 and of 4 chunks in ONE launch per product: A^T y walks the chunks as
segments of one workgroup, each with its own value table in the same LDS.  Chunk c's entries are the common draw times 1, 3, 7,
11: the same value id names another value in every chunk, so a table read that reaches across the segment's end -- the last
packet's read-ahead of a prefetch-target packet, the first packet's in front of the prologue's barrier -- changes bits.  -m gpu."""
import os

import numpy as np
import pytest
import scipy.sparse

from oracle import oracle
from test_gpu_tall_frame import _random, _with_long_rows

pytestmark = pytest.mark.gpu

SWITCHES = ("SLP_STRIP_MIN_NNZ", "SLP_TALL_R", "SLP_TALL_C", "SLP_TALL_RECORDS")
POLICIES = ((0, 6), (1, 7))
FORMS = ("0", "1")


@pytest.fixture(autouse=True)
def _small_matrices_take_the_tall_format():
    os.environ["SLP_STRIP_MIN_NNZ"] = "1"
    yield
    for name in SWITCHES:
        os.environ.pop(name, None)


def _reference(a_host):
    rng = np.random.RandomState(3)
    x, y = rng.randn(a_host.shape[1]), rng.randn(a_host.shape[0])
    oa = oracle.as_csr(a_host)
    return x, y, oracle.matvec(oa, x), oracle.rmatvec(oa, y)


def _check(a_host, rows_per_block, width, tall_a=True, tall_at=True):
    """Both products of both value kinds in both packet forms against the oracle (computed once)."""
    from pysparselp_amd.device import DeviceMatrix

    os.environ["SLP_TALL_R"], os.environ["SLP_TALL_C"] = str(rows_per_block), str(width)
    x, y, ax, aty = _reference(a_host)
    for form in FORMS:
        os.environ["SLP_TALL_RECORDS"] = form
        a = DeviceMatrix.from_csr(a_host)
        try:
            for policy, want in POLICIES:
                a.set_format(policy)
                k, kt = a.spmv_kernel(False), a.spmv_kernel(True)
                print("shape", a_host.shape, "nnz", a_host.nnz, "R", rows_per_block, "C", width, "records", form, "policy", policy, "kernels", k, kt)
                if tall_a:
                    assert k == want, (form, policy, k)
                    assert int(a._l.slp_matrix_tall_records(a._h, 0)) == int(form)
                if tall_at:
                    assert kt == want, (form, policy, kt)
                    assert int(a._l.slp_matrix_tall_records(a._h, 1)) == int(form)
                assert np.array_equal(a.matvec(x), ax), (form, policy, k)
                assert np.array_equal(a.rmatvec(y), aty), (form, policy, kt)
        finally:
            a.close()


# ---- streams around the ring sizes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8, 9])
def test_streams_as_long_as_a_ring_one_longer_and_one_shorter(k):
    a = _random(1024, 1024 * k, 0.5e-3, 40 + k)
    _check(a, 1024, 1024)   # A: one stream of k cells; A^T: k streams of one cell


# ---- lists of 4-5, continuation packets, packets without a tile --------------------------------------------------------------
@pytest.mark.parametrize("density", [0.5e-3, 0.6e-3])
def test_a_partial_fifth_slot_behind_items_read_ahead(density):
    a = _random(4096, 8192, density, 31)
    cell = a[:2048, :4096].nnz
    assert 4096 < cell < 5120 + 1024, cell
    _check(a, 2048, 4096)


def test_continuation_packets_and_packets_without_a_tile():
    a = _with_long_rows(_random(4096, 8192, 0.5e-3, 33), 4)
    assert np.diff(a.indptr).max() >= 40
    _check(a, 2048, 4096)


# ---- tile edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1024, 3072, 4096])
@pytest.mark.parametrize("n, density", [(3 * 4096 + 321, 3e-4), (700, 2e-3)])
def test_tiles_that_end_inside_a_piece(n, density, width):
    a = _random(3000, n, density, 36 + n % 7)
    _check(a, 1024, width, tall_at=False)   # (A^T: n rows of up to 6 entries per strip -- not every one a tall-cell copy; compared all the same)


# ---- segments with tables of their own --------------------------------------------------------------------------------------
FACTORS = (1.0, 3.0, 7.0, 11.0)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("policy, kernel", POLICIES)
@pytest.mark.parametrize("chunks", [3, 4])
def test_every_segment_reads_its_own_value_table(chunks, policy, kernel, form):
    from pysparselp_amd.device import ChunkedDeviceMatrix, DeviceMatrix

    cuts = [0, 2048, 4096 + 10, 6144, 8192][:chunks + 1]
    base = _with_long_rows(_random(cuts[-1], 8192, 0.55e-3, 35), 6).tocsr()
    scale = np.ones(base.shape[0])
    for c, (r0, r1) in enumerate(zip(cuts, cuts[1:])):
        scale[r0:r1] = FACTORS[c]
    a_host = scipy.sparse.diags(scale).dot(base).tocsr()   # (an entry is rounded to two decimals: its product with 3, 7, 11 is one rounding)
    a_host.sort_indices()
    x, y, ax, aty = _reference(a_host)
    os.environ["SLP_TALL_R"], os.environ["SLP_TALL_C"], os.environ["SLP_TALL_RECORDS"] = "2048", "4096", form
    g = ChunkedDeviceMatrix(a_host.shape[1], expect_chunks=chunks)
    try:
        for r0, r1 in zip(cuts, cuts[1:]):
            ch = DeviceMatrix.from_csr(a_host[r0:r1])
            if policy:
                ch.set_format(policy)
            g.append(ch)
        assert g.spmv_kernel(False) == kernel and g.spmv_kernel(True) == kernel, (g.spmv_kernel(False), g.spmv_kernel(True))
        assert int(g._l.slp_matrix_product_launches(g._h, 1)) == 1     # A^T y: the chunks are segments of one workgroup
        assert int(g._l.slp_matrix_product_launches(g._h, 0)) == 1
        assert np.array_equal(g.matvec(x), ax)
        assert np.array_equal(g.rmatvec(y), aty)
    finally:
        g.close()
