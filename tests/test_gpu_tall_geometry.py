"""Tall cells on strips of any multiple of 256 columns, row blocks taller than 9 984 rows and a value table sized by its
dictionary (csrc/slp_tall_plan.h, slp_tall.hip, slp_tall_spmv.hip).  Every comparison is bit for bit against the oracle's
sequential sums (oracle/slp_oracle.c), both orientations, value-dictionary items (policy 0, kernel 6) and fp64 entries
(policy 1, kernel 7), the way ``test_gpu_tall_frame.py`` checks the cell frame; no tolerance anywhere.

What can go wrong with a run-time width: the builder's division by C (an entry in the wrong strip or column), the first column
of a tile (``strip * C``), the dealing of a tile's C / 2 16-byte pieces to the 1 024 lanes -- a second piece on the first
C / 2 - 1 024 lanes only (1 280: no second piece and a first piece on 640 lanes; 2 560: 256 lanes; 3 072: 512; 3 584: 768) --
and a last tile that ends inside a piece (odd column count).  With taller blocks: the row field of an item (14 bits, the local
row + 1 up to 13 021), the sums' area in LDS pushing the value table and the tiles to other offsets, and a table of 2 048
entries leaving room for fewer rows.  -m gpu."""
import os

import numpy as np
import pytest
import scipy.sparse

from oracle import oracle

pytestmark = pytest.mark.gpu

SWITCHES = ("SLP_STRIP_MIN_NNZ", "SLP_TALL_R", "SLP_TALL_C")


@pytest.fixture(autouse=True)
def _small_matrices_take_the_tall_format():
    os.environ["SLP_STRIP_MIN_NNZ"] = "1"
    yield
    for name in SWITCHES:
        os.environ.pop(name, None)


def _random(m, n, density, seed, decimals=2):
    rng = np.random.RandomState(seed)
    k = int(round(density * m * n))
    a = scipy.sparse.coo_matrix((np.ones(k), (rng.randint(0, m, size=k), rng.randint(0, n, size=k))), shape=(m, n)).tocsr()
    a.sum_duplicates()
    a.sort_indices()
    a.data = np.round(rng.randn(a.nnz), decimals)
    a.data[a.data == 0] = 0.5
    return a


def _with_rows(base, rows, seed):
    """``rows``: (row, first column, span, entries) -- the row's entries are replaced by ``entries`` ones inside the span."""
    rng = np.random.RandomState(seed)
    a = base.tolil()
    for r, c0, span, k in rows:
        a[r, :] = 0
        for c in c0 + np.sort(rng.choice(span, size=k, replace=False)):
            a[r, int(c)] = 0.1 * (1 + int(c) % 7)
    a = a.tocsr()
    a.eliminate_zeros()
    a.sort_indices()
    return a


def _check(a_host, rows_per_block, width, want_rows=None, policies=((0, 6), (1, 7))):
    """Both products of both value kinds against the oracle; A must run on the tall-cell kernel of the policy with the forced
    strip width (``want_rows``: and with that many rows per block)."""
    from pysparselp_amd.device import DeviceMatrix

    os.environ["SLP_TALL_R"], os.environ["SLP_TALL_C"] = str(rows_per_block), str(width)
    a = DeviceMatrix.from_csr(a_host)
    try:
        rng = np.random.RandomState(3)
        x, y = rng.randn(a_host.shape[1]), rng.randn(a_host.shape[0])
        oa = oracle.as_csr(a_host)
        ax, aty = oracle.matvec(oa, x), oracle.rmatvec(oa, y)
        for policy, want in policies:
            a.set_format(policy)
            k, kt = a.spmv_kernel(False), a.spmv_kernel(True)
            c, r = int(a._l.slp_matrix_strip_width(a._h, 0)), int(a._l.slp_matrix_tall_rows(a._h, 0))
            ct, rt = int(a._l.slp_matrix_strip_width(a._h, 1)), int(a._l.slp_matrix_tall_rows(a._h, 1))
            print("shape", a_host.shape, "nnz", a_host.nnz, "policy", policy, "kernels", k, kt, "C", c, ct, "R", r, rt)
            assert k == want and c == width, (policy, k, c)
            assert kt == want and ct == width, (policy, kt, ct)       # the copy of A^T: the same kernel on the forced width
            assert rt == (want_rows[policy] if want_rows else rows_per_block), (policy, rt)   # (one dictionary for both copies)
            if want_rows:
                assert r == want_rows[policy], (policy, r)
            assert np.array_equal(a.matvec(x), ax), (policy, k)
            assert np.array_equal(a.rmatvec(y), aty), (policy, kt)
    finally:
        a.close()


# ---- strip widths that are no power of two -------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1280, 2560, 3072, 3584])
def test_strips_of_any_multiple_of_256_columns(width):
    n = 3 * width + 1235                                   # odd: the last tile ends inside a 16-byte piece
    _check(_random(4096, n, 5e-4, 40 + width // 256), 2048, width)


def test_continuation_packets_on_strips_of_3072_columns():
    width, n = 3072, 3 * 3072 + 1235
    a = _with_rows(_random(4096, n, 5e-4, 47), [(7, 100, 200, 30), (2050, width - 20, 200, 40), (4095, n - 230, 230, 17)], 8)
    assert np.diff(a.indptr).max() >= 40                   # 40 entries over the edge of two strips: 20-odd items in one lane's list
    _check(a, 2048, width)


# ---- row blocks taller than 9984 rows --------------------------------------------------------------------------------------
def _tall_block_matrix(m, values=None, seed=51):
    """m x 6145 at density 1e-4 (strips of 3072 columns: the third holds one column): a row with entries in every strip, an empty
    row, and an entry in row 13 020 -- local row + 1 = 13 021, the largest row field.  ``values``: that many distinct values."""
    a = _with_rows(_random(m, 6145, 1e-4, seed), [(5, 0, 3, 3), (9000, 3071, 2, 2), (13020, 6000, 100, 3), (11111, 0, 1, 0)], 9).tolil()
    a[9000, 6144] = 0.7                                     # row 9000: columns 3071 | 3072 | 6144 -- all three strips
    a = a.tocsr()
    a.sort_indices()
    assert a.indptr[11112] == a.indptr[11111] and a[13020].nnz == 3 and set(a[9000].indices // 3072) == {0, 1, 2}
    if values:
        assert a.nnz >= values
        pool = (np.arange(values) + 1.0) / 4096.0 * np.where(np.arange(values) % 2, -1.0, 1.0)
        a.data = pool[np.random.RandomState(seed).permutation(a.nnz) % values]
        assert np.unique(a.data).size == values
    return a


@pytest.mark.parametrize("m", [13021, 13022])
def test_a_row_block_of_13021_rows(m):
    """13 021 rows: one block of the full height; 13 022: a last block of one row."""
    _check(_tall_block_matrix(m), 13021, 3072, want_rows={0: 13021, 1: 13021})


@pytest.mark.parametrize("values, rows", [(1, 13021), (1152, 13021), (1153, 13021), (2048, 12287)])
def test_the_value_table_takes_what_its_dictionary_needs(values, rows):
    """8 (R + 1) + 8 capacity + 16 C <= 163 840: beside 13 021 rows of sums and tiles of 3 072 columns the table holds 1 280 entries;
    a dictionary of 2 048 values takes the whole table and leaves (163 840 - 16 384 - 49 152) / 8 - 1 = 12 287 rows."""
    _check(_tall_block_matrix(13022, values), 13021, 3072, want_rows={0: rows, 1: 13021})


def test_abs_power_sums_on_the_fp64_copy_at_3072_columns():
    from pysparselp_amd.device import DeviceMatrix

    a_host = _random(4096, 3 * 3072 + 1235, 5e-4, 52)
    os.environ["SLP_TALL_R"], os.environ["SLP_TALL_C"] = "2048", "3072"
    a = DeviceMatrix.from_csr(a_host)
    try:
        a.set_format(1)
        assert a.spmv_kernel(False) == 7 and a.spmv_kernel(True) == 7
        assert int(a._l.slp_matrix_strip_width(a._h, 0)) == 3072 and int(a._l.slp_matrix_strip_width(a._h, 1)) == 3072
        oa = oracle.as_csr(a_host)
        rng = np.random.RandomState(5)
        x, y = rng.randn(a_host.shape[1]), rng.randn(a_host.shape[0])
        for p in (1.0, 2.0, 0.5):
            powered = oracle.Csr(oa.indptr, oa.indices, np.abs(oa.data) ** p, oa.shape)
            assert np.array_equal(a.abs_pow_matvec(x, p), oracle.matvec(powered, x)), p
            assert np.array_equal(a.abs_pow_matvec(y, p, transposed=True), oracle.rmatvec(powered, y)), p
    finally:
        a.close()


# ---- chunks ------------------------------------------------------------------------------------------------------------------
def _chunked(a_host, cuts, policy, expect_rows=0):
    from pysparselp_amd.device import ChunkedDeviceMatrix, DeviceMatrix

    g = ChunkedDeviceMatrix(a_host.shape[1], expect_chunks=len(cuts) - 1, expect_rows=expect_rows)
    for r0, r1 in zip(cuts, cuts[1:]):
        ch = DeviceMatrix.from_csr(a_host[r0:r1])
        if policy:
            ch.set_format(policy)
        g.append(ch)
    return g


@pytest.mark.parametrize("policy, want", [(0, 6), (1, 7)])
def test_three_unequal_chunks_at_3072_columns_in_one_launch(policy, want):
    from pysparselp_amd.device import DeviceMatrix

    a_host = _random(6144, 3 * 3072 + 1235, 5e-4, 53)
    os.environ["SLP_TALL_R"], os.environ["SLP_TALL_C"] = "2048", "3072"
    whole = DeviceMatrix.from_csr(a_host)
    g = _chunked(a_host, [0, 1024, 4096 + 10, 6144], policy)
    try:
        whole.set_format(policy)
        assert g.spmv_kernel(False) == want and g.spmv_kernel(True) == want
        assert int(g._l.slp_matrix_strip_width(g._h, 0)) == 3072 and int(g._l.slp_matrix_strip_width(g._h, 1)) == 3072
        assert int(g._l.slp_matrix_product_launches(g._h, 0)) == 1 and int(g._l.slp_matrix_product_launches(g._h, 1)) == 1
        rng = np.random.RandomState(6)
        x, y = rng.randn(a_host.shape[1]), rng.randn(a_host.shape[0])
        oa = oracle.as_csr(a_host)
        ax, aty = g.matvec(x), g.rmatvec(y)
        assert np.array_equal(ax, whole.matvec(x)) and np.array_equal(aty, whole.rmatvec(y))    # the unchunked product
        assert np.array_equal(ax, oracle.matvec(oa, x)) and np.array_equal(aty, oracle.rmatvec(oa, y))
    finally:
        g.close()
        whole.close()


@pytest.mark.parametrize("policy, want", [(0, 6), (1, 7)])
def test_unequal_chunks_share_the_row_blocks_of_the_whole_matrix(policy, want):
    """Rows per block left to the planner: the chunks of a matrix whose row count is announced take their shares of a multiple of
    the compute units of row blocks, each counted from what the chunks in front took -- on 256 compute units 300 000 rows are
    256 blocks: 128 of 1 172 rows for the first 150 000, 42 of 1 191 for the next 50 002 and 86 of 1 163 for the rest.  One launch, the unchunked sums."""
    import torch

    a_host = _random(300000, 3072 + 1027, 2e-4, 55)
    os.environ["SLP_TALL_C"] = "3072"
    g = _chunked(a_host, [0, 150000, 200002, 300000], policy, expect_rows=300000)
    try:
        assert g.spmv_kernel(False) == want and g.spmv_kernel(True) == want
        assert int(g._l.slp_matrix_strip_width(g._h, 0)) == 3072 and int(g._l.slp_matrix_strip_width(g._h, 1)) == 3072
        assert int(g._l.slp_matrix_product_launches(g._h, 0)) == 1 and int(g._l.slp_matrix_product_launches(g._h, 1)) == 1
        rows = int(g._l.slp_matrix_tall_rows(g._h, 0))
        print("compute units", torch.cuda.get_device_properties(0).multi_processor_count, "rows per block of the first chunk", rows)
        if torch.cuda.get_device_properties(0).multi_processor_count == 256:
            assert rows == 1172
        rng = np.random.RandomState(8)
        x, y = rng.randn(a_host.shape[1]), rng.randn(a_host.shape[0])
        oa = oracle.as_csr(a_host)
        assert np.array_equal(g.matvec(x), oracle.matvec(oa, x)) and np.array_equal(g.rmatvec(y), oracle.rmatvec(oa, y))
    finally:
        g.close()


def test_a_fourth_chunk_whose_dictionary_outgrows_the_carried_capacity():
    """The first chunk settles strip width and table capacity (1 280 entries beside 13 021 rows) for the chunks behind it; a chunk
    with 1 500 distinct values takes the whole table, and the products then run chunk by chunk."""
    a_host = _random(8192, 3 * 3072 + 1235, 5e-4, 54)
    lo = a_host.indptr[6144]
    assert a_host.nnz - lo >= 1500
    pool = (np.arange(1500) + 1.0) / 2048.0
    a_host.data[lo:] = pool[np.arange(a_host.nnz - lo) % 1500]
    os.environ["SLP_TALL_R"], os.environ["SLP_TALL_C"] = "13021", "3072"
    cuts = [0, 1024, 4096 + 10, 6144, 8192]
    rng = np.random.RandomState(7)
    x, y = rng.randn(a_host.shape[1]), rng.randn(a_host.shape[0])
    three = _chunked(a_host[:6144], cuts[:4], 0)
    try:
        assert int(three._l.slp_matrix_product_launches(three._h, 0)) == 1 and int(three._l.slp_matrix_product_launches(three._h, 1)) == 1
    finally:
        three.close()
    g = _chunked(a_host, cuts, 0)
    try:
        assert g.spmv_kernel(False) == 6 and g.spmv_kernel(True) == 6
        assert int(g._l.slp_matrix_product_launches(g._h, 0)) == 4 and int(g._l.slp_matrix_product_launches(g._h, 1)) == 4
        oa = oracle.as_csr(a_host)
        assert np.array_equal(g.matvec(x), oracle.matvec(oa, x))
        assert np.array_equal(g.rmatvec(y), oracle.rmatvec(oa, y))
    finally:
        g.close()
