"""The stored item of the tall-cell format (csrc/slp_tall_item.h): every field where the LDS address wants it -- the value id at
bit 3, the column at bit 14, the SUM FIELD (1 + the value table's capacity + the local row: where the row's running sum lies in the
product kernel's LDS, behind the scratch cell and the table) with its low 6 bits at bit 26 and its upper 8 bits in the fifth byte;
fp64 items: sum field at bit 3, column at bit 17.  Every comparison is bit for bit against the oracle's sequential sums
(oracle/slp_oracle.c), both orientations, value-dictionary items (policy 0, kernel 6) and fp64 entries (policy 1, kernel 7), as
``test_gpu_tall_frame.py`` does it; no tolerance anywhere.

What can go wrong with the encoding: a field that spills into its neighbour (value ids above 1 023: bit 10; columns 2 047 / 2 048
/ 3 071 / 4 095; sum fields around 64 -- where the word's 6 bits end and the fifth byte begins -- around 2^13 and at the block's
last row), the fifth bytes of the other three items of a group leaking into an address, the table's capacity entering the sum
field (a table of 1 280 entries beside 13 021 rows, one of 1 536 and 2 048 on shorter blocks, none with fp64 entries), the scratch
cell at LDS address 0 taking the skip items and the words no lane owns (lists of 3, 4 and 5 in one cell, slots narrower than slot 0,
a slot two lanes wide), continuation packets, empty cells and strips, a ragged last strip, a short last row block, chunks in one
launch (A^T: the sums stay in LDS over three segments whose tables are reloaded).  -m gpu."""
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


def _values(rng, k, decimals=2):
    v = np.round(rng.randn(k), decimals)
    v[v == 0] = 0.5
    return v


def _from_triplets(m, n, rows, cols, seed, decimals=2):
    """CSR with sorted rows from (row, column) pairs (duplicates merged), values rounded to ``decimals`` places."""
    a = scipy.sparse.coo_matrix((np.ones(len(rows)), (np.asarray(rows), np.asarray(cols))), shape=(m, n)).tocsr()
    a.sum_duplicates()
    a.sort_indices()
    a.data = _values(np.random.RandomState(seed), a.nnz, decimals)
    return a


def _random_pairs(m, n, density, seed):
    rng = np.random.RandomState(seed)
    k = int(round(density * m * n))
    return list(rng.randint(0, m, size=k)), list(rng.randint(0, n, size=k))


def _check(a_host, rows_per_block, width, policies=((0, 6), (1, 7)), want_rows=None):
    """Both products of both value kinds against the oracle; both copies must run on the tall-cell kernel of the policy with the
    forced strip width (``want_rows``: the copy of A with that many rows per block)."""
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
            c, ct = int(a._l.slp_matrix_strip_width(a._h, 0)), int(a._l.slp_matrix_strip_width(a._h, 1))
            r, rt = int(a._l.slp_matrix_tall_rows(a._h, 0)), int(a._l.slp_matrix_tall_rows(a._h, 1))
            print("shape", a_host.shape, "nnz", a_host.nnz, "policy", policy, "kernels", k, kt, "C", c, ct, "R", r, rt)
            assert k == want and kt == want, (policy, k, kt)
            assert c == width and ct == width, (policy, c, ct)
            if want_rows:
                assert r == want_rows, (policy, r)
            assert np.array_equal(a.matvec(x), ax), (policy, k)
            assert np.array_equal(a.rmatvec(y), aty), (policy, kt)
    finally:
        a.close()


# ---- sum fields above 2^13, the split between the word and the fifth byte, the columns' upper bits ---------------------------
def test_one_block_of_13021_rows_on_two_strips_of_3072_columns():
    """Beside 13 021 rows and tiles of 3 072 columns the table holds 1 280 entries: the sum fields run from 1 281 to 14 301 (fp64
    items: 1 to 13 021).  Planted: local rows 63, 64, 8 191, 8 192 and 13 020 x columns 0, 2 047, 2 048, 3 071 of either strip."""
    m, n = 13021, 6144
    rows, cols = _random_pairs(m, n, 3e-4, 61)
    for r in (63, 64, 8191, 8192, 13020):
        for c in (0, 2047, 2048, 3071):
            rows += [r, r]
            cols += [c, 3072 + c]
    a = _from_triplets(m, n, rows, cols, 62)
    assert all(a[r, c] != 0 for r in (63, 64, 8191, 8192, 13020) for c in (0, 2047, 2048, 3071, 3072, 6143))
    _check(a, 13021, 3072, want_rows=13021)


# ---- value ids with bit 10 set ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("values", [1500, 2048])
def test_more_than_1024_distinct_values(values):
    rows, cols = _random_pairs(4096, 8192, 0.5e-3, 63)
    a = _from_triplets(4096, 8192, rows, cols, 64)
    pool = (np.arange(values) + 1.0) / 4096.0 * np.where(np.arange(values) % 2, -1.0, 1.0)
    a.data = pool[np.random.RandomState(65).permutation(a.nnz) % values]
    assert np.unique(a.data).size == values > 1024          # the dictionary: one entry per distinct stored value
    _check(a, 2048, 4096, policies=((0, 6),))               # kernel 6: the copy with value-dictionary items


# ---- lists of 3, 4 and 5 in one cell ---------------------------------------------------------------------------------------
def _cell_with_lists_of_3_4_and_5():
    """4 096 x 8 192 as ONE row block on two strips of 4 096 columns.  Strip 0: two rows of 5 entries, 900 of 2, 1 766 of 1 --
    3 576 items over 1 024 lanes: the two long rows are lists of 5 on lanes 0 and 1 (a fifth-item slot two lanes wide), the first
    3 576 - 3 x 1 024 = 504 lanes are brought to 4 items and the rest to 3 (slot 3 is 504 lanes wide, no multiple of 64, in front
    of the fifth-byte words; the last lanes, four items short because of the two long rows, get skip items).  Strip 1: 700 rows
    of one entry -- slot 0 is 700 lanes wide and the non-zero fifth-byte words follow it directly."""
    rng = np.random.RandomState(66)
    rows, cols = [], []
    order = rng.permutation(4096)
    cursor = 0
    for count, entries in ((2, 5), (900, 2), (1766, 1)):
        for r in order[cursor:cursor + count]:
            rows += [r] * entries
            cols += list(rng.choice(4096, size=entries, replace=False))
        cursor += count
    for r in rng.choice(4096, size=700, replace=False):
        rows.append(r)
        cols.append(4096 + rng.randint(4096))
    a = _from_triplets(4096, 8192, rows, cols, 67)
    per_row = np.diff(a[:, :4096].tocsr().indptr)
    assert a[:, :4096].nnz == 3576 and (per_row == 5).sum() == 2 and (per_row == 2).sum() == 900 and (per_row == 1).sum() == 1766
    assert a[:, 4096:].nnz == 700
    return a


def test_lists_of_3_4_and_5_in_one_cell_and_a_slot_of_700_lanes():
    _check(_cell_with_lists_of_3_4_and_5(), 4096, 4096, want_rows=4096)


# ---- continuation packets, empty cells and strips, ragged edges, the three instantiated widths -------------------------------
def _edges(width):
    """3 000 rows in blocks of 1 024 (the last: 952) x 3 strips and 321 columns (odd: the last tile ends inside a 16-byte piece).
    Strip 1 is empty, the cell (block 1, strip 0) is empty, row 7 has 30 entries inside 200 columns of strip 0 (four packets for one
    lane), row 2 999 has 17 in the last, ragged strip."""
    m, n = 3000, 3 * width + 321
    rng = np.random.RandomState(68 + width // 1024)
    rows, cols = _random_pairs(m, n, min(4e-4 * 4096 / width, 6e-4), 69 + width // 1024)   # (below 2.5 entries per row and 4 096 columns)
    keep = [(r, c) for r, c in zip(rows, cols) if not (width <= c < 2 * width) and not (1024 <= r < 2048 and c < width) and r not in (7, 2999)]
    keep += [(7, 100 + int(c)) for c in rng.choice(200, size=30, replace=False)]
    keep += [(2999, 3 * width + int(c)) for c in rng.choice(321, size=17, replace=False)]
    a = _from_triplets(m, n, [r for r, _ in keep], [c for _, c in keep], 70)
    assert a[:, width:2 * width].nnz == 0 and a[1024:2048, :width].nnz == 0 and a[7].nnz == 30 and a[2999, 3 * width:].nnz == 17
    return a


@pytest.mark.parametrize("width", [1024, 3072, 4096])
def test_long_rows_empty_cells_an_empty_strip_and_ragged_edges(width):
    _check(_edges(width), 1024, width)


def test_abs_power_sums_on_the_fp64_copy():
    """``slp_matrix_spmv_abs_pow`` walks the fp64 copy (sum field at bit 3, column at bit 17) with the POW instantiation."""
    from pysparselp_amd.device import DeviceMatrix

    a_host = _edges(3072)
    os.environ["SLP_TALL_R"], os.environ["SLP_TALL_C"] = "1024", "3072"
    a = DeviceMatrix.from_csr(a_host)
    try:
        a.set_format(1)
        assert a.spmv_kernel(False) == 7 and a.spmv_kernel(True) == 7
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
@pytest.mark.parametrize("policy, want", [(0, 6), (1, 7)])
def test_three_chunks_in_one_launch(policy, want):
    """A x: one grid over the row blocks of all chunks; A^T y: one workgroup per column block walks the three chunks in order over
    ONE set of running sums -- the sum fields of all three chunks must name the same LDS cells (one table capacity), and each
    chunk's table is loaded in front of the sums without touching them."""
    from pysparselp_amd.device import ChunkedDeviceMatrix, DeviceMatrix

    rows, cols = _random_pairs(6144, 8192, 0.55e-3, 71)
    rows += [7] * 30
    cols += list(100 + np.random.RandomState(72).choice(200, size=30, replace=False))
    a_host = _from_triplets(6144, 8192, rows, cols, 73)
    os.environ["SLP_TALL_R"], os.environ["SLP_TALL_C"] = "2048", "4096"
    cuts = [0, 2048, 4096 + 10, 6144]
    g = ChunkedDeviceMatrix(a_host.shape[1], expect_chunks=len(cuts) - 1)
    try:
        for r0, r1 in zip(cuts, cuts[1:]):
            ch = DeviceMatrix.from_csr(a_host[r0:r1])
            if policy:
                ch.set_format(policy)
            g.append(ch)
        assert g.spmv_kernel(False) == want and g.spmv_kernel(True) == want, (g.spmv_kernel(False), g.spmv_kernel(True))
        assert int(g._l.slp_matrix_product_launches(g._h, 0)) == 1 and int(g._l.slp_matrix_product_launches(g._h, 1)) == 1
        rng = np.random.RandomState(6)
        x, y = rng.randn(a_host.shape[1]), rng.randn(a_host.shape[0])
        oa = oracle.as_csr(a_host)
        assert np.array_equal(g.matvec(x), oracle.matvec(oa, x))
        assert np.array_equal(g.rmatvec(y), oracle.rmatvec(oa, y))
    finally:
        g.close()
