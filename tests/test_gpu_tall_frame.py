"""The cell frame of the tall-cell product kernel (csrc/slp_tall_spmv.hip): slot loads through ONE payload descriptor (a slot
is the load's scalar offset and the descriptor's num_records), header fields read once per packet step, and the staging of
the x-tile (the form by dwords, tools/lab/patches/tall_frame_step3_addtid_tile.patch, passes the same cases).  Every comparison is bit for bit against the oracle's sequential sums (oracle/slp_oracle.c); no tolerance anywhere.

Slot edges.  A slot of a packet is followed in the payload by the next slot's non-zero words, so a load that reads past its
slot's width adds foreign items to a row, and one that stops short of it drops items: the sums differ in many bits.  (Measured
with these cases: the range check of a raw buffer on gfx950 covers the scalar offset -- a lane is out of range when scalar
offset + vector offset >= num_records; with num_records = the slot's width alone every case below fails, with the slot's last
byte + 1 all pass.)  The cells wanted are those with lists 4-5 items long, so that the fifth-item slot
is some hundred lanes wide -- not a multiple of a wave's 64 -- and some waves take the second group of four while others skip
it: 4 200 and 5 030 items per cell (1 024 lanes).  The format selector gives tall cells to matrices with fewer than 2.5
entries per row and 4 096 columns, and the LDS strips to rows with 3 or more entries per 5 888 / 7 680 columns
(slp_tall.hip tall_wanted, slp_strip.hip strip_wanted), so a cell of 1 024 rows holds at most 2 560 items: the cells of that
size are formed from 2 048 rows (``SLP_TALL_R=2048``, 4 096 x 8 192 at densities 0.5e-3 and 0.6e-3: 4 194 / 5 033 items per
cell, both value kinds on tall cells in both orientations).  The shape 2 048 x 12 288 at 1.0e-3 / 1.2e-3 with 1 024-row
blocks is run as well: there A goes to the strips and A^T (12 288 rows, one 2 048-column strip, lists 2-3 long) to tall cells.

Tile edges.  x is drawn from randn, so a dword of the tile that lands in another place changes bits: a last tile that ends
inside a wave's 256-byte piece (n = 3 * 4096 + 321, odd), a matrix narrower than one strip (n = 700), the three strip
widths, and a last row block of 952 rows (m = 3000 in blocks of 1024).  -m gpu."""
import os

import numpy as np
import pytest
import scipy.sparse

from oracle import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _small_matrices_take_the_tall_format():
    os.environ["SLP_STRIP_MIN_NNZ"] = "1"
    yield
    del os.environ["SLP_STRIP_MIN_NNZ"]
    os.environ.pop("SLP_TALL_R", None)
    os.environ.pop("SLP_TALL_C", None)


def _check(a_host, rows_per_block=None, policies=((0, 6), (1, 7)), width=None, tall_a=True, tall_at=None):
    """Both products of both value kinds against the oracle.  ``tall_a``: A must run on the tall-cell kernel of the policy
    (``tall_at``: A^T must); printed either way."""
    from pysparselp_amd.device import DeviceMatrix

    for name, v in (("SLP_TALL_R", rows_per_block), ("SLP_TALL_C", width)):
        if v:
            os.environ[name] = str(v)
        else:
            os.environ.pop(name, None)
    a = DeviceMatrix.from_csr(a_host)
    try:
        rng = np.random.RandomState(3)
        x, y = rng.randn(a_host.shape[1]), rng.randn(a_host.shape[0])
        ax, aty = oracle.matvec(oracle.as_csr(a_host), x), oracle.rmatvec(oracle.as_csr(a_host), y)
        for policy, want in policies:   # value-dictionary items (5 bytes) / fp64 entries (4 + 8 bytes)
            a.set_format(policy)
            k, kt = a.spmv_kernel(False), a.spmv_kernel(True)
            print("shape", a_host.shape, "nnz", a_host.nnz, "R", rows_per_block, "C", width, "policy", policy, "kernels", k, kt)
            if tall_a:
                assert k == want, (policy, k)
            if tall_at:
                assert kt == want, (policy, kt)
            assert np.array_equal(a.matvec(x), ax), (policy, k)
            assert np.array_equal(a.rmatvec(y), aty), (policy, kt)
    finally:
        a.close()


def _random(m, n, density, seed, decimals=2):
    """Uniformly placed entries with rounded values (few distinct values: a value dictionary exists)."""
    rng = np.random.RandomState(seed)
    k = int(round(density * m * n))
    a = scipy.sparse.coo_matrix((np.ones(k), (rng.randint(0, m, size=k), rng.randint(0, n, size=k))), shape=(m, n)).tocsr()
    a.sum_duplicates()
    a.sort_indices()
    a.data = np.round(rng.randn(a.nnz), decimals)
    a.data[a.data == 0] = 0.5
    return a


def _with_long_rows(base, seed):
    """A few rows of 9-30 entries inside one strip (and 40 over two): continuation packets, packets without a tile."""
    rng = np.random.RandomState(seed)
    base = base.tocoo()
    m, n = base.shape
    rows, cols, vals = [base.row], [base.col], [base.data]
    for r, (c0, k) in ((7, (100, 30)), (8, (4096 + 5, 9)), (m // 2 + 3, (n - 230, 17)), (m - 1, (0, 13)), (m // 2, (4096 - 100, 40))):
        cc = c0 + np.sort(rng.choice(200, size=k, replace=False))
        keep = ~((rows[0] == r) & np.isin(cols[0], cc))
        rows[0], cols[0], vals[0] = rows[0][keep], cols[0][keep], vals[0][keep]
        rows.append(np.full(k, r)); cols.append(cc); vals.append(np.where(np.round(rng.randn(k), 1) == 0, 0.3, np.round(rng.randn(k), 1)))
    a = scipy.sparse.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=base.shape).tocsr()
    a.sort_indices()
    return a


# ---- slot edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("density", [0.5e-3, 0.6e-3])
def test_slots_whose_width_is_no_multiple_of_a_wave_are_followed_by_other_slots(density):
    a = _random(4096, 8192, density, 31)
    cell = a[:2048, :4096].nnz                     # lists of 4-5 items over 1024 lanes: the fifth-item slot is part of the lanes
    assert 4096 < cell < 5120 + 1024 and a.nnz / 4096 / 2 < 2.5, cell
    _check(a, 2048, width=4096, tall_at=True)      # A: 2 row blocks x 2 strips; A^T: 4 row blocks x 1 strip


@pytest.mark.parametrize("density", [1.0e-3, 1.2e-3])
def test_the_2048_by_12288_shape_in_blocks_of_1024_rows(density):
    a = _random(2048, 12288, density, 32)
    _check(a, 1024, width=4096, tall_a=False, tall_at=True)


def test_continuation_packets_and_packets_without_a_tile_behind_full_slots():
    a = _with_long_rows(_random(4096, 8192, 0.5e-3, 33), 4)
    assert np.diff(a.indptr).max() >= 40
    _check(a, 2048, width=4096)
    _check(a, 1024, width=4096)


def test_abs_power_sums_on_the_fp64_copy():
    """``slp_matrix_spmv_abs_pow`` -- the sums behind Chambolle-Pock's preconditioners (ChambollePockPPD.py:122-179) -- walks the
    fp64 copy with the POW instantiation of the kernel: the value array's slots go through the second descriptor."""
    from pysparselp_amd.device import DeviceMatrix

    a_host = _with_long_rows(_random(4096, 8192, 0.6e-3, 34), 5)
    os.environ["SLP_TALL_R"], os.environ["SLP_TALL_C"] = "2048", "4096"
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


@pytest.mark.parametrize("policy, want", [(0, 6), (1, 7)])
def test_three_chunks_in_one_launch(policy, want):
    """A ``ChunkedDeviceMatrix`` of 3 row chunks: A x is one grid over the row blocks of all chunks, A^T y one workgroup per
    column block that walks the chunks in order (``nseg`` = 3: the descriptors are rebuilt per segment)."""
    from pysparselp_amd.device import ChunkedDeviceMatrix, DeviceMatrix

    a_host = _with_long_rows(_random(6144, 8192, 0.55e-3, 35), 6)
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
        rng = np.random.RandomState(6)
        x, y = rng.randn(a_host.shape[1]), rng.randn(a_host.shape[0])
        oa = oracle.as_csr(a_host)
        assert np.array_equal(g.matvec(x), oracle.matvec(oa, x))
        assert np.array_equal(g.rmatvec(y), oracle.rmatvec(oa, y))
    finally:
        g.close()


# ---- tile edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [4096, 2048, 1024])
@pytest.mark.parametrize("n, density", [(3 * 4096 + 321, 3e-4), (700, 2e-3)])
def test_tiles_that_end_inside_a_piece_and_a_last_row_block_of_952_rows(n, density, width):
    a = _random(3000, n, density, 36 + n % 7)
    _check(a, 1024, width=width)
