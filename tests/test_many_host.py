"""The host helpers that the three list solvers share (``pysparselp_amd/_many.py``): the stacking of the LPs' CSR blocks against
``scipy.sparse.block_diag`` and the checks of the starts.  None of it needs a GPU or the library."""
import numpy as np
import pytest
import scipy.sparse

from pysparselp_amd._many import check_starts, concat_starts, stack_blocks


def _blocks():
    """Three random CSR blocks of 0, 1 and 5 rows over 3, 4 and 2 columns, entries in the order scipy made them."""
    rs = np.random.RandomState(5)
    return [scipy.sparse.random(rows, cols, density=0.6, format="csr", random_state=rs) for rows, cols in ((0, 3), (1, 4), (5, 2))]


def _triples(blocks):
    return [(a.indptr, a.indices, a.data) for a in blocks]


def test_stacked_blocks_with_offsets_are_the_block_diagonal():
    blocks = _blocks()
    assert sum(a.nnz for a in blocks) >= 4
    want = scipy.sparse.block_diag(blocks).tocsr()
    indptr, indices, data = stack_blocks(_triples(blocks), [0, 3, 7])
    assert (indptr.dtype, indices.dtype, data.dtype) == (np.int64, np.int32, np.float64)
    assert all(v.flags.c_contiguous for v in (indptr, indices, data))
    assert np.array_equal(indptr, want.indptr) and np.array_equal(indices, want.indices) and np.array_equal(data, want.data)


def test_stacked_blocks_without_offsets_keep_their_local_columns():
    blocks = _blocks()
    # the same columns for all: pad every block to the widest, stack by rows
    want = scipy.sparse.vstack([scipy.sparse.csr_matrix((a.data, a.indices, a.indptr), shape=(a.shape[0], 4)) for a in blocks]).tocsr()
    indptr, indices, data = stack_blocks(_triples(blocks))
    assert np.array_equal(indptr, want.indptr) and np.array_equal(indices, want.indices) and np.array_equal(data, want.data)
    assert indptr.shape == (7,) and indptr[0] == 0 and indptr[1] == blocks[1].nnz


def test_no_blocks_stack_to_an_empty_matrix():
    indptr, indices, data = stack_blocks([])
    assert np.array_equal(indptr, [0]) and indptr.dtype == np.int64
    assert indices.shape == (0,) and indices.dtype == np.int32
    assert data.shape == (0,) and data.dtype == np.float64


def test_starts_are_checked_per_lp_and_concatenated():
    lps = [(np.zeros(2),), (np.zeros(3),), (np.zeros(1),)]
    assert check_starts(None, lps) is None
    with pytest.raises(ValueError, match="x0 must be None or a sequence of 3 starts, one per LP"):
        check_starts([None, None], lps)
    with pytest.raises(ValueError, match="x0 must be None or a sequence of 3 starts, one per LP"):
        check_starts(1.0, lps)
    with pytest.raises(ValueError, match=r"LP 1: x0 has shape \(2,\), c has 3 entries"):
        check_starts([None, [1.0, 2.0], None], lps)
    bad = [[1.0, 2.0], None, [np.inf]]
    with pytest.raises(ValueError, match="LP 2: x0 has an entry that is not finite"):
        check_starts(bad, lps, finite=True)
    x0 = check_starts(bad, lps)
    assert x0[1] is None and np.array_equal(x0[0], [1.0, 2.0]) and np.array_equal(x0[2], [np.inf])
    assert all(v is None or (v.dtype == np.float64 and v.flags.c_contiguous) for v in x0)
    flat = concat_starts(x0, [2, 3, 1])
    assert np.array_equal(flat, [1.0, 2.0, 0.0, 0.0, 0.0, np.inf]) and flat.dtype == np.float64 and flat.flags.c_contiguous
    assert concat_starts([None, None, None], [2, 3, 1]) is None
    assert concat_starts(None, [2, 3, 1]) is None
