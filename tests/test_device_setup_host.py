"""Route choice of ``setup="auto" | "host" | "device"`` (``host_setup.py``) without a GPU: the threshold keeps every golden
fixture LP on the host route, the row slices handed to the device are views of the caller's arrays (no host copy of the
values), and an unknown ``setup`` is refused."""
import glob
import os

import numpy as np
import pytest
import scipy.sparse

from conftest import GOLDEN, csr_of


def test_device_setup_threshold_keeps_the_fixtures_on_the_host():
    from pysparselp_amd import host_setup
    from pysparselp_amd.SparseLP import DEVICE_SETUP_ENTRIES

    assert DEVICE_SETUP_ENTRIES >= 1e7
    largest = 0
    for path in glob.glob(os.path.join(GOLDEN, "lp_*.npz")):
        d = dict(np.load(path))
        nnz = host_setup.nnz_of(csr_of(d, "Ae"), csr_of(d, "Ai"))
        largest = max(largest, nnz)
        assert host_setup.choose("auto", nnz) == "host", path
    assert largest > 0
    assert host_setup.choose("auto", int(DEVICE_SETUP_ENTRIES)) == "device"
    assert host_setup.choose("host", 10 ** 12) == "host" and host_setup.choose("device", 0) == "device"


def test_unknown_setup_is_refused():
    from pysparselp_amd import host_setup

    with pytest.raises(ValueError, match="setup"):
        host_setup.choose("gpu", 10)


def test_row_slices_are_views_of_the_host_blocks():
    from pysparselp_amd import host_setup

    a = scipy.sparse.random(50, 30, density=0.2, format="csr", random_state=3)
    part = host_setup.rows_of(a, 10, 35)
    assert part.shape == (25, 30) and part.indptr[0] == 0 and part.nnz == a.indptr[35] - a.indptr[10]
    assert np.shares_memory(part.data, a.data) and np.shares_memory(part.indices, a.indices)
    assert np.array_equal(part.tocsr().toarray(), a[10:35].toarray())
    assert host_setup.rows_of(a, 7, 7) is None and host_setup.rows_of(None, 0, 3) is None


def test_without_a_communicator_every_row_is_local():
    from pysparselp_amd import host_setup

    a_eq = scipy.sparse.random(4, 9, density=0.5, format="csr", random_state=1)
    a_in = scipy.sparse.random(11, 9, density=0.5, format="csr", random_state=2)
    assert host_setup.local_blocks(a_eq, a_in) == ((0, 4), (0, 11))
    assert host_setup.local_blocks(None, a_in) == ((0, 0), (0, 11))


def test_distinct_value_count_stops_at_the_dictionary_size():
    from pysparselp_amd import host_setup

    few = host_setup.rows_of(scipy.sparse.csr_matrix(np.round(np.random.RandomState(0).randn(40, 40), 1)), 0, 40)
    many = host_setup.rows_of(scipy.sparse.random(100, 100, density=0.5, format="csr", random_state=0), 0, 100)
    assert host_setup.few_distinct_values((few, None))
    assert not host_setup.few_distinct_values((few, many))
