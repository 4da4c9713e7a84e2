"""The two packet forms of a tall-cell copy (csrc/slp_tall_item.h): slot-major, and the first four list positions of a packet as
one 16-byte record per lane, which the product kernel reads with ONE load where the slot-major form takes four.  The planner
chooses per copy by the bytes the records would add (csrc/slp_tall_plan.h: at most 1/16), ``SLP_TALL_RECORDS=0|1`` forces the form,
the chunks of a chunked matrix follow their first chunk, and ``slp_matrix_tall_records`` says which form a copy has.

Every product -- both value kinds (value-dictionary items: policy 0, kernel 6; fp64 entries: policy 1, kernel 7), both orientations,
the form forced on, forced off and chosen by the planner -- is compared bit for bit with the oracle's sequential sums
(oracle/slp_oracle.c); no tolerance anywhere.  What can go wrong with records: a padding word that does not decode to the scratch
cell (lists of 3 and fewer inside slot 0's lanes; a strip of single-entry rows: records of one item and three zero words), the
descriptor's end over a lane count that is no multiple of 64, the second group's start behind the records and their fifth bytes, a
continuation packet whose record holds a single item (lists of 9 and 17), the sizes of the builder's scan (the exact-size second
attempt), and a launch over chunks of differing form.  -m gpu."""
import os

import numpy as np
import pytest

from oracle import oracle
from test_gpu_tall_items import _cell_with_lists_of_3_4_and_5, _from_triplets, _random_pairs

pytestmark = pytest.mark.gpu

SWITCHES = ("SLP_STRIP_MIN_NNZ", "SLP_TALL_R", "SLP_TALL_C", "SLP_TALL_RECORDS", "SLP_TALL_BUILD_ROOM")
POLICIES = ((0, 6), (1, 7))
FORMS = (("1", 1), ("0", 0), (None, None))   # SLP_TALL_RECORDS, the form it must give (None: the planner's -- the case says which)


@pytest.fixture(autouse=True)
def _small_matrices_take_the_tall_format():
    os.environ["SLP_STRIP_MIN_NNZ"] = "1"
    yield
    for name in SWITCHES:
        os.environ.pop(name, None)


def _force(form):
    if form is None:
        os.environ.pop("SLP_TALL_RECORDS", None)
    else:
        os.environ["SLP_TALL_RECORDS"] = form


def _reference(a_host):
    rng = np.random.RandomState(3)
    x, y = rng.randn(a_host.shape[1]), rng.randn(a_host.shape[0])
    oa = oracle.as_csr(a_host)
    return x, y, oracle.matvec(oa, x), oracle.rmatvec(oa, y)


def _check(a_host, rows_per_block, width, automatic, policies=POLICIES):
    """Both products of both value kinds in the three forms against the oracle (computed once); ``automatic``: the forms the planner
    must choose for the copy of A and of A^T, by policy.  Returns {(policy, form): (bytes of the copy of A, of A^T)}."""
    from pysparselp_amd.device import DeviceMatrix

    os.environ["SLP_TALL_R"], os.environ["SLP_TALL_C"] = str(rows_per_block), str(width)
    x, y, ax, aty = _reference(a_host)
    sizes = {}
    for policy, kernel in policies:
        for form, want in FORMS:
            _force(form)
            a = DeviceMatrix.from_csr(a_host)
            try:
                a.set_format(policy)
                assert a.spmv_kernel(False) == kernel and a.spmv_kernel(True) == kernel, (policy, form)
                rec = int(a._l.slp_matrix_tall_records(a._h, 0)), int(a._l.slp_matrix_tall_records(a._h, 1))
                print("shape", a_host.shape, "nnz", a_host.nnz, "policy", policy, "SLP_TALL_RECORDS", form, "records", rec)
                assert rec == (automatic[policy] if form is None else (want, want)), (policy, form, rec)
                assert int(a._l.slp_matrix_strip_width(a._h, 0)) == width and int(a._l.slp_matrix_tall_rows(a._h, 0)) == rows_per_block
                assert np.array_equal(a.matvec(x), ax), (policy, form)
                assert np.array_equal(a.rmatvec(y), aty), (policy, form)
                sizes[(policy, form)] = (int(a._l.slp_matrix_format_bytes(a._h, 0)), int(a._l.slp_matrix_format_bytes(a._h, 1)))
            finally:
                a.close()
    return sizes


def _two_cells_of_4000():
    """13 021 x 6 144 at 1e-4: ONE row block on two strips of 3 072 columns, about 4 000 items per cell -- the cell of the
    benchmark's LP (lists of four on most lanes, of three on the last ~100)."""
    rows, cols = _random_pairs(13021, 6144, 1e-4, 81)
    return _from_triplets(13021, 6144, rows, cols, 82)


def test_the_benchmarks_cell_takes_records_and_stays_below_the_csr():
    a = _two_cells_of_4000()
    assert 7900 < a.nnz <= 8000
    # the copy of A^T has the same entries in five cells of about 1 600 (6 144 rows on five strips): lists of one and two, slot-major;
    # fp64 items (policy 1) are never given records by the planner
    sizes = _check(a, 13021, 3072, automatic={0: (1, 0), 1: (0, 0)})
    for t in (0, 1):
        records, slot_major = sizes[(0, "1")][t], sizes[(0, "0")][t]
        print("copy of", "A^T" if t else "A", ": records", records, "bytes, slot-major", slot_major, "bytes, ratio %.4f" % (records / slot_major),
              "-- %.2f and %.2f bytes per entry" % (records / a.nnz, slot_major / a.nnz))
        assert sizes[(0, None)][t] == (slot_major if t else records)   # the planner's copy is the forced one of the same form
    records, slot_major = sizes[(0, None)][0], sizes[(0, "0")][0]
    assert slot_major < records < 12 * a.nnz          # records cost bytes, and still less than the CSR's 12 per entry


def test_lists_of_3_4_and_5_and_a_strip_of_700_single_entry_rows():
    """The one-block 4 096 x 8 192 cell of ``test_gpu_tall_items.py``: a slot 3 of 504 lanes (the records behind it carry a zero
    word), a fifth-item slot two lanes wide (the second group behind 5 w[0] words), and a second strip of 700 single-entry rows --
    700 records (no multiple of 64) of one item and three zero words.  2 138 items per cell on average: the planner stays slot-major
    (+ 62 %)."""
    _check(_cell_with_lists_of_3_4_and_5(), 4096, 4096, automatic={0: (0, 0), 1: (0, 0)})


def test_continuation_packets_whose_record_holds_one_item():
    """One cell of 2 048 x 4 096 with a row of 9 and a row of 17 entries: their lanes' second and third packets hold a record with a
    single item (and, in between, a full packet); the lanes beside them have none there."""
    rows, cols = _random_pairs(2048, 4096, 4e-4, 83)
    keep = [(r, c) for r, c in zip(rows, cols) if r not in (5, 9)]
    rng = np.random.RandomState(84)
    keep += [(5, int(c)) for c in rng.choice(4096, size=9, replace=False)]
    keep += [(9, int(c)) for c in rng.choice(4096, size=17, replace=False)]
    a = _from_triplets(2048, 4096, [r for r, _ in keep], [c for _, c in keep], 85)
    assert a[5].nnz == 9 and a[9].nnz == 17 and 3000 < a.nnz < 3600
    _check(a, 2048, 4096, automatic={0: (0, 0), 1: (0, 0)})   # (below 3 795 items per cell: + 16 % and more)


def test_small_cells_stay_slot_major_and_below_the_csr():
    """8 192 x 8 192 in blocks of 1 024 rows on strips of 4 096 columns: in either orientation 8 streams of two cells of about 140
    items in lists of one -- the cells of a finely chunked matrix, down-scaled: as records every item would take 20 bytes.  The
    planner keeps the compact form, at less than the CSR's 12 bytes per entry in both orientations (8 bytes per item and 512 bytes
    of directory per stream)."""
    rows, cols = _random_pairs(8192, 8192, 140 * 16 / (8192 * 8192), 86)
    a = _from_triplets(8192, 8192, rows, cols, 87, decimals=1)
    assert 2100 < a.nnz <= 2240
    sizes = _check(a, 1024, 4096, automatic={0: (0, 0), 1: (0, 0)})
    for t in (0, 1):
        print("copy of", "A^T" if t else "A", ": slot-major %.2f bytes per entry, records %.2f" % (sizes[(0, None)][t] / a.nnz, sizes[(0, "1")][t] / a.nnz))
        assert sizes[(0, None)][t] < 12 * a.nnz < sizes[(0, "1")][t]


@pytest.mark.parametrize("policy, kernel", POLICIES)
def test_three_chunks_follow_the_first_chunks_form_in_one_launch(policy, kernel):
    """Chunks of about 4 600 items per cell of the copy of A (lists of four and five: records cost nothing, the planner takes them).
    The switch is set for the FIRST chunk only and unset for the other two, which follow it through the carry against their own rule
    -- records for the copy of A^T and for fp64 items, slot-major for the copy of A -- or the composite could not run in one launch.
    A x: one grid over the row blocks of all chunks; A^T y: the column sums stay in LDS over three segments."""
    from pysparselp_amd.device import ChunkedDeviceMatrix, DeviceMatrix

    rows, cols = _random_pairs(6144, 8192, 0.55e-3, 71)
    rows += [7] * 30
    cols += list(100 + np.random.RandomState(72).choice(200, size=30, replace=False))
    a_host = _from_triplets(6144, 8192, rows, cols, 73)
    x, y, ax, aty = _reference(a_host)
    os.environ["SLP_TALL_R"], os.environ["SLP_TALL_C"] = "2048", "4096"
    cuts = [0, 2048, 4096 + 10, 6144]
    results = {}
    # (left to the planner: the copy of A has records; that of A^T -- 8 192 rows on ONE strip of a chunk's 2 048 columns, 2 300 items
    # per cell -- stays slot-major, in every chunk; fp64 items are never given records by the planner)
    for first, rest, want in (("1", None, (1, 1)),("0", None, (0, 0)), (None, None, (1, 0) if policy == 0 else (0, 0))):
        g = ChunkedDeviceMatrix(a_host.shape[1], expect_chunks=len(cuts) - 1)
        try:
            for k, (r0, r1) in enumerate(zip(cuts, cuts[1:])):
                _force(first if k == 0 else rest)
                ch = DeviceMatrix.from_csr(a_host[r0:r1])
                if policy:
                    ch.set_format(policy)
                g.append(ch)
            assert g.spmv_kernel(False) == kernel and g.spmv_kernel(True) == kernel
            # the first chunk's form -- and every chunk's: a composite whose parts differ in it keeps its chunk-by-chunk launches
            assert (int(g._l.slp_matrix_tall_records(g._h, 0)), int(g._l.slp_matrix_tall_records(g._h, 1))) == want, first
            assert int(g._l.slp_matrix_product_launches(g._h, 0)) == 1 and int(g._l.slp_matrix_product_launches(g._h, 1)) == 1, first
            results[first] = (g.matvec(x), g.rmatvec(y))
        finally:
            g.close()
    for first, (gx, gy) in results.items():
        assert np.array_equal(gx, ax) and np.array_equal(gy, aty), first
    assert np.array_equal(results["1"][0], results["0"][0]) and np.array_equal(results["1"][1], results["0"][1])


@pytest.mark.parametrize("policy, kernel", POLICIES)
def test_the_exact_size_second_attempt_writes_the_same_records(policy, kernel):
    """``SLP_TALL_BUILD_ROOM=0.5``: the single pass is given half of its estimate, some cell does not fit, and the pass is repeated
    into buffers of the sizes the scan found -- sizes that come from ``tall_packet_lane_words`` in records form."""
    from pysparselp_amd.device import DeviceMatrix

    a_host = _two_cells_of_4000()
    x, y, ax, aty = _reference(a_host)
    os.environ["SLP_TALL_R"], os.environ["SLP_TALL_C"], os.environ["SLP_TALL_RECORDS"] = "13021", "3072", "1"
    sizes = []
    for room in (None, "0.5"):
        if room:
            os.environ["SLP_TALL_BUILD_ROOM"] = room
        a = DeviceMatrix.from_csr(a_host)
        try:
            a.set_format(policy)
            assert a.spmv_kernel(False) == kernel and a.spmv_kernel(True) == kernel
            assert int(a._l.slp_matrix_tall_records(a._h, 0)) == 1 and int(a._l.slp_matrix_tall_records(a._h, 1)) == 1
            assert np.array_equal(a.matvec(x), ax) and np.array_equal(a.rmatvec(y), aty), room
            sizes.append((int(a._l.slp_matrix_format_bytes(a._h, 0)), int(a._l.slp_matrix_format_bytes(a._h, 1))))
        finally:
            a.close()
    print("bytes of the copies, first attempt and exact-size second attempt:", sizes)
    assert sizes[0] == sizes[1]
