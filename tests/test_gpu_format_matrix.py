"""Every product format x every way the solvers use it, against the oracle.  -m gpu.

``slp_matrix_spmv_kernel`` codes (one per orientation): 0 CSR walk, 1 fp64 LDS strips, 2 dictionary pairs, 3 dictionary quads,
4 wide strips with a dictionary, 5 wide strips with fp64 values, 6 tall cells with a dictionary, 7 tall cells with fp64 values.
Every case reaches its format through the switches the suite already uses (SLP_STRIP_MIN_NNZ, SLP_VALUE_DICT, SLP_DICT_VARIANT,
SLP_TALL, SLP_STRIP_SPLIT, SLP_TALL_SPLIT) and asserts the codes it meant to reach in both orientations.

Shapes (random LPs of the device generator, values rounded to 0.01, so a value dictionary exists unless switched off):
  STRIPS 14 000 x 30 000 at 1e-3 (4.2e5 entries): codes 0 (default entry threshold), 1, 2, 3;
  WIDE   300 000 x 300 000 at 2.5e-5 (2.25e6 entries, 2.5 entries per row and 131 072-column strip, SLP_TALL=0): codes 4, 5;
  TALL   40 000 x 200 000 at 2.5e-4 (2e6 entries, ~1 entry per row and 4096-column cell in both orientations): codes 6, 7.

Variants: ``plain``; ``chunked`` -- a composite of row chunks NOT cut at m_eq (two chunks; one chunk for WIDE, whose columns
orientation needs more than 2 x 131 072 rows per chunk: a chunk of the whole matrix, CSR released); ``cut`` -- two chunks cut at
m_eq (TALL: the equality chunk is still tall both ways); ``released`` -- ``release_csr`` after the copies are built; ``S2`` / ``S4``
-- strip-range splits (SLP_STRIP_SPLIT on codes 1-5, SLP_TALL_SPLIT=2 on 6/7; a wide copy has 3 strips, so S4 is not run there).

Which test covers which cell (format code x operation):
  test_products                  A x, A^T y in ORDER_SEQUENTIAL bit for bit: all codes, all variants; ORDER_AUTO of S2/S4 and
                                 ORDER_TREE on code 0 within the per-row bound below.
  test_abs_pow_products          |A|^p x and (|A|^p)^T y, p in {0, 0.5, 1, 2} bit for bit, p = 1.5 within the row bound: codes 1-7,
                                 all variants (S2/S4: every p within the row bound).
  test_two_vector_pass           matvec2 (strip_spmv2: ADMM-CG cg_rows2 / cg_cols2): both outputs bit for bit two single products on
                                 the same copy, both orientations, x1 != x0; S == 1 also bit for bit the oracle: codes 0-7, all
                                 variants (composites: the accum path of chunked / cut).
  test_chambolle_pock            T and Sigma (alpha = 1 bit for bit, alpha = 0.5 within the row bound), split_form(), and x after 8
                                 iterations bit for bit: codes 0-7 x {plain, chunked, cut, released} x m_eq in {0, m/10, m/10 + 1}
                                 (cut: m/10).  The code-5 rows are the regression for the fp64 wide strips that could not raise
                                 their entries to a power (mixed rows, released CSR, chunked); the WIDE rows also pin the signed
                                 zero of the clip np.minimum(np.maximum(x2, lb), ub) where lb = -0.0, ub = +0.0.
  test_matrix_free_admm          matrix-free ADMM with m_eq = m/10 <= 1e-9 against oracle.lp_admm_cg: codes 0-7.

Per-row bound (where bit-exactness is not the contract): ``|dev_i - oracle_i| <= 2 gamma(k_i + 2) (|A||x|)_i``
(``oracle.row_error_bound``), rows without entries +0.0 bit for bit."""
import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

STRIPS = dict(name="strips", m=14_000, n=30_000, density=1e-3, seed=4)
WIDE = dict(name="wide", m=300_000, n=300_000, density=2.5e-5, seed=3)
TALL = dict(name="tall", m=40_000, n=200_000, density=2.5e-4, seed=5)

SWITCHES = ("SLP_STRIP_MIN_NNZ", "SLP_VALUE_DICT", "SLP_DICT_VARIANT", "SLP_TALL", "SLP_TALL_R", "SLP_STRIP_SPLIT", "SLP_TALL_SPLIT",
            "SLP_CP_SPLIT")

# format: (shape, switches, kernel code in both orientations)
FORMATS = {
    "csr": (STRIPS, {}, 0),
    "fp64": (STRIPS, {"SLP_STRIP_MIN_NNZ": "1", "SLP_VALUE_DICT": "0"}, 1),
    "pairs": (STRIPS, {"SLP_STRIP_MIN_NNZ": "1", "SLP_VALUE_DICT": "1", "SLP_DICT_VARIANT": "1"}, 2),
    "quads": (STRIPS, {"SLP_STRIP_MIN_NNZ": "1", "SLP_VALUE_DICT": "1", "SLP_DICT_VARIANT": "2"}, 3),
    "wide_dict": (WIDE, {"SLP_STRIP_MIN_NNZ": "1", "SLP_VALUE_DICT": "1", "SLP_TALL": "0"}, 4),
    "wide_fp64": (WIDE, {"SLP_STRIP_MIN_NNZ": "1", "SLP_VALUE_DICT": "0", "SLP_TALL": "0"}, 5),
    "tall_dict": (TALL, {"SLP_STRIP_MIN_NNZ": "1", "SLP_VALUE_DICT": "1"}, 6),
    "tall_fp64": (TALL, {"SLP_STRIP_MIN_NNZ": "1", "SLP_VALUE_DICT": "0"}, 7),
}
VARIANTS = {
    "csr": ("plain",),
    "fp64": ("plain", "chunked", "released", "S2", "S4"),
    "pairs": ("plain", "chunked", "released", "S2", "S4"),
    "quads": ("plain", "chunked", "released", "S2", "S4"),
    "wide_dict": ("plain", "chunked", "released", "S2"),
    "wide_fp64": ("plain", "chunked", "released", "S2"),
    "tall_dict": ("plain", "chunked", "cut", "released", "S2"),
    "tall_fp64": ("plain", "chunked", "cut", "released", "S2"),
}
CASES = [(f, v) for f in FORMATS for v in VARIANTS[f]]
SEQUENTIAL_CASES = [(f, v) for f, v in CASES if not v.startswith("S")]


def bits_equal(a, b):
    """Bit-for-bit equality of two float64 arrays (-0.0 and +0.0 differ, NaNs compare by payload)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))


def assert_rows_within(got, a, x, ref, k_extra=2):
    """Per-row bound of re-associated products (``oracle.row_error_bound``); empty rows +0.0 bit for bit."""
    bound = oracle.row_error_bound(a, x, k_extra)
    empty = np.diff(a.indptr) == 0
    assert bits_equal(got[empty], np.zeros(int(empty.sum())))
    err = np.abs(got - ref)
    bad = np.flatnonzero(~(err <= bound))
    assert bad.size == 0, f"{bad.size} rows over the bound, e.g. row {bad[0]}: {err[bad[0]]} > {bound[bad[0]]}"


_HOST = {}


def _host(shape):
    """Host CSR of A and of A^T (oracle form) for a shape, and |A|^p of both on demand (cached)."""
    from pysparselp_amd.device import DeviceMatrix

    key = shape["name"]
    if key not in _HOST:
        d = DeviceMatrix.random(shape["m"], shape["n"], shape["density"], shape["seed"])
        s = d.download()
        d.close()
        _HOST[key] = dict(s=s, a=oracle.as_csr(s), at=oracle.as_csr(s.T.tocsr()), pow={}, lp={}, cp={}, admm=None)
    return _HOST[key]


def _powered(h, p, transposed):
    key = (p, transposed)
    if key not in h["pow"]:
        c = h["at" if transposed else "a"]
        h["pow"][key] = oracle.Csr(c.indptr, c.indices, np.abs(c.data) ** p, c.shape)
    return h["pow"][key]


def _lp(shape, m_eq):
    """(c, lb, ub, b) of the generator's LP with ``m_eq`` equality rows (randomLP.py:62-68), cached."""
    from pysparselp_amd.device import DeviceMatrix

    h = _host(shape)
    if m_eq not in h["lp"]:
        d = DeviceMatrix.random(shape["m"], shape["n"], shape["density"], shape["seed"])
        xf, c, lb, ub, b = d.random_lp_vectors(shape["density"], shape["seed"], m_eq=m_eq)
        d.close()
        h["lp"][m_eq] = (c, lb, ub, b)
    return h["lp"][m_eq]


def _matrix(monkeypatch, fmt, variant, m_eq=0):
    """The case's DeviceMatrix, its kernel codes checked in both orientations."""
    from pysparselp_amd.device import ChunkedDeviceMatrix, DeviceMatrix

    shape, switches, code = FORMATS[fmt]
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    if variant in ("S2", "S4"):
        monkeypatch.setenv("SLP_TALL_SPLIT" if code in (6, 7) else "SLP_STRIP_SPLIT", variant[1])
    m, n, dens, seed = shape["m"], shape["n"], shape["density"], shape["seed"]
    if variant in ("chunked", "cut"):
        if variant == "cut":
            assert m_eq % 2 == 0
            cuts = ChunkedDeviceMatrix.cuts(m, 2, cut_at=m_eq)
        else:
            cuts = [0, m] if shape is WIDE else ChunkedDeviceMatrix.cuts(m, 2)
            assert m_eq not in cuts[1:-1]
        a = ChunkedDeviceMatrix(n, expect_chunks=len(cuts) - 1, expect_rows=m)
        for r0, r1 in zip(cuts, cuts[1:]):
            a.append(DeviceMatrix.random(r1 - r0, n, dens, seed, r0))
        assert a.chunks == len(cuts) - 1
    else:
        a = DeviceMatrix.random(m, n, dens, seed)
    assert (a.spmv_kernel(False), a.spmv_kernel(True)) == (code, code), (fmt, variant)
    if variant == "released":
        a.release_csr()
    return a


def _vectors(shape, seed=1):
    rng = np.random.RandomState(seed)
    x0, y0 = rng.randn(shape["n"]), rng.randn(shape["m"])
    x1, y1 = 1e3 * rng.randn(shape["n"]), 1e3 * rng.randn(shape["m"])  # other magnitudes: swapped outputs show
    return x0, x1, y0, y1


@pytest.mark.parametrize("fmt, variant", CASES)
def test_products(monkeypatch, fmt, variant):
    from pysparselp_amd._lib import ORDER_AUTO, ORDER_SEQUENTIAL, ORDER_TREE

    shape = FORMATS[fmt][0]
    h = _host(shape)
    x, _, y, _ = _vectors(shape)
    ax, aty = oracle.matvec(h["a"], x), oracle.rmatvec(h["a"], y)
    a = _matrix(monkeypatch, fmt, variant)
    try:
        assert bits_equal(a.matvec(x, ORDER_SEQUENTIAL), ax)
        assert bits_equal(a.rmatvec(y, ORDER_SEQUENTIAL), aty)
        if variant.startswith("S"):
            assert_rows_within(a.matvec(x, ORDER_AUTO), h["a"], x, ax)
            assert_rows_within(a.rmatvec(y, ORDER_AUTO), h["at"], y, aty)
        if fmt == "csr":
            assert_rows_within(a.matvec(x, ORDER_TREE), h["a"], x, ax)
            assert_rows_within(a.rmatvec(y, ORDER_TREE), h["at"], y, aty)
    finally:
        a.close()


@pytest.mark.parametrize("fmt, variant", [c for c in CASES if c[0] != "csr"])
def test_abs_pow_products(monkeypatch, fmt, variant):
    shape = FORMATS[fmt][0]
    h = _host(shape)
    x, _, y, _ = _vectors(shape, seed=2)
    a = _matrix(monkeypatch, fmt, variant)
    split = variant.startswith("S")
    try:
        for p in (0.0, 0.5, 1.0, 2.0, 1.5):
            for transposed, v in ((False, x), (True, y)):
                pa = _powered(h, p, transposed)
                got, ref = a.abs_pow_matvec(v, p, transposed=transposed), oracle.matvec(pa, v)
                if p == 1.5 or split:
                    assert_rows_within(got, pa, v, ref)
                else:
                    assert bits_equal(got, ref), (p, transposed)
    finally:
        a.close()


@pytest.mark.parametrize("fmt, variant", CASES)
def test_two_vector_pass(monkeypatch, fmt, variant):
    shape = FORMATS[fmt][0]
    h = _host(shape)
    x0, x1, y0, y1 = _vectors(shape, seed=3)
    a = _matrix(monkeypatch, fmt, variant)
    exact = not variant.startswith("S") and fmt != "csr"   # (ORDER_AUTO on the CSR walk of these rows is the TREE order)
    try:
        for transposed, v0, v1 in ((False, x0, x1), (True, y0, y1)):
            w0, w1 = a.matvec2(v0, v1, transposed=transposed)
            one = a.rmatvec if transposed else a.matvec
            assert bits_equal(w0, one(v0)) and bits_equal(w1, one(v1)), transposed
            mat = h["at" if transposed else "a"]
            r0, r1 = oracle.matvec(mat, v0), oracle.matvec(mat, v1)
            if exact:
                assert bits_equal(w0, r0) and bits_equal(w1, r1), transposed
            else:
                assert_rows_within(w0, mat, v0, r0)
                assert_rows_within(w1, mat, v1, r1)
    finally:
        a.close()


def _expected_form(fmt, variant, m_eq):
    """slp_cp_split_form of the case (DeviceCP.split_form): 0 one kind of rows / the CSR walk forming both sums, 1 two copies
    (chunks cut at m_eq, or row-range copies of the solver's own: even m_eq, both ranges large enough for a copy -- not WIDE's
    equality rows, 30 000 columns of A_e^T), 2 masked products over the whole K^T copy."""
    shape, _, code = FORMATS[fmt]
    if m_eq == 0:
        return 0
    if variant == "cut":
        return 1
    if variant in ("chunked", "released"):
        return 2
    if code == 0:
        return 0
    return 2 if (m_eq % 2 or shape is WIDE) else 1


def _cp_cases():
    out = []
    for fmt, variant in SEQUENTIAL_CASES:
        m = FORMATS[fmt][0]["m"]
        for m_eq in ((m // 10,) if variant == "cut" else (0, m // 10, m // 10 + 1)):
            out.append((fmt, variant, m_eq))
    return out


def _cp_reference(shape, m_eq, alpha, iters):
    h = _host(shape)
    key = (m_eq, alpha, iters)
    if key not in h["cp"]:
        c, lb, ub, b = _lp(shape, m_eq)
        s = h["s"]
        ae, ai = (oracle.as_csr(s[:m_eq]), oracle.as_csr(s[m_eq:])) if m_eq else (None, h["a"])
        t, se, si = oracle.cp_setup(ae, ai, alpha)
        sig = np.concatenate((se, si)) if m_eq else si
        x = None
        if iters:
            x, _ = oracle.chambolle_pock_ppd(c, ae, b[:m_eq] if m_eq else None, ai, None, b[m_eq:], lb, ub, alpha=alpha,
                                             nb_max_iter=iters, nb_iter_plot=10 ** 9)
        h["cp"][key] = (t, sig, x)
    return h["cp"][key]


@pytest.mark.parametrize("fmt, variant, m_eq", _cp_cases())
def test_chambolle_pock(monkeypatch, fmt, variant, m_eq):
    from pysparselp_amd import _lib
    from pysparselp_amd._lib import ORDER_AUTO, ORDER_SEQUENTIAL
    from pysparselp_amd.scale import DeviceCP

    shape = FORMATS[fmt][0]
    h = _host(shape)
    c, lb, ub, b = _lp(shape, m_eq)
    iters = 8
    a = _matrix(monkeypatch, fmt, variant, m_eq)
    try:
        for alpha in (1.0, 0.5):
            t_ref, sig_ref, x_ref = _cp_reference(shape, m_eq, alpha, iters if alpha == 1.0 else 0)
            # (code 0: ORDER_AUTO walks rows longer than 16 entries in TREE order; the CSR walk is the sequential chain on request)
            cp = DeviceCP(a, b, c, lb, ub, alpha=alpha, m_eq=m_eq, order=ORDER_SEQUENTIAL if fmt == "csr" else ORDER_AUTO)
            try:
                assert cp.split_form() == _expected_form(fmt, variant, m_eq)
                t, sig = np.empty(shape["n"]), np.empty(shape["m"])
                _lib.check(cp._l.slp_cp_get_preconditioners(cp._h, _lib.ptr(t), _lib.ptr(sig)))
                if alpha == 1.0:
                    assert bits_equal(t, t_ref) and bits_equal(sig, sig_ref)
                    cp.iterate(iters)
                    x = cp.x()
                    assert bits_equal(x, x_ref), float(np.max(np.abs(x - x_ref)))
                else:
                    # T: sums of |v|^1.5 (pow: an ulp apart between libm and ocml) -- per column the row bound of the sum (one
                    # more addition for (0 + s_eq) + s_ineq), then a rounding of 1 / s on each side
                    k = np.diff(h["at"].indptr).astype(np.float64) + 3
                    u = 2.0 ** -53
                    rel = 2 * (k * u / (1 - k * u)) + 2 * u
                    assert np.all(np.abs(t - t_ref) <= rel * np.abs(t_ref))
                    assert bits_equal(t[k == 3], t_ref[k == 3])          # empty columns: T = 1
                    assert bits_equal(sig, sig_ref)                      # |v|^0.5: a square root on both sides, exact
            finally:
                cp.close()
    finally:
        a.close()


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_matrix_free_admm_with_equality_rows(monkeypatch, fmt):
    from pysparselp_amd.admm_cg import DeviceADMM

    shape = FORMATS[fmt][0]
    h = _host(shape)
    m_eq = shape["m"] // 10
    c, lb, ub, b = _lp(shape, m_eq)
    iters = 6
    if h["admm"] is None:
        s = h["s"]
        h["admm"] = oracle.lp_admm_cg(c, oracle.as_csr(s[:m_eq]), b[:m_eq], oracle.as_csr(s[m_eq:]), None, b[m_eq:], lb, ub,
                                      nb_iter=iters - 1, nb_iter_plot=10 ** 9)
    want = h["admm"]
    a = _matrix(monkeypatch, fmt, "plain")
    try:
        s = DeviceADMM(a, b, c, lb, ub, m_eq=m_eq)
        try:
            s.iterate(iters)
            got = s.x(shape["n"])
        finally:
            s.close()
        err = float(np.max(np.abs(got - want) / (1 + np.abs(want))))
        assert err <= 1e-9, err
    finally:
        a.close()
