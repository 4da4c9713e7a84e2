"""What test_gpu_cp_many_live.py and test_gpu_admm_many_live.py share: the walks that drive a compacted list state beside an
uncompacted one, written once over a ``kind`` -- an object that says how its solver makes a state, arms its test, reads its
records and iterates and what the CPU restatement expects (each test file defines its own).  Every comparison is exact: which
workgroup runs an LP changes no bit.  No test here; needs no GPU to import."""
import numpy as np

CALLS = (1, 1, 9, 40, 79, 20, 30, 20)   # iterate calls of the call-by-call walks: 200 iterations


def forms_of(st):
    """0 (lds) or 1 (global) per LP."""
    return np.array([st.FORMS.index(st.form(k)) for k in range(st.count)])


def assert_same(a, b, where=""):
    """Nested tuples and lists of arrays: the same types, dtypes and bits."""
    assert type(a) is type(b), (where, type(a), type(b))
    if isinstance(a, (tuple, list)):
        assert len(a) == len(b), where
        for i, (u, v) in enumerate(zip(a, b)):
            assert_same(u, v, f"{where}[{i}]")
        return
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (where, a.dtype, b.dtype, a.shape, b.shape)
    assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), where


def snapshot(kind, st):
    """The iterates, the records and the report of a state."""
    return tuple(kind.iterates(st)) + (tuple(kind.state(st)), st.report())


def assert_state(kind, got, want):
    """The records against the CPU restatement, in the columns that are exact in any order (``kind.exact``: the iterations, the
    flags and the maxima; the two sums of the certificate are compared with the uncompacted state's instead)."""
    for name, g, w in zip(kind.names, got, want):
        print(name, g, "expected", w)
    for c in kind.exact:
        assert np.array_equal(got[c], want[c], equal_nan=c > 1), kind.names[c]


def check_live(kind, st, forms):
    """``live_state`` against the flags read back: per form the count and ``flatnonzero``, lds first.  Returns it."""
    live, order, launched, cap = st.live_state()
    stopped = kind.state(st)[1]
    assert live.dtype == np.int64 and launched.dtype == np.int64 and cap.dtype == np.int64 and order.dtype == np.int32
    assert live.shape == launched.shape == cap.shape == (2,)
    want = [np.flatnonzero(~stopped & (forms == g)) for g in (0, 1)]
    assert np.array_equal(live, [len(w) for w in want]), (live, stopped, forms)
    assert np.array_equal(order, np.concatenate(want)), (order, want)
    return live, order, launched, cap


def on_and_off(kind, problems):
    """Two states of the same list, compaction on in the first; the forms and the group sizes."""
    on, off = kind.make(problems), kind.make(problems)
    on.set_compaction(True)
    forms = forms_of(on)
    assert np.array_equal(forms, forms_of(off))
    return on, off, forms, np.array([(forms == 0).sum(), (forms == 1).sum()])


def walk_on_against_off(kind, form, kmax, every):
    """Item 1: both states through CALLS, compared after every call; the grids of the compacted one follow the live counts."""
    want = kind.expected(kind.cases, every, sum(CALLS))
    assert want[1].sum() >= 3 and len(set(want[0][want[1]])) >= 3 and not want[1].all()   # the list the item asks for
    on, off, forms, sizes = on_and_off(kind, [kind.problem(c) for c in kind.cases])
    try:
        if form is not None:
            assert {on.form(k) for k in range(on.count)} == {form}
        for st in (on, off):
            kind.arm(st, every)
            assert np.array_equal(check_live(kind, st, forms)[2], [0, 0])   # nothing launched yet
        assert_same(snapshot(kind, on), snapshot(kind, off), "start")
        launched, shrunk = np.zeros(2, dtype=np.int64), False
        for i, k in enumerate(CALLS):
            before = check_live(kind, on, forms)[0]
            on.iterate(k)
            off.iterate(k)
            assert_same(snapshot(kind, on), snapshot(kind, off), f"call {i}")
            launched = np.where(before > 0, before, launched)   # a form without a live LP launches nothing
            got_on, got_off = check_live(kind, on, forms), check_live(kind, off, forms)
            print("call", i, "live before", before, "launched", got_on[2], "cap", got_on[3], "uncompacted", got_off[2], got_off[3])
            assert np.array_equal(got_on[2], launched)
            assert np.array_equal(got_off[2], sizes)
            ran = sizes > 0
            assert (got_on[3][ran] >= got_off[3][ran]).all() and (got_off[3][ran] >= 1).all()
            if kmax is not None:
                assert (got_on[3][ran] == kmax).all() and (got_off[3][ran] == kmax).all()
            shrunk = shrunk or bool((got_on[2] < sizes).any())
        assert shrunk   # the grid did shrink
        assert_state(kind, kind.state(on), want)
    finally:
        on.close()
        off.close()


def walk_both_forms(kind, cases, every=1, k=5, calls=60, more=2):
    """Item 2: an unforced list with LPs of both forms, in calls of ``k`` iterations.  Once every LP of one form has stopped
    while the other form goes on, the dead form launches nothing more and the other one stays bit for bit."""
    on, off, forms, sizes = on_and_off(kind, [kind.problem(c) for c in cases])
    try:
        assert (sizes > 0).all(), sizes
        for st in (on, off):
            kind.arm(st, every)
        dead, frozen, after = None, None, 0
        for i in range(calls):
            live = check_live(kind, on, forms)[0]
            if dead is None and (live == 0).sum() == 1:
                dead = int(np.flatnonzero(live == 0)[0])
                frozen = on.live_state()[2][dead]
                print("form", dead, "has no live LP before call", i, "its last grid", frozen)
            on.iterate(k)
            off.iterate(k)
            assert_same(snapshot(kind, on), snapshot(kind, off), f"call {i}")
            assert np.array_equal(check_live(kind, off, forms)[2], sizes)
            if dead is not None:
                now = check_live(kind, on, forms)
                assert now[2][dead] == frozen and now[2][1 - dead] == live[1 - dead] > 0
                after += 1
                if after == more:
                    break
        assert dead is not None and after == more   # one form ran out while the other one went on
    finally:
        on.close()
        off.close()


def walk_scan_edges(kind, rotation, count, every=10, calls=40):
    """Item 4: ``count`` LPs, the fixtures of ``rotation`` in turn, in calls of ``every`` iterations until all are stopped."""
    problems = [kind.problem(rotation[k % len(rotation)]) for k in range(count)]
    on = kind.make(problems)
    off = kind.make(problems) if count in (65, 1025) else None
    try:
        on.set_compaction(True)
        forms = forms_of(on)
        per = (count + 1023) // 1024                     # the LPs of one lane of the scan
        starts = np.arange(per, count, per)              # the first LP of every chunk but the first
        for st in (on, off):
            if st is not None:
                kind.arm(st, every, loose=True)
        straddled = False
        for i in range(calls):
            stopped = kind.state(on)[1]
            check_live(kind, on, forms)
            if stopped.all():
                break
            straddled = straddled or bool((stopped[starts - 1] & stopped[starts]).any())
            on.iterate(every)
            if off is not None:
                off.iterate(every)
        assert kind.state(on)[1].all(), "the list did not stop within the calls"
        if count > 1:
            assert straddled   # a call saw retired LPs on both sides of a boundary between two lanes' chunks, with LPs still live
        if off is not None:
            assert_same(snapshot(kind, on), snapshot(kind, off), "final")
        # all stopped: a further call launches nothing and changes nothing
        before, grid = snapshot(kind, on), on.live_state()[2]
        on.iterate(every)
        assert_same(snapshot(kind, on), before, "after the end")
        live, order, launched, _ = on.live_state()
        assert np.array_equal(live, [0, 0]) and order.size == 0 and np.array_equal(launched, grid)
    finally:
        on.close()
        if off is not None:
            off.close()


def walk_split_steps(kind, every, total):
    """Item 5: whole iterations made of the two half steps on an armed, compacted state stop where the restatement says."""
    want = kind.expected(kind.cases, every, total)
    assert want[1].any() and not want[1].all()
    on = kind.make([kind.problem(c) for c in kind.cases])
    try:
        on.set_compaction(True)
        forms = forms_of(on)
        sizes = np.array([(forms == 0).sum(), (forms == 1).sum()])
        kind.arm(on, every)
        first, second = kind.halves(on)
        for _ in range(total):
            first()
            second()
        assert_state(kind, kind.state(on), want)
        kind.assert_iterates(on, kind.cases, want[0])
        launched = check_live(kind, on, forms)[2]
        assert (launched <= sizes).all() and (launched < sizes).any()
    finally:
        on.close()


def walk_unarmed(kind):
    """Item 6: without a test armed a compacted state launches the whole list."""
    on, off, forms, sizes = on_and_off(kind, [kind.problem(c) for c in kind.cases])
    try:
        for k in (1, 12, 37):
            on.iterate(k)
            off.iterate(k)
            assert_same(snapshot(kind, on), snapshot(kind, off))
            assert np.array_equal(check_live(kind, on, forms)[2], sizes)
            assert np.array_equal(check_live(kind, on, forms)[0], sizes)
        first, second = kind.halves(on)
        other = kind.halves(off)
        for half in (first, other[0], second, other[1]):
            half()
        assert_same(snapshot(kind, on), snapshot(kind, off))
        assert np.array_equal(check_live(kind, on, forms)[2], sizes)
        assert np.array_equal(kind.state(on)[0], np.full(on.count, 51))
    finally:
        on.close()
        off.close()


def walk_rearm(kind, every=1, first=100, more=60):
    """Item 7: a new tolerance clears the flags: every LP is live again and the run goes on as the uncompacted one."""
    on, off, forms, sizes = on_and_off(kind, [kind.problem(c) for c in kind.cases])
    try:
        for st in (on, off):
            kind.arm(st, every, loose=True)
            st.iterate(first)
        iterations, stopped = kind.state(on)[:2]
        assert stopped.sum() >= 2
        assert (check_live(kind, on, forms)[0] < sizes).any()
        for st in (on, off):
            kind.arm(st, every, tight=True)
        live, order, _, _ = check_live(kind, on, forms)
        assert np.array_equal(live, sizes) and order.size == on.count and not kind.state(on)[1].any()
        for k in (1, more - 1):
            before = check_live(kind, on, forms)[0]
            on.iterate(k)
            off.iterate(k)
            assert_same(snapshot(kind, on), snapshot(kind, off))
            assert np.array_equal(on.live_state()[2], before)
            if k == 1:
                assert np.array_equal(before, sizes)   # the first call after the re-arming began with every LP live
        assert (kind.state(on)[0] > iterations)[stopped].all()   # the revived LPs went on
    finally:
        on.close()
        off.close()


def check_c_abi(kind, st, set_compaction, live_state, name):
    """Item 9: refusals with the function's name in front, NULL outputs, ``live_state`` before compaction was ever on, and no
    call changes a record.  ``st`` is armed and has run."""
    from pysparselp_amd import SlpError, _lib

    before = snapshot(kind, st)
    forms = forms_of(st)
    check_live(kind, st, forms)   # compaction was never on
    for bad in (2, -1, 7):
        with pytest_raises(SlpError, f"{name}_set_compaction: on must be 0 or 1"):
            _lib.check(set_compaction(st._h, bad))
    with pytest_raises(SlpError, f"{name}_set_compaction: NULL handle"):
        _lib.check(set_compaction(None, 1))
    with pytest_raises(SlpError, f"{name}_live_state: NULL handle"):
        _lib.check(live_state(None, None, None, None, None))
    _lib.check(live_state(st._h, None, None, None, None))
    live = np.zeros(2, dtype=np.int64)
    _lib.check(live_state(st._h, _lib.ptr(live), None, None, None))
    order = np.full(st.count, 77, dtype=np.int32)
    _lib.check(live_state(st._h, None, _lib.ptr(order), None, None))
    assert np.array_equal(order[:live.sum()], check_live(kind, st, forms)[1]) and (order[live.sum():] == -1).all()
    for on in (1, 1, 0, 1, 0):
        _lib.check(set_compaction(st._h, on))
        check_live(kind, st, forms)
    assert_same(snapshot(kind, st), before, "no call changes a record")


class pytest_raises:
    """``pytest.raises`` whose message has to START with ``text``."""

    def __init__(self, exc, text):
        self.exc, self.text = exc, text

    def __enter__(self):
        return self

    def __exit__(self, kind, value, tb):
        assert kind is not None and issubclass(kind, self.exc), f"{self.exc.__name__} not raised"
        assert str(value).startswith(self.text), (str(value), self.text)
        return True
