"""What the batched and list benchmarks of this directory share."""
import numpy as np


def spread(v):
    """(max - min) / median of the repeats of one measurement."""
    v = np.asarray(v, dtype=np.float64)
    return float((v.max() - v.min()) / np.median(v)) if v.size > 1 else 0.0


def timed_between_events(lib, states, k, fill):
    """Milliseconds for `k` iterations of every dual-gradient-ascent state, one state after another, between two HIP events
    (slp_timer_start / _stop); `fill(state, k)` tops up each state's draws first, so that nothing is read back in between."""
    from pysparselp_amd import _lib

    for st in states:
        fill(st, k)
    ms = np.zeros(1)
    _lib.check(lib.slp_timer_start())
    for st in states:
        st.iterate(k, refill=False)
    _lib.check(lib.slp_timer_stop(_lib.ptr(ms)))
    return float(ms[0])
