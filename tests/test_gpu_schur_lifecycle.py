"""Who owns the scratch of a free-landmark handle, through the two paths no other test takes (``vinsat_amd/csrc/vba_schur_context.h``:
one scratch per feature, released by ``vba_schur_destroy`` and, for the queries, by ``vba_schur_enable_dynamics``).  Both on case
``"12"`` of tests/schur_dyn_cases.py, the smallest the suite has.  Everything is compared bit for bit: the launches of a trial do not
depend on what else the handle has allocated.
"""
import ctypes

import numpy as np
import pytest

import schur_dyn_cases as C

pytestmark = pytest.mark.gpu


def engine(d, dynamics=False):
    from vinsat_amd.schur import SchurBA
    kw = dict(time_idx=d["time_idx"], sigma_dyn=d["sigma_dyn"]) if dynamics else {}
    return SchurBA(d["states0"], d["X0"], d["uv"], d["w"], d["pose_of_row"], d["landmark_of_row"], d["intrinsics"], sigma_prior=d["sigma"], **kw)


def trial(e, d):
    """``(iterate tuple, states, landmarks)`` of one trial from the case's start."""
    e.set_state(d["states0"], d["Xs"])
    r = e.iterate(1e-3)
    return (r, *e.get_state())


def same_bits(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_dynamics_enabled_after_the_queries_have_allocated():
    """``SchurBA`` enables the factor in its constructor; here it comes after a covariance and a reliability query, so
    ``vba_schur_enable_dynamics`` has their scratch (sized for 6 n) to throw away."""
    from vinsat_amd._lib import VbaError
    d = C.case("12")
    ref = engine(d, dynamics=True)
    want = trial(ref, d)
    ref.close()
    assert want[0][2]                                   # an accepted trial: the state moved
    e = engine(d)
    e.set_state(d["states0"], d["Xs"])
    assert e.covariance(pairs=True)["info"] == 0 and e.reliability()["info"] == 0
    t = np.ascontiguousarray(d["time_idx"], dtype=np.int32)
    e._check(e.lib.vba_schur_enable_dynamics(e.h, t.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), float(d["sigma_dyn"])))
    e.dynamics = True                                   # (as the constructor sets it)
    got = trial(e, d)
    assert same_bits(got, want)
    for call in (e.covariance, e.reliability, e.snoop):
        with pytest.raises(VbaError, match="not available on a handle with the dynamics factor"):
            call()
    e.close()


def test_every_features_scratch_on_one_handle():
    """Covariance, reliability, snooping and re-weighting state all allocated on one handle: the trial after them is the trial of a
    handle that ran none of them, ``close`` releases all of it, and a handle made afterwards gives the same bits again."""
    d = C.case("12")
    fresh = engine(d)
    want = trial(fresh, d)
    fresh.close()
    e = engine(d)
    e.set_state(d["states0"], d["Xs"])
    assert e.covariance()["info"] == 0 and e.reliability()["info"] == 0
    s = e.snoop(crit=float("inf"))
    assert s["info"] == 0 and s["rows"] + s["landmarks"] == 0
    assert e.reweight(2.0)["status"] == 0               # alpha = 2 puts the uploaded weights back
    got = trial(e, d)
    e.close()
    assert same_bits(got, want)
    after = engine(d)
    again = trial(after, d)
    after.close()
    assert same_bits(again, want)
