"""Which of the eleven query entries of the free-landmark mode serves which kind of handle, what a refusal says, in which order an
entry checks its arguments, and that a refused call leaves nothing behind -- on 12 / 150 (``schur_att_rel_cases.case("12")``: the
smallest case that carries ``time_idx`` and ``cumrot``) through the C entries themselves (``schur_query_harness.raw_query``).  The
entries share their bodies across the kinds of handle; this is what such sharing could change without changing a number.

The plain-named entries (``vba_schur_covariance``, ``_reliability``, ``_snoop``, ``_outlier_power``) check: null argument, the
dynamics refusal, ``lamda``, their other arguments, uploaded / state.  The ``_dyn`` and ``_att`` entries: null argument, ``lamda``,
their other arguments (snoop: ``crit``, then ``min_rows`` / ``min_track``; power: ``ncp``, then ``crit``), uploaded / state, the kind
of the handle.
"""
import ctypes

import numpy as np
import pytest

import schur_att_rel_cases as T
import schur_query_harness as H

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = 1, 4
NO_DYN, NO_ATT = "dynamics factor is not enabled", "attitude factor is not enabled"
FEATURE_MS = {"cov": "vba_schur_last_covariance_ms", "rel": "vba_schur_last_reliability_ms", "snoop": "vba_schur_last_snoop_ms",
              "power": "vba_schur_last_outlier_power_ms"}
HAS_DYN, HAS_ATT = " is not available on a handle with the dynamics factor", " is not available on a handle with the attitude factor"


def expected(entry, handle):
    """None if the entry serves a handle of this kind, else the text its refusal carries."""
    _, kind = H.ENTRIES[entry]
    if kind == "plain":
        return None if handle == "plain" else entry + HAS_DYN
    if handle == "plain":
        return NO_DYN
    if kind == "att":
        return None if handle == "att" else NO_ATT
    if handle == "att" and entry != "vba_schur_covariance_dyn":     # (the covariance query of a dynamics handle serves both)
        return entry + HAS_ATT
    return None


def refused(e, entry, code, text, **kw):
    rc = H.raw_query(e, entry, kw.pop("lam", 1e-3), **kw)[0]
    assert rc == code and text in H.last_error(e), (entry, rc, H.last_error(e))


def nothing_rejected(e):
    rows, lms, totals = np.full(e.m, 7, dtype=np.uint8), np.full(e.L, 7, dtype=np.uint8), (ctypes.c_int * 3)(7, 7, 7)
    assert e.lib.vba_schur_rejected(e.h, rows.ctypes.data_as(ctypes.c_void_p), lms.ctypes.data_as(ctypes.c_void_p), totals) == 0
    assert list(totals) == [0, 0, 0] and not rows.any() and not lms.any()


@pytest.mark.parametrize("handle", H.KINDS)
def test_serve_refuse_matrix_and_a_refusal_leaves_nothing_behind(handle):
    d = T.case("12")
    e, never = H.engine_of(handle, d), H.engine_of(handle, d)
    served = []
    for entry in H.ENTRIES:
        why = expected(entry, handle)
        if why is None:
            rc, info, *out = H.raw_query(e, entry, 1e-3)
            assert rc == 0 and info == 0, (entry, rc, info, H.last_error(e))
            if H.ENTRIES[entry][0] == "snoop":
                assert out[0] == [0, 0, 0] and out[1] == float("inf")
            else:
                assert all(np.any(b != 7.0) for b in out), entry
            served.append(entry)
        else:
            refused(e, entry, ESTATE, why)
            nothing_rejected(e)
    print(f"FIGURES query contract {handle}: served {served}")
    assert len(served) == {"plain": 4, "dyn": 4, "att": 4}[handle]
    nothing_rejected(e)
    assert e.iterate(1e-3) == never.iterate(1e-3)
    for a, b in zip(e.get_state(), never.get_state()):
        assert np.array_equal(a, b)
    e.close(), never.close()


@pytest.mark.parametrize("handle", H.KINDS)
def test_order_of_the_checks(handle):
    d = T.case("12")
    e = H.engine_of(handle, d)
    lib, s = e.lib, e.structure
    bare = ctypes.c_void_p()            # created, nothing uploaded: a handle of no kind yet
    assert lib.vba_schur_create(0, e.n, e.m, e.L, int(s["blk_i"].size), int(s["pair_k"].size), ctypes.byref(bare)) == 0
    for entry, (feature, kind) in H.ENTRIES.items():
        why = expected(entry, handle)
        # a null argument comes first on every handle, whatever else is wrong
        refused(e, entry, EINVAL, "null argument", lam=-1.0, info=False)
        refused(e, entry, EINVAL, "null argument", lam=-1.0, handle=False)
        if entry == "vba_schur_covariance_dyn":
            for on in ((False, True, True, True), (True, False, True, True)):
                refused(e, entry, EINVAL, "null argument", lam=-1.0, on=on)
        # a plain-named entry refuses the handle before it looks at lamda; the others look at lamda first
        if kind == "plain" and why is not None:
            refused(e, entry, ESTATE, why, lam=-1.0)
            refused(e, entry, ESTATE, why, lam=float("nan"), crit=-1.0, ncp=0.0, min_rows=-1)
        else:
            refused(e, entry, EINVAL, "lamda must be >= 0", lam=-1.0, crit=-1.0, ncp=0.0, min_rows=-1)
            refused(e, entry, EINVAL, "lamda must be >= 0", lam=float("nan"))
            if feature == "snoop":
                refused(e, entry, EINVAL, "crit must be >= 0", crit=-1.0, min_rows=-1)
                refused(e, entry, EINVAL, "min_rows and min_track must be >= 0", min_rows=-1)
                refused(e, entry, EINVAL, "min_rows and min_track must be >= 0", min_track=-1)
            if feature == "power":
                refused(e, entry, EINVAL, "ncp must be positive and finite", ncp=0.0, crit=0.0)
                refused(e, entry, EINVAL, "ncp must be positive and finite", ncp=float("inf"))
                refused(e, entry, EINVAL, "crit must be > 0", crit=0.0)
            if why is not None:         # ... and the kind of the handle behind the arguments
                refused(e, entry, ESTATE, why)
        # uploaded / state comes before the kind of the handle (a handle without the dynamics factor), behind the arguments
        h, e.h = e.h, bare
        try:
            refused(e, entry, ESTATE, "upload the problem and set the state first")
            refused(e, entry, EINVAL, "lamda must be >= 0", lam=-1.0)
        finally:
            e.h = h
    nothing_rejected(e)
    assert lib.vba_schur_destroy(bare) == 0
    e.close()


def test_last_ms_getters_check_their_arguments_and_read_their_feature():
    d = T.case("12")
    e = H.engine_of("att", d)
    getters = {"vba_schur_last_covariance_ms": "cov", "vba_schur_last_covariance_dyn_ms": "cov"}
    getters.update({f"vba_schur_last_{name}{sfx}_ms": f for f, name in (("rel", "reliability"), ("snoop", "snoop"), ("power", "outlier_power"))
                    for sfx in ("", "_dyn", "_att")})
    assert len(getters) == 11
    ms = ctypes.c_float(-1.0)
    for name in getters:
        fn = getattr(e.lib, name)
        assert fn(None, ctypes.byref(ms)) == EINVAL and fn(e.h, None) == EINVAL and "null argument" in H.last_error(e)
        assert fn(e.h, ctypes.byref(ms)) == 0 and ms.value == 0.0           # nothing has run yet
    read = lambda name: (getattr(e.lib, name)(e.h, ctypes.byref(ms)), ms.value)[1]
    for entry, feature in (("vba_schur_covariance_dyn", "cov"), ("vba_schur_reliability_att", "rel"), ("vba_schur_snoop_att", "snoop"),
                           ("vba_schur_outlier_power_att", "power")):
        before = {name: read(name) for name in getters}
        assert H.raw_query(e, entry, 1e-3)[:2] == (0, 0)
        after = {name: read(name) for name in getters}
        for name, f in getters.items():     # the getters of one feature read one figure; a query leaves the other features' alone
            if f == feature:
                assert after[name] > 0.0 and after[name] == after[FEATURE_MS[feature]], (entry, name)
            else:
                assert after[name] == before[name], (entry, name)
    e.close()
