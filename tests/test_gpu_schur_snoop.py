"""``vba_schur_snoop`` / ``SchurBA.snoop`` on the GPU.

The rule: masks, counts and ``crit_used`` of the device equal the NumPy rule of tests/schur_snoop_oracle.py applied to the device's
OWN ``reliability()`` output at that state (the tests themselves are held against the CPU reference by tests/test_gpu_schur_rel.py).
The promise: after a snoop the handle gives, bit for bit, what a fresh handle gives that was built with those rows' weights zeroed
and the same state; after ``restore_rejected`` the bits of a handle that never snooped.  The planted window is chosen and vetted on
the CPU (tests/schur_snoop_cases.py, tests/test_schur_snoop_host.py).  Every test needs the entry points and fails where they do
not exist.
"""
import ctypes

import numpy as np
import pytest

import schur_cases as C
import schur_query_harness as H
import schur_rel_cases as R
import schur_snoop_cases as SC
import schur_snoop_oracle as SO

pytestmark = pytest.mark.gpu
REL_OUTPUTS = ("leverage", "wtest", "lm_leverage", "lm_wtest", "lm_stats", "pose_stats")
CASES = (("12", 0.0), ("12", 1e-3), ("43", 1e-3), ("pose_without_rows", 1e-3), ("more_landmarks_than_rows", 1e-3),
         ("more_poses_than_landmarks", 1e-3), ("zero_weights", 1e-3))


def _open(name=None, d=None, state=None, w=None):
    d = R.problem(name) if d is None else d
    return d, H.engine(d, state=state, w=w)


def _shaken(d):
    """The case's start with 30 % of the landmarks moved off by 2 sigma per axis (seeded): at the fixtures' own start every
    ``lm_wtest`` is far below the row tests and no catalogue entry would ever win its group."""
    rng = np.random.default_rng(77)
    X = d["Xs"].copy()
    pick = rng.random(X.shape[0]) < 0.3
    X[pick] += rng.normal(0.0, 2.0 * d["sigma"], (int(pick.sum()), 3))
    return d["states0"], X


_same_rel = H._same(REL_OUTPUTS)


def _same_cov(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in ((a["pose"], b["pose"]), (a["landmark"], b["landmark"]), (a["pairs"][2], b["pairs"][2])))


def _weights(e, d):
    rows, _ = e.rejected()
    return np.where(rows, 0.0, d["w"])


def _crit90(rel, w, scaled=True):
    """About the 90th percentile of the finite tests, in the units ``snoop`` takes (divided by s0 with ``scaled``)."""
    t = np.concatenate([rel["wtest"][w > 0.0], rel["lm_wtest"]])
    q = float(np.percentile(t[np.isfinite(t)], 90))
    return q / float(np.sqrt(rel["fit"]["s0sq"])) if scaled else q


def _snoop_against_the_rule(e, d, rel, lam, crit, scaled, min_rows, min_track, label):
    """One device call from a handle without rejections against the rule at the device's own tests; the handle is restored."""
    want = SO.select_from(rel, d, crit, scaled, min_rows, min_track)
    got = e.snoop(lam, crit, scaled, min_rows, min_track)
    rows, lms = e.rejected()
    print(f"FIGURES schur snoop {label} lam={lam:g} crit={crit:.4g} scaled={scaled} min_rows={min_rows} min_track={min_track}: device "
          f"{(got['rows'], got['landmarks'], got['rows_via_landmarks'])} rule {want['counts']} crit_used {got['crit_used']!r} margin {want['margin']:.2e}")
    assert got["info"] == 0 and (got["rows"], got["landmarks"], got["rows_via_landmarks"]) == want["counts"]
    assert np.array_equal(rows, want["rows"] | want["via"]) and np.array_equal(lms, want["landmarks"])
    assert got["crit_used"] == want["crit_used"]
    if scaled:
        assert got["crit_used"] == crit * np.sqrt(rel["fit"]["s0sq"])              # bitwise: one correctly rounded root, one product
    e.restore_rejected()
    rows, lms = e.rejected()
    assert not rows.any() and not lms.any()
    return want


@pytest.mark.parametrize("name,lam", CASES)
def test_device_follows_the_rule_at_its_own_tests(name, lam):
    d = R.problem(name)
    _, e = _open(d=d, state=_shaken(d))
    rel = e.reliability(lam)
    crit = _crit90(rel, d["w"])
    cnt = np.bincount(d["pose_of_row"][d["w"] > 0.0], minlength=e.n)
    first = _snoop_against_the_rule(e, d, rel, lam, crit, True, 6, 3, name)
    assert first["counts"][0] > 0 and (first["counts"][1] > 0 or name not in ("43", "more_landmarks_than_rows"))
    _snoop_against_the_rule(e, d, rel, lam, 0.5 * crit, True, 6, 3, f"{name} half the critical value")
    assert _same_rel(rel, e.reliability(lam))                           # restored: the query reads as before
    _snoop_against_the_rule(e, d, rel, lam, crit * float(np.sqrt(rel["fit"]["s0sq"])), False, 6, 3, name)
    # min_rows at the exact count of a pose that rejected a row (keeps it), and one below (rejects it)
    i = int(d["pose_of_row"][np.nonzero(first["rows"])[0][0]])
    c_lm = int((first["marked"][d["landmark_of_row"]] & (d["pose_of_row"] == i) & (d["w"] > 0.0)).sum())
    at = _snoop_against_the_rule(e, d, rel, lam, crit, True, int(cnt[i]) - c_lm, 3, f"{name} pose {i} at its count")
    below = _snoop_against_the_rule(e, d, rel, lam, crit, True, int(cnt[i]) - c_lm - 1, 3, f"{name} pose {i} one below")
    assert not at["rows"][d["pose_of_row"] == i].any() and below["rows"][d["pose_of_row"] == i].sum() == 1
    # min_track at the edges of the tracks there are
    for mt in (0, 1, int(np.bincount(d["landmark_of_row"]).max()), int(np.bincount(d["landmark_of_row"]).max()) + 1):
        _snoop_against_the_rule(e, d, rel, lam, crit, True, 2, mt, f"{name} min_track")
    assert e.last_snoop_ms() > 0.0
    e.close()


@pytest.mark.parametrize("mode", ["0", "1", "2"])
def test_handle_behaves_as_a_fresh_one_with_those_weights_zeroed(mode, monkeypatch):
    monkeypatch.setenv("VBA_SCHUR_CLASSIC", mode)                       # read in vba_schur_create
    d = R.problem("43")
    _, e = _open(d=d, state=_shaken(d))
    rel0 = e.reliability(1e-3)
    crit = _crit90(rel0, d["w"])
    got = e.snoop(1e-3, crit, True, 6, 3)
    assert got["rows"] > 0 and got["landmarks"] > 0
    rows1, lms1 = e.rejected()
    assert rows1.sum() == got["rows"] + got["rows_via_landmarks"] and lms1.sum() == got["landmarks"]
    _, f = _open(d=d, state=_shaken(d), w=np.where(rows1, 0.0, d["w"]))
    for lam in (0.0, 1e-3):
        assert _same_cov(e.covariance(lam, pairs=True), f.covariance(lam, pairs=True))
        assert _same_rel(e.reliability(lam), f.reliability(lam))
    assert e.iterate(1e-3) == f.iterate(1e-3) and e.iterate(1e-4) == f.iterate(1e-4)
    assert all(np.array_equal(a, b) for a, b in zip(e.get_state(), f.get_state()))
    assert _same_cov(e.covariance(0.0, pairs=True), f.covariance(0.0, pairs=True))
    # a second snoop, at the new state, accumulates: the rule at the device's tests with the weights as they stand
    rel = e.reliability(1e-3)
    w_now = _weights(e, d)
    want = SO.select_from(rel, d, _crit90(rel, w_now), True, 6, 3, w=w_now)
    got2 = e.snoop(1e-3, _crit90(rel, w_now), True, 6, 3)
    rows2, lms2 = e.rejected()
    assert (got2["rows"], got2["landmarks"], got2["rows_via_landmarks"]) == want["counts"] and got2["rows"] > 0
    assert np.array_equal(rows2, rows1 | want["rows"] | want["via"]) and np.array_equal(lms2, lms1 | want["landmarks"])
    totals = (ctypes.c_int * 3)()
    assert e.lib.vba_schur_rejected(e.h, None, None, totals) == 0
    assert list(totals) == [got["rows"] + got2["rows"], got["landmarks"] + got2["landmarks"], got["rows_via_landmarks"] + got2["rows_via_landmarks"]]
    # restored: the bits of a handle that never snooped, at this state
    e.restore_rejected()
    _, g = _open("43", state=e.get_state())
    assert _same_rel(e.reliability(0.0), g.reliability(0.0)) and _same_cov(e.covariance(1e-3, pairs=True), g.covariance(1e-3, pairs=True))
    assert e.iterate(1e-5) == g.iterate(1e-5) and all(np.array_equal(a, b) for a, b in zip(e.get_state(), g.get_state()))
    for h in (e, f, g):
        h.close()


def test_upload_starts_clean():
    d, e = _open("12")
    rel = e.reliability(1e-3)
    assert e.snoop(1e-3, _crit90(rel, d["w"]), True, 6, 3)["rows"] > 0 and e.rejected()[0].any()
    _, f = _open("12")                                                  # a new handle: nothing rejected
    assert not f.rejected()[0].any() and not f.rejected()[1].any() and f.last_snoop_ms() == 0.0
    f.restore_rejected()                                                # a no-op on a handle that never snooped
    # the same handle uploaded again: masks and totals cleared, the weights are the uploaded ones
    s, p = e.structure, lambda a: a.ctypes.data_as(ctypes.c_void_p)
    uv = np.asarray(d["uv"], dtype=np.float64)[e.order]
    u, v, w = np.ascontiguousarray(uv[:, 0]), np.ascontiguousarray(uv[:, 1]), np.ascontiguousarray(d["w"][e.order])
    K, X0 = np.ascontiguousarray(d["intrinsics"], dtype=np.float64), np.ascontiguousarray(d["X0"], dtype=np.float64)
    e._check(e.lib.vba_schur_upload(e.h, p(s["lm_ptr"]), p(s["row_pose"]), p(s["row_lm"]), p(u), p(v), p(w), p(s["pose_ptr"]), p(s["pose_rows"]),
                                    p(s["blk_i"]), p(s["blk_j"]), p(s["blk_ptr"]), p(s["pair_k"]), p(s["pair_k2"]), p(K), p(X0), float(d["sigma"])))
    totals = (ctypes.c_int * 3)(7, 7, 7)
    assert e.lib.vba_schur_rejected(e.h, None, None, totals) == 0 and list(totals) == [0, 0, 0]
    assert not e.rejected()[0].any() and not e.rejected()[1].any()
    assert _same_rel(e.reliability(1e-3), rel) and _same_rel(f.reliability(1e-3), rel)
    e.close()
    f.close()


def _snapshot(e):
    st, X = e.get_state()
    dc, dl = e.last_step()
    ms = e.last_ms()
    return [st, X, dc.copy(), dl.copy(), e.cholesky_factor(),
            np.array([e.last_info(), ms["build"], ms["factor"], ms["solve"], e.last_covariance_ms(), e.last_reliability_ms()])]


def test_a_snoop_that_rejects_nothing_changes_nothing():
    d, e = _open("43")
    _, f = _open("43")
    for h in (e, f):
        h.iterate(1e-3)
    e.covariance(0.0)
    rel = e.reliability(1e-3)
    before = _snapshot(e)
    got = e.snoop(1e-3, float("inf"), True, 6, 3)
    assert (got["rows"], got["landmarks"], got["rows_via_landmarks"], got["info"]) == (0, 0, 0, 0) and got["crit_used"] == float("inf")
    got = e.snoop(1e-3, float("inf"), False, 0, 0)
    assert (got["rows"], got["landmarks"], got["rows_via_landmarks"]) == (0, 0, 0)
    for a, b in zip(before, _snapshot(e)):
        assert a.tobytes() == b.tobytes()
    assert not e.rejected()[0].any() and not e.rejected()[1].any()
    assert _same_rel(rel, e.reliability(1e-3))
    assert e.iterate(1e-4) == f.iterate(1e-4) and all(np.array_equal(a, b) for a, b in zip(e.get_state(), f.get_state()))
    e.close()
    f.close()


def test_failed_factorisation_rejects_nothing():
    from vinsat_amd._lib import VbaError
    _, row, _ = C.late_failure_reference()
    d, e = _open(d=C.case("late_failure"))
    _, f = _open(d=C.case("late_failure"))
    with pytest.raises(VbaError, match=f"row {row}"):
        e.snoop(0.0, 1.0, True, 6, 3)
    got = e.snoop(0.0, 1.0, True, 6, 3, strict=False)
    assert got["info"] == row + 1 == 595 and (got["rows"], got["landmarks"], got["rows_via_landmarks"]) == (0, 0, 0) and np.isnan(got["crit_used"])
    assert e.snoop(0.0, 1.0, False, 6, 3, strict=False)["crit_used"] == 1.0
    assert not e.rejected()[0].any() and not e.rejected()[1].any() and e.last_info() == 0
    assert e.iterate(1e-3) == f.iterate(1e-3) and all(np.array_equal(a, b) for a, b in zip(e.get_state(), f.get_state()))
    e.close()
    f.close()


def test_two_handles_and_two_calls_give_equal_masks():
    d, e = _open("43")
    _, f = _open("43")
    crit = _crit90(e.reliability(1e-3), d["w"])
    a = e.snoop(1e-3, crit, True, 6, 3)
    ma = e.rejected()
    e.restore_rejected()
    b = e.snoop(1e-3, crit, True, 6, 3)
    mb = e.rejected()
    c = f.snoop(1e-3, crit, True, 6, 3)
    mc = f.rejected()
    assert a == b == c and a["rows"] > 0
    for m in (mb, mc):
        assert np.array_equal(ma[0], m[0]) and np.array_equal(ma[1], m[1])
    e.close()
    f.close()


def test_argument_and_state_errors():
    from vinsat_amd._lib import load
    lib = load()
    d, e = _open("12")
    info, nul = ctypes.c_int(), None
    bad = [(None, 0.0, 3.0, 1, 6, 3), (e.h, -1.0, 3.0, 1, 6, 3), (e.h, float("nan"), 3.0, 1, 6, 3), (e.h, 0.0, -1.0, 1, 6, 3),
           (e.h, 0.0, float("nan"), 1, 6, 3), (e.h, 0.0, 3.0, 1, -1, 3), (e.h, 0.0, 3.0, 1, 6, -1)]
    for args in bad:
        assert lib.vba_schur_snoop(*args, nul, nul, ctypes.byref(info)) == 1, args        # VBA_EINVAL
    assert lib.vba_schur_snoop(e.h, 0.0, 3.0, 1, 6, 3, nul, nul, None) == 1
    assert lib.vba_schur_rejected(None, None, None, None) == 1 and lib.vba_schur_snoop_restore(None) == 1 and lib.vba_schur_last_snoop_ms(None, None) == 1
    assert not e.rejected()[0].any()
    s = e.structure
    h = ctypes.c_void_p()
    assert lib.vba_schur_create(0, e.n, e.m, e.L, int(s["blk_i"].size), int(s["pair_k"].size), ctypes.byref(h)) == 0
    rc = lib.vba_schur_snoop(h, 0.0, 3.0, 1, 6, 3, nul, nul, ctypes.byref(info))
    assert rc != 0 and rc == lib.vba_schur_reliability(h, 0.0, *[None] * 7, ctypes.byref(info))
    lib.vba_schur_destroy(h)
    e.close()


def _lm_by_hand(e, lamda0=1e-4, max_iters=20, tol=1e-10):
    """The driver ``SchurBA.solve()`` has always been."""
    lam, hist = float(lamda0), []
    for _ in range(max_iters):
        c0, c1, ok = e.iterate(lam)
        hist.append((c0, c1, ok, lam))
        if ok:
            lam = max(lam * 0.1, 1e-9)
            if c0 - c1 <= tol * max(c0, 1e-300):
                break
        else:
            lam *= 10.0
            if lam > 1e8:
                break
    return hist


def test_planted_window_and_the_solve_driver():
    """The rounds the host test vetted (their totals, every planted item and no other), every round's masks against the rule at the
    device's own tests; ``solve(snoop=...)`` ends with the same masks; ``solve()`` returns the history it always returned."""
    d = SC.planted()
    opts = dict(SC.SNOOP)
    rounds, lam = opts.pop("rounds"), opts.pop("lamda")
    _, e = _open(d=d)
    _, f = _open(d=d)
    _, g = _open(d=d)
    assert e.solve() == _lm_by_hand(g)
    totals = []
    for k in range(rounds):
        rel = e.reliability(lam)
        w_now = _weights(e, d)
        want = SO.select_from(rel, d, w=w_now, **opts)
        before = e.rejected()
        got = e.snoop(lam, **opts)
        after = e.rejected()
        totals.append((got["rows"], got["landmarks"], got["rows_via_landmarks"]))
        print(f"FIGURES schur snoop planted round {k}: device {totals[-1]} rule {want['counts']} crit_used {got['crit_used']:.4g} margin {want['margin']:.2e}")
        assert totals[-1] == want["counts"] and got["crit_used"] == want["crit_used"]
        assert np.array_equal(after[0], before[0] | want["rows"] | want["via"]) and np.array_equal(after[1], before[1] | want["landmarks"])
        if got["rows"] + got["landmarks"] == 0:
            break
        e.solve()
    assert tuple(totals) == SC.EXPECTED_ROUNDS
    rows, lms = e.rejected()
    via = np.isin(d["landmark_of_row"], d["displaced_lms"])
    assert np.array_equal(np.nonzero(rows & ~via)[0], d["planted_rows"]) and np.array_equal(np.nonzero(lms)[0], d["displaced_lms"])
    assert np.array_equal(rows & via, via & (d["w"] > 0.0))
    st, _ = e.get_state()
    print(f"FIGURES schur snoop planted: mean position error with snooping {SC.position_error(d, st):.4g} km")
    # the driver
    hist = f.solve(snoop=SC.SNOOP)
    snoops = [h[1] for h in hist if h[0] == "snoop"]
    assert tuple((s["rows"], s["landmarks"], s["rows_via_landmarks"]) for s in snoops) == SC.EXPECTED_ROUNDS
    frows, flms = f.rejected()
    assert np.array_equal(frows, rows) and np.array_equal(flms, lms)
    assert all(np.array_equal(a, b) for a, b in zip(e.get_state(), f.get_state()))
    for h in (e, f, g):
        h.close()
