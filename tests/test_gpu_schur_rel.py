"""``vba_schur_reliability`` / ``SchurBA.reliability`` on the GPU against the CPU reference of tests/schur_rel_cases.py.

Bars: ``max(100 x floor of the case, 1e-11)`` relative to the largest entry of the family (leverage / wtest / lm_leverage /
lm_wtest); the floor is the disagreement of the reference's two NumPy routes (tests/test_schur_rel_host.py holds it below 1e-8).
Every figure is printed before it is asserted.  Rows whose ``I - P_k`` has a smallest eigenvalue below 1e-3 in the REFERENCE are
held on leverage only, at most 1 % of a case's rows (the reference alone leaves out 5 of 1474 in ``behind_the_camera``, where the
leverage reaches 1.99999, and none elsewhere); landmarks seen from one pose at ``lamda = 0`` have an exactly singular ``I - P_l``
and are held on lm_leverage only (``schur_rel_cases.LM_EIG_MIN``: 37 landmarks of ``more_landmarks_than_rows``, none elsewhere).
Every test here needs the entry point and fails where it does not exist.

Device against reference, measured on an MI355X: see DESIGN section 9.2.
"""
import ctypes
import functools

import numpy as np
import pytest

import schur_cases as C
import schur_query_harness as H
import schur_rel_cases as R

pytestmark = pytest.mark.gpu
OUTPUTS = H.REL_OUTPUTS["plain"]
_same, _raw = H._same(OUTPUTS), functools.partial(H._raw, "plain")


def _open(name=None, d=None, state=None):
    d = R.problem(name) if d is None else d
    return d, H.engine(d, state=state)


def _consistent(d, e, got, lam):
    """Statistics and totals against the device's own rows (sums to rounding of another order, maxima and counts exactly), and the
    trace identity ``t_rows + t_prior + lamda tr(H^-1) = 6 n + 3 L`` with the trace from the device's covariance blocks."""
    fit = got["fit"]
    H.statistics_and_totals("plain", R, d, e, got)
    c = e.covariance(lam)
    trace = np.trace(c["pose"], axis1=1, axis2=2).sum() + np.trace(c["landmark"], axis1=1, axis2=2).sum()
    ident = fit["t_rows"] + fit["t_prior"] + lam * trace
    print(f"FIGURES rel identity {ident!r} of {6 * e.n + 3 * e.L}, rho {fit['rho']!r}")
    return ident


def _matches(e, name, lam, label=""):
    r, d = R.reference(name, lam), R.problem(name)
    got = e.reliability(lam)
    assert got["info"] == 0
    fig = R.figures(got, r)
    out, lm_out = int((~r.kept).sum()), int((~r.lm_kept).sum())
    print(f"FIGURES rel {name} {label} lam={lam:g} " + " ".join(f"{k}={fig[k]:.2e} (floor {r.floor[k]:.1e}, bar {R.bar(r, k):.1e})" for k in R.FAMILIES) +
          f" rows left out {out} of {r.kept.size}, landmarks {lm_out} of {r.lm_kept.size}; omega {abs(got['fit']['omega'] - r.fit['omega']) / r.fit['omega']:.1e}")
    assert out <= R.MAX_LEFT_OUT * r.kept.size
    assert np.all(np.isfinite(got["leverage"])) and np.all(np.isfinite(got["lm_leverage"]))
    assert np.all(np.isfinite(got["wtest"][r.kept])) and np.all(np.isfinite(got["lm_wtest"][r.lm_kept]))
    left = got["lm_wtest"][~r.lm_kept]
    assert np.all(np.isnan(left) | (left >= 0.0))
    for k in R.FAMILIES:
        assert fig[k] <= R.bar(r, k), k
    assert abs(got["fit"]["omega"] - r.fit["omega"]) <= 1e-10 * r.fit["omega"]         # (the bar of c0 in tests/test_schur_gpu.py)
    ident = _consistent(d, e, got, lam)
    assert abs(ident - r.unknowns) <= 1e-9 * r.unknowns         # (the identity sums the four families: their bars are 1e-11 .. 7e-8)
    return got, r


@pytest.mark.parametrize("name,lam", [c for c in R.CASES if c[0] not in ("more_landmarks_than_rows", "zero_weights", "behind_the_camera")])
def test_matches_the_reference(name, lam):
    d, e = _open(name)
    got, r = _matches(e, name, lam)
    assert not (~r.kept).any() and r.lm_kept.all()
    assert e.last_reliability_ms() > 0.0
    if lam == 0.0:
        assert abs(got["fit"]["rho"] - (2 * e.m - 6 * e.n)) <= 1e-9 * e.m        # all weights positive
    e.close()


def test_zero_weights_are_rows_without_a_test():
    d, e = _open("zero_weights")
    got, r = _matches(e, "zero_weights", 1e-3)
    off = d["w"] == 0.0
    assert off.sum() == (e.m + 6) // 7
    assert np.array_equal(got["leverage"][off], np.zeros(off.sum())) and np.array_equal(got["wtest"][off], np.zeros(off.sum()))
    assert got["fit"]["m_eff"] == e.m - off.sum()
    e.close()


def test_unobserved_landmarks_and_short_tracks():
    d, e = _open("more_landmarks_than_rows")
    got, r = _matches(e, "more_landmarks_than_rows", 0.0)
    track = np.bincount(d["landmark_of_row"], minlength=e.L)
    assert set(np.unique(track)) == set(range(6)) and int((~r.lm_kept).sum()) == int((track == 1).sum())
    u = d["unobserved"]
    assert u.size > 200
    for lam in (0.0, 1e-3):
        g = got if lam == 0.0 else e.reliability(lam)
        is2 = 1.0 / (d["sigma"] * d["sigma"])
        closed = (3.0 * (1.0 / (is2 + lam))) * is2                   # the rounding order include/vinsat_ba.h states
        assert np.array_equal(g["lm_wtest"][u], np.zeros(u.size)) and np.array_equal(g["lm_leverage"][u], np.full(u.size, closed))
        assert np.array_equal(g["lm_stats"][u], np.zeros((u.size, 3)))
    assert abs(got["fit"]["rho"] - (2 * e.m - 6 * e.n)) <= 1e-9 * e.m
    e.close()


def test_long_tracks_with_high_leverage():
    d, e = _open("more_poses_than_landmarks")
    got, r = _matches(e, "more_poses_than_landmarks", 1e-3)
    assert np.bincount(d["landmark_of_row"]).max() == 12 and 1.1 < got["leverage"].max() < 1.3
    e.close()


def test_landmarks_behind_the_camera():
    d, e = _open("behind_the_camera")
    got, r = _matches(e, "behind_the_camera", 1e4)
    assert 0 < (~r.kept).sum() <= R.MAX_LEFT_OUT * e.m and np.array_equal(np.nonzero(~r.kept)[0], d["clamped_rows"])
    assert got["leverage"][~r.kept].max() > 1.9999
    e.close()


def _converged(d):
    dd, e = _open(d=d)
    hist = e.solve()
    assert any(ok for _, _, ok, _ in hist) and hist[-1][0] - hist[-1][1] <= 1e-6 * hist[-1][0]
    return e


def test_planted_outlier_ranks_first():
    from vinsat_amd.schur import suspects
    d = R.planted_outlier()
    e = _converged(d)
    got = e.reliability(0.0)
    order = np.argsort(-got["wtest"])
    print(f"FIGURES rel planted row {d['planted_row']}: first {order[:3]} {got['wtest'][order[:3]]} s0sq {got['fit']['s0sq']:.3f}")
    assert order[0] == d["planted_row"] and got["fit"]["max_wtest"] == got["wtest"][order[0]]
    crit = 0.5 * (got["wtest"][order[0]] + got["wtest"][order[1]])
    rows, lms = suspects(got, crit)
    assert np.array_equal(rows, [d["planted_row"]]) and lms.size == 0
    rows, _ = suspects(got, crit / np.sqrt(got["fit"]["s0sq"]), scaled=True)
    assert np.array_equal(rows, [d["planted_row"]])
    # the landmark and the pose of that row carry it in their statistics
    assert got["lm_stats"][d["landmark_of_row"][d["planted_row"]], 1] == got["wtest"][order[0]]
    assert got["pose_stats"][d["pose_of_row"][d["planted_row"]], 1] == got["wtest"][order[0]]
    e.close()


def test_displaced_catalogue_entry_ranks_first():
    from vinsat_amd.schur import suspects
    d = R.displaced_landmark()
    e = _converged(d)
    got = e.reliability(0.0)
    order = np.argsort(-got["lm_wtest"])
    print(f"FIGURES rel displaced landmark {d['displaced_lm']}: first {order[:3]} {got['lm_wtest'][order[:3]]} largest row {got['fit']['max_wtest']:.3f}")
    assert order[0] == d["displaced_lm"] and got["fit"]["max_lm_wtest"] == got["lm_wtest"][order[0]]
    crit = 0.5 * (got["lm_wtest"][order[0]] + max(got["lm_wtest"][order[1]], got["fit"]["max_wtest"]))
    rows, lms = suspects(got, crit)
    assert rows.size == 0 and np.array_equal(lms, [d["displaced_lm"]])
    e.close()


@pytest.mark.parametrize("mode", ["0", "1", "2"])
def test_failed_factorisation_gives_nan_and_the_row(mode, monkeypatch):
    _, row, _ = C.late_failure_reference()
    monkeypatch.setenv("VBA_SCHUR_CLASSIC", mode)                   # read in vba_schur_create
    d, e = _open(d=C.case("late_failure"))
    rc, info, *bufs = _raw(e, 0.0)
    print(f"FIGURES rel late_failure classic={mode} info={info} expected={row + 1}")
    assert rc == 0 and info == row + 1 == 595
    assert all(np.all(np.isnan(b)) for b in bufs)
    assert e.last_info() == 0                       # the handle's own record belongs to its iterates
    from vinsat_amd._lib import VbaError
    with pytest.raises(VbaError, match=f"row {row}"):
        e.reliability(0.0)
    g = e.reliability(0.0, strict=False)
    assert g["info"] == info and all(np.all(np.isnan(g[k])) for k in OUTPUTS[:-1]) and all(np.isnan(v) for v in g["fit"].values())
    e.close()


@pytest.mark.parametrize("mode", ["1", "2"])
def test_comparison_factorisations_serve_the_query(mode, monkeypatch):
    monkeypatch.setenv("VBA_SCHUR_CLASSIC", mode)
    d, e = _open("43")
    _matches(e, "43", 1e-3, label=f"classic={mode}")
    e.close()


def test_null_outputs_return_the_same_bits():
    d, e = _open("12")
    full = _raw(e, 1e-3)
    assert full[0] == 0 and full[1] == 0
    masks = [0, 1, 2, 3, 0b1111000, 0b0000100, 0b1000000, 0b0110000, 0b1010101, 0b0101010, 0b1111110]
    for mask in masks:
        on = [bool(mask >> k & 1) for k in range(7)]
        rc, info, *bufs = _raw(e, 1e-3, on)
        assert rc == 0 and info == 0
        for k in range(7):
            assert (bufs[k] is None) == (not on[k])
            if on[k]:
                assert np.array_equal(bufs[k], full[2 + k], equal_nan=True), (mask, OUTPUTS[k])
    e.close()


def test_queries_repeat_bit_for_bit_on_one_handle_and_across_handles():
    d, e = _open("43")
    _, f = _open("43")
    a, b, c = e.reliability(0.0), e.reliability(0.0), f.reliability(0.0)
    e.reliability(1e-3)                             # (another damping through the same scratch in between)
    e.covariance(1e-2)
    g = e.reliability(0.0)
    for o in (b, c, g):
        assert _same(a, o)
    e.close()
    f.close()


def _snapshot(e):
    st, X = e.get_state()
    dc, dl = e.last_step()
    ms = e.last_ms()
    return [st, X, dc.copy(), dl.copy(), e.cholesky_factor(), np.array([e.last_info(), ms["build"], ms["factor"], ms["solve"], e.last_covariance_ms()])]


def test_query_changes_nothing_the_handle_shows():
    d, e = _open("43")
    e.iterate(1e-3)
    cov = e.covariance(0.0, pairs=True)
    before = _snapshot(e)
    e.reliability(0.0)
    e.reliability(1e-2)
    after = _snapshot(e)
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()
    again = e.covariance(0.0, pairs=True)
    assert np.array_equal(cov["pose"], again["pose"]) and np.array_equal(cov["landmark"], again["landmark"]) and np.array_equal(cov["pairs"][2], again["pairs"][2])
    e.close()


def test_iterates_and_covariances_return_the_same_bits_with_queries_between_them():
    """Handle e asks for the reliability (first, before any covariance query: its first query allocates both scratches) around every
    call; handle f never does."""
    d, e = _open("43")
    _, f = _open("43")
    runs = []
    for eng, ask in ((e, True), (f, False)):
        out = []
        for lam in (1e-3, 1e-4, 1e-5):
            if ask:
                assert eng.reliability(0.0)["info"] == 0
            out.append(eng.iterate(lam))
            if ask:
                eng.reliability(lam)
            c = eng.covariance(lam, pairs=True)
            out.append((c["pose"].tobytes(), c["landmark"].tobytes(), c["pairs"][2].tobytes()))
        runs.append((out, *eng.get_state()))
    assert runs[0][0] == runs[1][0] and any(o[2] for o in runs[0][0][::2])
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])
    e.close()
    f.close()


def test_first_query_of_a_handle_that_never_asked_for_a_covariance():
    d, e = _open("12")
    _, f = _open("12")
    f.covariance(0.0)
    assert _same(e.reliability(0.0), f.reliability(0.0))
    e.close()
    f.close()


def test_rows_come_back_in_the_callers_order():
    d = R.problem("12")
    perm = np.random.default_rng(3).permutation(d["uv"].shape[0])
    p = dict(d)
    for k in ("uv", "w", "pose_of_row", "landmark_of_row"):
        p[k] = d[k][perm]
    _, e = _open(d=p)
    r = R.reference("12", 0.0)
    got = e.reliability(0.0)
    back = dict(got)
    for k in ("leverage", "wtest"):
        back[k] = np.empty(e.m)
        back[k][perm] = got[k]
    fig = R.figures(back, r)
    print("FIGURES rel permuted rows", fig)
    assert all(fig[k] <= R.bar(r, k) for k in R.FAMILIES)
    e.close()


def test_argument_and_state_errors():
    from vinsat_amd._lib import load
    lib = load()
    d, e = _open("12")
    info = ctypes.c_int()
    nul = [None] * 7
    assert lib.vba_schur_reliability(None, 0.0, *nul, ctypes.byref(info)) == 1           # VBA_EINVAL
    assert lib.vba_schur_reliability(e.h, 0.0, *nul, None) == 1
    assert lib.vba_schur_reliability(e.h, -1.0, *nul, ctypes.byref(info)) == 1
    assert lib.vba_schur_reliability(e.h, float("nan"), *nul, ctypes.byref(info)) == 1
    assert lib.vba_schur_last_reliability_ms(None, None) == 1
    s = e.structure
    h = ctypes.c_void_p()
    assert lib.vba_schur_create(0, e.n, e.m, e.L, int(s["blk_i"].size), int(s["pair_k"].size), ctypes.byref(h)) == 0
    rc = lib.vba_schur_reliability(h, 0.0, *nul, ctypes.byref(info))
    assert rc != 0 and rc == lib.vba_schur_covariance(h, 0.0, None, None, None, ctypes.byref(info))
    lib.vba_schur_destroy(h)
    e.close()
