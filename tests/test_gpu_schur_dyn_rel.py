"""``vba_schur_reliability_dyn`` / ``vba_schur_snoop_dyn`` (``SchurBA.state_reliability``, ``SchurBA.state_snoop``) on the GPU: the
reliability query and the snoop of a handle with the dynamics factor against the CPU reference of tests/schur_dyn_rel_cases.py (cases
and bars: that module; tests/test_schur_dyn_rel_host.py holds the floors below 1e-8 and the conditions of the planted outliers).
PARITY UNPINNED as the rest of the add-on.  Every figure is printed before it is asserted.  Device against reference, measured on
an MI355X: DESIGN 9.7.
"""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import schur_cases as SC
import schur_dyn_cov_cases as V
import schur_dyn_rel_cases as Q
import schur_query_harness as H

pytestmark = pytest.mark.gpu
OUTPUTS = H.REL_OUTPUTS["dyn"]
engine = functools.partial(H.engine, dynamics=True)
_fitv, _same, _same_cov, _raw = H._fitv, H._same(OUTPUTS), H._same_cov, functools.partial(H._raw, "dyn")


def _matches(e, name, lam, label=""):
    r, d = Q.reference(name, lam), Q.case(name)
    got = e.state_reliability(lam)
    assert got["info"] == 0
    fig = Q.figures(got, r)
    om = abs(got["fit"]["omega"] - r.cost) / r.cost
    print(f"FIGURES state rel {name} {label} lam={lam:g} " + " ".join(f"{k}={fig[k]:.2e} (floor {r.floor[k]:.1e}, bar {Q.bar(r, k):.1e})" for k in Q.FAMILIES) +
          f" landmarks left out {int((~r.lm_kept).sum())}; omega {om:.1e}")
    assert all(np.all(np.isfinite(got[k])) for k in ("leverage", "wtest", "lm_leverage", "edge_leverage", "edge_omega"))
    assert np.all(np.isfinite(got["lm_wtest"][r.lm_kept]))
    for k in Q.FAMILIES:
        assert fig[k] <= Q.bar(r, k), k
    assert np.all(got["edge_leverage"] > 0.0) and np.all(got["edge_leverage"] <= 6.0)
    assert Q.rel(got["edge_omega"], r.edge_omega) <= 1e-10         # (a cost share: the bar of c0 in tests/schur_dyn_cases.py)
    assert om <= 1e-12
    H.statistics_and_totals("dyn", Q, d, e, got, r)
    return got, r


# ------------------------------------------------------------------------------------------------ 1. accuracy, device identity
@pytest.mark.parametrize("name,lam", Q.CASES)
def test_matches_the_reference(name, lam):
    e = engine(Q.case(name))
    got, r = _matches(e, name, lam)
    assert e.last_state_reliability_ms() > 0.0
    # the trace identity from the device's own outputs
    c = e.state_covariance(lam)
    trace = np.trace(c["state"], axis1=1, axis2=2).sum() + np.trace(c["landmark"], axis1=1, axis2=2).sum()
    fit = got["fit"]
    ident = fit["t_rows"] + fit["t_prior"] + fit["t_edges"] + lam * trace
    print(f"FIGURES state rel identity {name} lam={lam:g}: {ident!r} of {r.unknowns}, rho {fit['rho']!r}, t_edges {fit['t_edges']!r} of {6 * (e.n - 1)}")
    assert abs(ident - r.unknowns) <= 1e-9 * r.unknowns
    if lam == 0.0:
        assert abs(fit["rho"] - (2 * e.m - 3 * e.n - 6)) <= 1e-9 * r.unknowns
    e.close()


# ------------------------------------------------------------------------------------------------ 2. failure case
def test_failed_factorisation_gives_nan_and_the_row():
    from vinsat_amd._lib import VbaError
    name, lam = Q.FAILURE
    _, _, _, S9 = V.failure_system()
    row, _ = SC.first_bad_pivot(S9)
    e = engine(Q.case(name))
    rc, info, *bufs = _raw(e, lam)
    print(f"FIGURES state rel failure info={info} expected={row + 1}")
    assert rc == 0 and info == row + 1 == 124
    assert all(np.all(np.isnan(b)) for b in bufs)
    assert e.last_info() == 0                       # the handle's own record belongs to its iterates
    with pytest.raises(VbaError, match=f"row {row}\\b"):
        e.state_reliability(lam)
    g = e.state_reliability(lam, strict=False)
    assert g["info"] == info and all(np.all(np.isnan(g[k])) for k in OUTPUTS[:-1]) and all(np.isnan(v) for v in g["fit"].values())
    s = e.state_snoop(lam, strict=False)
    assert s["info"] == info and s["rows"] == s["landmarks"] == s["rows_via_landmarks"] == 0 and np.isnan(s["crit_used"])
    assert not e.rejected()[0].any()
    _matches(e, name, 1e-3, label="after the failure")
    e.close()


# ------------------------------------------------------------------------------------------------ 3. bits
def test_second_query_second_handle_and_null_outputs_give_the_same_bits():
    d = Q.case("29")
    e, f = engine(d), engine(d)
    a = e.state_reliability(1e-3)
    e.state_reliability(0.0)                        # (another damping and another query through the same scratch in between)
    e.state_covariance(1e-2)
    assert _same(a, e.state_reliability(1e-3)) and _same(a, f.state_reliability(1e-3))
    full = _raw(e, 1e-3)
    assert full[0] == 0 and full[1] == 0
    for on in itertools.product((False, True), repeat=9):           # every NULL combination
        rc, info, *bufs = _raw(e, 1e-3, on)
        assert rc == 0 and info == 0
        for k in range(9):
            assert (bufs[k] is None) == (not on[k])
            if on[k]:
                assert np.array_equal(bufs[k], full[2 + k], equal_nan=True), (on, OUTPUTS[k])
    e.close(), f.close()


@pytest.mark.parametrize("name", ("29", "86"))
def test_without_weight_the_factor_is_not_there(name):
    """sigma_dyn = 1e-30: rows and priors agree with the plain handle's reliability(1e-3)."""
    d = Q.case(name)
    p, t = engine(d, dynamics=False), engine(d, sigma_dyn=1e-30)
    plain, tiny = p.reliability(1e-3), t.state_reliability(1e-3)
    p.close(), t.close()
    fig = {k: Q.rel(tiny[k], plain[k]) for k in ("leverage", "wtest", "lm_leverage", "lm_wtest")}
    print(f"FIGURES state rel {name} sigma_dyn=1e-30 against the plain handle: " + " ".join(f"{k}={v:.2e}" for k, v in fig.items()))
    assert max(fig.values()) <= 1e-9
    for k in ("omega", "m_eff", "t_rows", "t_prior", "max_wtest", "max_lm_wtest"):
        assert abs(tiny["fit"][k] - plain["fit"][k]) <= 1e-9 * abs(plain["fit"][k]), k
    assert np.all(tiny["edge_leverage"] >= 0.0) and tiny["fit"]["t_edges"] <= 1e-9


# ------------------------------------------------------------------------------------------------ 4. the query changes nothing
def _snapshot(e):
    st, X = e.get_state()
    dc, dl = e.last_step()
    ms = e.last_ms()
    return [e.dynamics_residual(), e.dynamics_jacobian(), e.dynamics_edge_cost(), dc.copy(), dl.copy(), e.last_velocity_step(),
            e.cholesky_factor(), st, X, np.array([e.last_info(), ms["build"], ms["factor"], ms["solve"], e.last_state_covariance_ms()])]


def test_query_changes_nothing_the_handle_shows():
    """After an accepted trial the resident state is not the state the handle's r, D Phi and edge costs were built at: a query that
    built into the handle's arrays would change what the fetches return.  Handle f never asks."""
    d = Q.case("29")
    e, f = engine(d), engine(d)
    for eng in (e, f):
        for _ in range(6):
            if eng.iterate(1e-3)[2]:
                break
        else:
            raise AssertionError("no trial was accepted")
    cov = e.state_covariance(1e-3, pairs=True)
    before = _snapshot(e)
    assert e.state_reliability(0.0)["info"] == 0 and e.state_reliability(1e-3)["info"] == 0
    assert e.state_snoop(1e-3, crit=float("inf"))["rows"] == 0                 # (a snoop that rejects nothing changes nothing)
    for a, b in zip(before, _snapshot(e)):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(before[:-1], _snapshot(f)[:-1]):
        assert a.tobytes() == b.tobytes()
    again, other = e.state_covariance(1e-3, pairs=True), f.state_covariance(1e-3, pairs=True)
    assert _same_cov(cov, again) and _same_cov(cov, other) and np.array_equal(cov["pairs"][2], again["pairs"][2])
    assert e.iterate(1e-4) == f.iterate(1e-4)
    for a, b in zip(e.get_state(), f.get_state()):
        assert np.array_equal(a, b)
    assert _same(e.state_reliability(1e-3), f.state_reliability(1e-3))
    e.close(), f.close()


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_contract_and_refusals():
    from vinsat_amd._lib import VbaError
    d = Q.case("12")
    p = engine(d, dynamics=False)
    for call in (p.state_reliability, p.state_snoop, lambda: p.solve(max_iters=1, state_snoop=dict(rounds=1))):
        with pytest.raises(VbaError, match="dynamics factor is not enabled"):
            call()
    assert p.reliability()["info"] == 0
    p.close()
    e = engine(d)
    for call in (e.reliability, e.snoop, e.covariance, lambda: e.solve(max_iters=1, snoop=dict(rounds=1))):
        with pytest.raises(VbaError, match="not available on a handle with the dynamics factor"):
            call()
    with pytest.raises(ValueError):
        e.solve(max_iters=1, snoop=dict(), state_snoop=dict())
    for bad in (-1.0, float("nan")):
        with pytest.raises(VbaError, match="lamda must be >= 0"):
            e.state_reliability(bad)
        with pytest.raises(VbaError, match="lamda must be >= 0"):
            e.state_snoop(bad)
        with pytest.raises(VbaError, match="crit must be >= 0"):
            e.state_snoop(0.0, crit=bad)
    lib, info, nul = e.lib, ctypes.c_int(), [None] * 9
    assert lib.vba_schur_reliability_dyn(None, 0.0, *nul, ctypes.byref(info)) == 1         # VBA_EINVAL
    assert lib.vba_schur_reliability_dyn(e.h, 0.0, *nul, None) == 1
    assert lib.vba_schur_snoop_dyn(None, 0.0, 3.0, 1, 6, 3, None, None, ctypes.byref(info)) == 1
    assert lib.vba_schur_snoop_dyn(e.h, 0.0, 3.0, 1, 6, 3, None, None, None) == 1
    assert lib.vba_schur_snoop_dyn(e.h, 0.0, 3.0, 1, -1, 3, None, None, ctypes.byref(info)) == 1
    assert lib.vba_schur_last_reliability_dyn_ms(None, None) == 1 and lib.vba_schur_last_snoop_dyn_ms(None, None) == 1
    assert lib.vba_schur_reliability_dyn(e.h, 1e-3, *nul, ctypes.byref(info)) == 0 and info.value == 0     # everything NULL but info
    e.close()


# ------------------------------------------------------------------------------------------------ 6. planted outliers
def _converged(d):
    e = engine(d)
    hist = e.solve()
    assert any(ok for _, _, ok, _ in hist) and hist[-1][0] - hist[-1][1] <= 1e-6 * hist[-1][0]
    return e


def test_planted_row_is_suspected_and_rejected():
    from vinsat_amd.schur import suspects
    d, r = Q.planted_outlier(), Q.planted_reference("row")
    e = _converged(d)
    got = e.state_reliability(0.0)
    order = np.argsort(-got["wtest"])
    print(f"FIGURES state rel planted row {d['planted_row']}: first {order[:3]} {got['wtest'][order[:3]]} (oracle {r.wtest[order[0]]:.4f}) "
          f"largest landmark test {got['fit']['max_lm_wtest']:.3f} s0sq {got['fit']['s0sq']:.3f}")
    assert order[0] == d["planted_row"] and got["fit"]["max_wtest"] == got["wtest"][order[0]]
    crit = 0.5 * (got["wtest"][order[0]] + max(got["wtest"][order[1]], got["fit"]["max_lm_wtest"]))
    rows, lms = suspects(got, crit)
    assert np.array_equal(rows, [d["planted_row"]]) and lms.size == 0
    rows, _ = suspects(got, crit / np.sqrt(got["fit"]["s0sq"]), scaled=True)
    assert np.array_equal(rows, [d["planted_row"]])
    res = e.state_snoop(0.0, crit=crit, scaled=False)
    assert (res["rows"], res["landmarks"], res["rows_via_landmarks"], res["crit_used"]) == (1, 0, 0, crit)
    mask, lm_mask = e.rejected()
    assert np.array_equal(np.nonzero(mask)[0], [d["planted_row"]]) and not lm_mask.any()
    assert e.weights()[d["planted_row"]] == 0.0 and e.last_state_snoop_ms() > 0.0
    e.close()


def test_moved_catalogue_entry_is_suspected_and_rejected():
    from vinsat_amd.schur import suspects
    d, r = Q.displaced_landmark(), Q.planted_reference("landmark")
    e = _converged(d)
    got = e.state_reliability(0.0)
    order = np.argsort(-np.nan_to_num(got["lm_wtest"]))
    l = d["displaced_lm"]
    print(f"FIGURES state rel displaced landmark {l}: first {order[:3]} {got['lm_wtest'][order[:3]]} (oracle {r.lm_wtest[l]:.4f}) "
          f"largest row test {got['fit']['max_wtest']:.3f}")
    assert order[0] == l and got["fit"]["max_lm_wtest"] == got["lm_wtest"][l]
    crit = 0.5 * (got["lm_wtest"][l] + max(got["lm_wtest"][order[1]], got["fit"]["max_wtest"]))
    rows, lms = suspects(got, crit)
    assert rows.size == 0 and np.array_equal(lms, [l])
    res = e.state_snoop(0.0, crit=crit, scaled=False)
    track = int((d["landmark_of_row"] == l).sum())
    assert (res["rows"], res["landmarks"], res["rows_via_landmarks"]) == (0, 1, track)
    mask, lm_mask = e.rejected()
    assert np.array_equal(np.nonzero(lm_mask)[0], [l]) and np.array_equal(mask, d["landmark_of_row"] == l)
    e.close()


# ------------------------------------------------------------------------------------------------ 7. the snoop's promise
def _everything(e):
    return e.iterate(1e-3), e.state_covariance(1e-3), e.state_reliability(1e-3), e.get_state()


def test_handle_behaves_as_a_fresh_one_with_those_weights_zeroed():
    d = Q.planted_outlier()
    e = _converged(d)
    st = e.get_state()
    never = engine(d, state=st)
    rel0 = e.state_reliability(1e-3)
    res = e.state_snoop(1e-3, crit=3.29, scaled=True)
    print(f"FIGURES state snoop on the converged 29 / 300 with the planted row: {res}")
    assert res["info"] == 0 and res["rows"] >= 1
    assert res["crit_used"] == 3.29 * np.sqrt(rel0["fit"]["s0sq"])
    mask, _ = e.rejected()
    assert mask[d["planted_row"]] and mask.sum() == res["rows"] + res["rows_via_landmarks"]
    w = e.weights()
    assert np.array_equal(w == 0.0, mask) and np.array_equal(w[~mask], d["w"][~mask])
    fresh = engine(d, state=st, w=np.where(mask, 0.0, d["w"]))
    a, b = _everything(e), _everything(fresh)
    assert a[0] == b[0] and _same_cov(a[1], b[1]) and _same(a[2], b[2]) and all(np.array_equal(x, y) for x, y in zip(a[3], b[3]))
    fresh.close()
    # restore: the bits of a handle that never snooped (from the same state: e has moved on)
    e.restore_rejected()
    assert not e.rejected()[0].any() and np.array_equal(e.weights(), d["w"])
    e.set_state(*st)
    a, b = _everything(e), _everything(never)
    assert a[0] == b[0] and _same_cov(a[1], b[1]) and _same(a[2], b[2]) and all(np.array_equal(x, y) for x, y in zip(a[3], b[3]))
    e.close(), never.close()


def test_solve_with_state_snoop_rejects_the_planted_row():
    d = Q.planted_outlier()
    e, f = engine(d), engine(d)
    plain = f.solve()
    hist = e.solve(state_snoop=dict(crit=6.0, scaled=True, rounds=4))
    rounds = [h[1] for h in hist if h[0] == "snoop"]
    end = [h for h in hist if h[0] != "snoop"][-1][1]
    print(f"FIGURES solve(state_snoop): rounds {rounds}; cost {end!r} against {plain[-1][1]!r} without")
    assert rounds and rounds[0]["rows"] >= 1 and rounds[-1]["rows"] + rounds[-1]["landmarks"] == 0
    assert e.rejected()[0][d["planted_row"]]
    assert end < plain[-1][1]
    e.close(), f.close()
