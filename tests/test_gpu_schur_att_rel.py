"""``vba_schur_reliability_att`` / ``vba_schur_snoop_att`` / ``vba_schur_outlier_power_att`` (``SchurBA.attitude_reliability``,
``attitude_snoop``, ``attitude_outlier_power``) on the GPU: the three uncertainty queries of a handle with the dynamics AND the attitude
factor against the CPU reference of tests/schur_att_rel_cases.py (cases and bars: that module; tests/test_schur_att_rel_host.py holds
the floors below 1e-8, the conditions and the planted faults).  PARITY UNPINNED as the rest of the add-on.  Every figure is printed
before it is asserted.  Device against reference, measured on an MI355X: DESIGN 9.10.  Every test calls an entry that a library
without the feature does not have.
"""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import schur_att_rel_cases as T
import schur_power_cases as PW
import schur_query_harness as H

pytestmark = pytest.mark.gpu
OUTPUTS = H.REL_OUTPUTS["att"]
NCP = PW.NCP
engine = functools.partial(H.engine, dynamics=True, attitude=True)
_fitv, _same, _same_cov, _raw = H._fitv, H._same(OUTPUTS), H._same_cov, functools.partial(H._raw, "att")


# ------------------------------------------------------------------------------------------------ 1. accuracy, device identity
@pytest.mark.parametrize("name,lam", T.CASES)
def test_matches_the_reference(name, lam):
    r, d = T.reference(name, lam), T.case(name)
    e = engine(d)
    got = e.attitude_reliability(lam)
    assert got["info"] == 0 and e.last_attitude_reliability_ms() > 0.0
    fig = T.figures(got, r)
    fit = got["fit"]
    om = abs(fit["omega"] - r.cost) / r.cost
    print(f"FIGURES attitude rel {name} lam={lam:g} " + " ".join(f"{k}={fig[k]:.2e} (floor {r.floor[k]:.1e}, bar {T.bar(r, k):.1e})" for k in T.FAMILIES) +
          f" landmarks left out {int((~r.lm_kept).sum())}; omega {om:.1e}; att_leverage {got['att_leverage'].min():.3e} .. {got['att_leverage'].max():.5f}")
    assert all(np.all(np.isfinite(got[k])) for k in OUTPUTS[:-1] if k != "lm_wtest") and np.all(np.isfinite(got["lm_wtest"][r.lm_kept]))
    for k in T.FAMILIES:
        assert fig[k] <= T.bar(r, k), k
    assert np.all(got["edge_leverage"] > 0.0) and np.all(got["edge_leverage"] <= 6.0)
    assert np.all(got["att_leverage"] > 0.0) and np.all(got["att_leverage"] <= 3.0)
    assert T.rel(got["edge_omega"], r.edge_omega) <= 1e-10 and T.rel(got["att_omega"], r.att_omega) <= 1e-10   # (cost shares)
    assert om <= 1e-12
    ne = e.n - 1
    H.statistics_and_totals("att", T, d, e, got, r)
    # the trace identity from the device's own outputs
    c = e.state_covariance(lam)
    trace = np.trace(c["state"], axis1=1, axis2=2).sum() + np.trace(c["landmark"], axis1=1, axis2=2).sum()
    ident = fit["t_rows"] + fit["t_prior"] + fit["t_edges"] + fit["t_att"] + lam * trace
    print(f"FIGURES attitude rel identity {name} lam={lam:g}: {ident!r} of {r.unknowns}, rho {fit['rho']!r}, t_att {fit['t_att']!r} of {3 * ne}")
    assert abs(ident - r.unknowns) <= 1e-9 * r.unknowns
    if lam == 0.0:
        assert abs(fit["rho"] - (2 * e.m - 9)) <= 1e-9 * r.unknowns
    e.close()


# ------------------------------------------------------------------------------------------------ 2. the window with an empty pose
def test_empty_pose_window_is_answered_at_zero_damping():
    """43 / 450 at lamda = 0: the attitude factor holds pose 20, the undamped system is positive definite and every output is finite
    (a handle with the dynamics factor alone cannot factorise it)."""
    import schur_att_cases as AC
    d = T.case("43")
    e, p = engine(d), engine(d, attitude=False)
    got = e.attitude_reliability(0.0)
    plain = p.state_reliability(0.0, strict=False)
    i = AC.EMPTY_POSE["43"]
    print(f"FIGURES attitude rel 43 / 450 lam=0: info {got['info']}, the edges at pose {i}: att_leverage {got['att_leverage'][i - 1:i + 1]} "
          f"att_wtest {got['att_wtest'][i - 1:i + 1]}; dynamics only: info {plain['info']}")
    assert got["info"] == 0 and all(np.all(np.isfinite(got[k])) for k in OUTPUTS[:-1]) and np.all(np.isfinite(_fitv(got)))
    assert plain["info"] != 0 and np.all(np.isnan(plain["leverage"]))
    assert np.all(np.abs(got["att_leverage"][i - 1:i + 1] - 1.5) <= 1e-3)
    pw = e.attitude_outlier_power(0.0)
    assert pw["info"] == 0 and np.all(np.isfinite(pw["mdb"]))
    e.close(), p.close()


# ------------------------------------------------------------------------------------------------ 3. bits
def test_second_query_second_handle_and_null_outputs_give_the_same_bits():
    d = T.case("29")
    e, f = engine(d), engine(d)
    a = e.attitude_reliability(1e-3)
    e.attitude_reliability(0.0)                     # (another damping and other queries through the same scratch in between)
    e.state_covariance(1e-2)
    e.attitude_outlier_power(1e-2)
    assert _same(a, e.attitude_reliability(1e-3)) and _same(a, f.attitude_reliability(1e-3))
    e.close(), f.close()
    e = engine(T.case("12"))                        # every NULL combination: 4096 queries, on the smallest case
    full = _raw(e, 1e-3)
    assert full[0] == 0 and full[1] == 0
    for on in itertools.product((False, True), repeat=12):
        rc, info, *bufs = _raw(e, 1e-3, on)
        assert rc == 0 and info == 0
        for k in range(12):
            assert (bufs[k] is None) == (not on[k])
            if on[k]:
                assert np.array_equal(bufs[k], full[2 + k], equal_nan=True), (on, OUTPUTS[k])
    e.close()


@pytest.mark.parametrize("name", ("29", "86"))
def test_without_weight_the_factor_is_not_there(name):
    """sigma_att = 1e-30: rows, priors and orbit edges agree with state_reliability(1e-3) of a handle with the dynamics factor alone."""
    d = T.case(name)
    p, t = engine(d, attitude=False), engine(d, sigma_att=1e-30)
    plain, tiny = p.state_reliability(1e-3), t.attitude_reliability(1e-3)
    p.close(), t.close()
    fig = {k: T.rel(tiny[k], plain[k]) for k in ("leverage", "wtest", "lm_leverage", "lm_wtest", "edge_leverage", "edge_omega")}
    print(f"FIGURES attitude rel {name} sigma_att=1e-30 against the dynamics handle: " + " ".join(f"{k}={v:.2e}" for k, v in fig.items()))
    assert max(fig.values()) <= 1e-9
    for k in ("omega", "m_eff", "t_rows", "t_prior", "max_wtest", "max_lm_wtest", "t_edges", "omega_edges"):
        assert abs(tiny["fit"][k] - plain["fit"][k]) <= 1e-9 * abs(plain["fit"][k]), k
    assert np.all(tiny["att_leverage"] >= 0.0) and tiny["fit"]["t_att"] <= 1e-9 and tiny["fit"]["omega_att"] <= 1e-9


# ------------------------------------------------------------------------------------------------ 4. the query changes nothing
def _snapshot(e):
    st, X = e.get_state()
    dc, dl = e.last_step()
    ms = e.last_ms()
    return [e.last_velocity_step(), e.dynamics_residual(), e.dynamics_jacobian(), e.dynamics_edge_cost(), e.attitude_residual(),
            e.attitude_jacobian(), e.attitude_edge_cost(), dc.copy(), dl.copy(), e.cholesky_factor(), st, X,
            np.array([e.last_info(), ms["build"], ms["factor"], ms["solve"], e.last_state_covariance_ms()])]


def test_query_changes_nothing_the_handle_shows():
    """After an accepted trial the resident state is not the state the handle's a, J and edge costs were built at: a query that built
    into the handle's arrays would change what the fetches return.  Handle f never asks."""
    d = T.case("29")
    e, f = engine(d), engine(d)
    for eng in (e, f):
        for _ in range(6):
            if eng.iterate(1e-3)[2]:
                break
        else:
            raise AssertionError("no trial was accepted")
    cov = e.state_covariance(1e-3, pairs=True)
    before = _snapshot(e)
    assert e.attitude_reliability(0.0)["info"] == 0 and e.attitude_reliability(1e-3)["info"] == 0
    assert e.attitude_snoop(1e-3, crit=float("inf"))["rows"] == 0               # (a snoop that rejects nothing changes nothing)
    for a, b in zip(before, _snapshot(e)):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(before[:-1], _snapshot(f)[:-1]):
        assert a.tobytes() == b.tobytes()
    again, other = e.state_covariance(1e-3, pairs=True), f.state_covariance(1e-3, pairs=True)
    assert _same_cov(cov, again) and _same_cov(cov, other) and np.array_equal(cov["pairs"][2], again["pairs"][2])
    assert e.iterate(1e-4) == f.iterate(1e-4)
    for a, b in zip(e.get_state(), f.get_state()):
        assert np.array_equal(a, b)
    assert _same(e.attitude_reliability(1e-3), f.attitude_reliability(1e-3))
    e.close(), f.close()


# ------------------------------------------------------------------------------------------------ 5. contract
def test_contract_and_refusals():
    from vinsat_amd._lib import VbaError
    d = T.case("12")
    lib, info, nul = None, ctypes.c_int(), [None] * 12
    for dynamics, why in ((False, "dynamics factor is not enabled"), (True, "attitude factor is not enabled")):
        p = engine(d, attitude=False, dynamics=dynamics)
        for call in (p.attitude_reliability, p.attitude_snoop, p.attitude_outlier_power, lambda: p.solve(max_iters=1, attitude_snoop=dict(rounds=1))):
            with pytest.raises(VbaError, match=why):
                call()
        assert p.lib.vba_schur_reliability_att(p.h, 0.0, *nul, ctypes.byref(info)) == 4        # VBA_ESTATE
        assert p.lib.vba_schur_snoop_att(p.h, 0.0, 3.0, 1, 6, 3, None, None, ctypes.byref(info)) == 4
        assert p.lib.vba_schur_outlier_power_att(p.h, 0.0, NCP, 3.0, *[None] * 11, ctypes.byref(info)) == 4
        assert (p.state_reliability if dynamics else p.reliability)()["info"] == 0              # ... and its own query serves it
        p.close()
    e = engine(d)
    for call in (e.state_reliability, e.state_snoop, e.state_outlier_power):                    # the three old entries still refuse
        with pytest.raises(VbaError, match="not available on a handle with the attitude factor"):
            call()
    for call in (e.reliability, e.snoop, e.outlier_power):
        with pytest.raises(VbaError, match="not available on a handle with the dynamics factor"):
            call()
    with pytest.raises(ValueError):
        e.solve(max_iters=1, state_snoop=dict(), attitude_snoop=dict())
    for bad in (-1.0, float("nan")):
        for call in (e.attitude_reliability, e.attitude_snoop, e.attitude_outlier_power):
            with pytest.raises(VbaError, match="lamda must be >= 0"):
                call(bad)
        with pytest.raises(VbaError, match="crit must be >= 0"):
            e.attitude_snoop(0.0, crit=bad)
    with pytest.raises(VbaError, match="ncp must be positive and finite"):
        e.attitude_outlier_power(0.0, ncp=0.0)
    with pytest.raises(VbaError, match="crit must be > 0"):
        e.attitude_outlier_power(0.0, crit=0.0)
    lib = e.lib
    assert lib.vba_schur_reliability_att(None, 0.0, *nul, ctypes.byref(info)) == 1             # VBA_EINVAL
    assert lib.vba_schur_reliability_att(e.h, 0.0, *nul, None) == 1
    assert lib.vba_schur_snoop_att(None, 0.0, 3.0, 1, 6, 3, None, None, ctypes.byref(info)) == 1
    assert lib.vba_schur_snoop_att(e.h, 0.0, 3.0, 1, 6, 3, None, None, None) == 1
    assert lib.vba_schur_snoop_att(e.h, 0.0, 3.0, 1, -1, 3, None, None, ctypes.byref(info)) == 1
    assert lib.vba_schur_outlier_power_att(None, 0.0, NCP, 3.0, *[None] * 11, ctypes.byref(info)) == 1
    assert lib.vba_schur_outlier_power_att(e.h, 0.0, NCP, 3.0, *[None] * 11, None) == 1
    for name in ("vba_schur_last_reliability_att_ms", "vba_schur_last_snoop_att_ms", "vba_schur_last_outlier_power_att_ms"):
        assert getattr(lib, name)(None, None) == 1
    assert lib.vba_schur_reliability_att(e.h, 1e-3, *nul, ctypes.byref(info)) == 0 and info.value == 0     # everything NULL but info
    assert lib.vba_schur_outlier_power_att(e.h, 1e-3, NCP, 3.0, *[None] * 11, ctypes.byref(info)) == 0 and info.value == 0
    assert e.attitude_reliability(1e-3)["info"] == 0
    e.close()


def test_a_dynamics_handle_that_asked_before_the_attitude_factor_came():
    """state_reliability allocates the reliability scratch without the attitude arrays; enabling the factor afterwards renews it."""
    from vinsat_amd._lib import PD
    d = T.case("12")
    e, f = engine(d, attitude=False), engine(d)
    assert e.state_reliability(1e-3)["info"] == 0
    c = np.ascontiguousarray(d["cumrot"])
    e._check(e.lib.vba_schur_enable_attitude(e.h, c.ctypes.data_as(PD), float(d["sigma_att"])))
    e.attitude = True
    assert _same(e.attitude_reliability(1e-3), f.attitude_reliability(1e-3))
    e.close(), f.close()


# ------------------------------------------------------------------------------------------------ 6. planted row and catalogue entry
def _converged(d):
    e = engine(d)
    hist = e.solve()
    assert any(ok for _, _, ok, _ in hist) and hist[-1][0] - hist[-1][1] <= 1e-6 * hist[-1][0]
    return e


def test_planted_row_is_suspected_and_rejected():
    from vinsat_amd.schur import gyro_suspects, suspects
    d, r = T.planted_outlier(), T.planted_reference("row")
    e = _converged(d)
    got = e.attitude_reliability(0.0)
    order = np.argsort(-got["wtest"])
    print(f"FIGURES attitude rel planted row {d['planted_row']}: first {order[:3]} {got['wtest'][order[:3]]} (oracle {r.wtest[order[0]]:.4f}) "
          f"largest landmark test {got['fit']['max_lm_wtest']:.3f} largest attitude test {got['fit']['max_att_wtest']:.3f} s0sq {got['fit']['s0sq']:.3f}")
    assert order[0] == d["planted_row"] and got["fit"]["max_wtest"] == got["wtest"][order[0]]
    crit = 0.5 * (got["wtest"][order[0]] + max(got["wtest"][order[1]], got["fit"]["max_lm_wtest"]))
    rows, lms = suspects(got, crit)
    assert np.array_equal(rows, [d["planted_row"]]) and lms.size == 0 and gyro_suspects(got, 3.29).size == 0
    rows, _ = suspects(got, crit / np.sqrt(got["fit"]["s0sq"]), scaled=True)
    assert np.array_equal(rows, [d["planted_row"]])
    res = e.attitude_snoop(0.0, crit=crit, scaled=False)
    assert (res["rows"], res["landmarks"], res["rows_via_landmarks"], res["crit_used"]) == (1, 0, 0, crit)
    mask, lm_mask = e.rejected()
    assert np.array_equal(np.nonzero(mask)[0], [d["planted_row"]]) and not lm_mask.any()
    assert e.weights()[d["planted_row"]] == 0.0 and e.last_attitude_snoop_ms() > 0.0
    e.close()


def test_moved_catalogue_entry_is_suspected_and_rejected():
    from vinsat_amd.schur import suspects
    d, r = T.displaced_landmark(), T.planted_reference("landmark")
    e = _converged(d)
    got = e.attitude_reliability(0.0)
    order = np.argsort(-np.nan_to_num(got["lm_wtest"]))
    l = d["displaced_lm"]
    print(f"FIGURES attitude rel displaced landmark {l}: first {order[:3]} {got['lm_wtest'][order[:3]]} (oracle {r.lm_wtest[l]:.4f}) "
          f"largest row test {got['fit']['max_wtest']:.3f}")
    assert order[0] == l and got["fit"]["max_lm_wtest"] == got["lm_wtest"][l]
    crit = 0.5 * (got["lm_wtest"][l] + max(got["lm_wtest"][order[1]], got["fit"]["max_wtest"]))
    rows, lms = suspects(got, crit)
    assert rows.size == 0 and np.array_equal(lms, [l])
    res = e.attitude_snoop(0.0, crit=crit, scaled=False)
    track = int((d["landmark_of_row"] == l).sum())
    assert (res["rows"], res["landmarks"], res["rows_via_landmarks"]) == (0, 1, track)
    mask, lm_mask = e.rejected()
    assert np.array_equal(np.nonzero(lm_mask)[0], [l]) and np.array_equal(mask, d["landmark_of_row"] == l)
    # the rows zeroed through the landmark: the bits of a fresh handle with those weights zeroed, and restore gives back the
    # unsnooped bits (from the same state: the comparison iterates)
    st = e.get_state()
    fresh, never = engine(d, state=st, w=np.where(mask, 0.0, d["w"])), engine(d, state=st)
    a, b = _everything(e), _everything(fresh)
    assert a[0] == b[0] and _same_cov(a[1], b[1]) and _same(a[2], b[2]) and all(np.array_equal(x, y) for x, y in zip(a[3], b[3]))
    e.restore_rejected()
    assert not e.rejected()[0].any() and not e.rejected()[1].any() and np.array_equal(e.weights(), d["w"])
    e.set_state(*st)
    a, b = _everything(e), _everything(never)
    assert a[0] == b[0] and _same_cov(a[1], b[1]) and _same(a[2], b[2]) and all(np.array_equal(x, y) for x, y in zip(a[3], b[3]))
    e.close(), fresh.close(), never.close()


def _everything(e):
    return e.iterate(1e-3), e.state_covariance(1e-3), e.attitude_reliability(1e-3), e.get_state()


def test_handle_behaves_as_a_fresh_one_with_those_weights_zeroed():
    d = T.planted_outlier()
    e = _converged(d)
    st = e.get_state()
    never = engine(d, state=st)
    rel0 = e.attitude_reliability(1e-3)
    res = e.attitude_snoop(1e-3, crit=3.29, scaled=True)
    print(f"FIGURES attitude snoop on the converged 29 / 300 with the planted row: {res}")
    assert res["info"] == 0 and res["rows"] >= 1
    assert res["crit_used"] == 3.29 * np.sqrt(rel0["fit"]["s0sq"])          # (fit[5] counts the attitude equations)
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


def test_solve_with_attitude_snoop_rejects_the_planted_row():
    d = T.planted_outlier()
    e = engine(d)
    hist = e.solve(attitude_snoop=dict(crit=6))
    rounds = [h[1] for h in hist if h[0] == "snoop"]
    print(f"FIGURES solve(attitude_snoop): rounds {rounds}")
    assert rounds and rounds[0]["rows"] >= 1 and rounds[-1]["rows"] + rounds[-1]["landmarks"] == 0
    assert e.rejected()[0][d["planted_row"]]
    e.close()


# ------------------------------------------------------------------------------------------------ 7. gyro fault
def test_gyro_fault_is_the_one_suspect():
    """One gap rotation of 29 / 300 turned by schur_att_rel_cases.GYRO_ANGLE, fitted to convergence: gyro_suspects names exactly that
    edge (tests/test_schur_att_rel_host.py holds the reference's own margin); the snoop reports and rejects no edge."""
    from vinsat_amd.schur import gyro_suspects
    d, r = T.gyro_fault(), T.planted_reference("gyro")
    e = _converged(d)
    got = e.attitude_reliability(0.0)
    order = np.argsort(-got["att_wtest"])
    k = d["gyro_edge"]
    print(f"FIGURES gyro fault edge {k}: first {order[:3]} {got['att_wtest'][order[:3]]} (oracle {r.att_wtest[order[:3]]}) s0sq {got['fit']['s0sq']:.4f} "
          f"largest row test {got['fit']['max_wtest']:.3f}")
    assert got["info"] == 0 and np.all(np.isfinite(got["att_wtest"]))
    assert np.array_equal(gyro_suspects(got, 3.29), [k]) and np.array_equal(gyro_suspects(got, 3.29, scaled=True), [k])
    assert order[0] == k and got["fit"]["max_att_wtest"] == got["att_wtest"][k]
    w = e.weights()
    e.attitude_snoop(0.0, crit=float("inf"))
    assert np.array_equal(e.weights(), w)
    e.close()


# ------------------------------------------------------------------------------------------------ 8. outlier power
@pytest.mark.parametrize("name,lam", T.POWER_CASES)
def test_outlier_power_matches_the_reference(name, lam):
    r, d = T.power_reference(name, lam), T.case(name)
    e = engine(d)
    crit = 1.0
    got = e.attitude_outlier_power(lam, NCP, crit)
    rel = e.attitude_reliability(lam)
    assert got["info"] == 0 and e.last_attitude_outlier_power_ms() > 0.0
    fig = PW.figures(got, r)
    print(f"FIGURES attitude power {name} lam={lam:g} " + " ".join(f"{k}={fig[k]:.2e} (bar {PW.bar(r, k):.1e})" for k in PW.FAMILIES) +
          f" rows left out {r.left_out} of {r.kept.size}, landmarks {r.lm_left_out} of {r.lm_kept.size}")
    for k in PW.ROW_FAMILIES:
        assert np.all(np.isfinite(got[k][r.kept])), k
    for k in PW.LM_FAMILIES:
        assert np.all(np.isfinite(got[k][r.lm_kept])), k
    for k in PW.FAMILIES:
        assert fig[k] <= PW.bar(r, k), k
    # fit[0:13] and pose_fit[:, 1] carry the bits of attitude_reliability; the four slots behind them against the device's own arrays
    fit, rfit = list(got["fit"].values()), list(rel["fit"].values())
    assert len(fit) == 17 and list(got["fit"])[10:13] == ["t_att", "omega_att", "max_att_wtest"]
    assert np.array(fit[:13]).tobytes() == np.array(rfit).tobytes()
    assert got["pose_fit"][:, 1].tobytes() == np.ascontiguousarray(rel["pose_stats"][:, 0]).tobytes()
    with np.errstate(invalid="ignore"):
        over, lm_over = rel["wtest"] > crit, rel["lm_wtest"] > crit
    fin = lambda a: float(np.max(a[np.isfinite(a)], initial=0.0))
    assert fit[13] == float(over.sum()) and fit[15] == float(lm_over.sum())
    assert fit[14] == fin(got["ext_pos"]) and fit[16] == fin(got["lm_del_pos"])
    assert np.array_equal(got["pose_fit"][:, 3], np.bincount(d["pose_of_row"], weights=over.astype(float), minlength=e.n))
    from vinsat_amd.schur import scaled_power
    assert scaled_power(got)["s0"] == np.sqrt(rel["fit"]["s0sq"])
    e.close()
