"""The dynamics factor of the free-landmark mode ACROSS LONG GAPS on the GPU (``SchurBA(..., long_gaps=True)``,
``vba_schur_enable_dynamics_long``, vinsat_amd/csrc/vba_schur_dyn_long.hip): edges of more than 64 s propagated parallel in time.
PARITY UNPINNED as the rest of the add-on.  Cases and why each is there: tests/schur_dyn_long_cases.py.

Bars.  A LONG edge's factor answers to the exact chain of tests/exact_orbit.py per edge and per component (x_hat position and
velocity, the position and the velocity columns of Phi) at the bar of ``test_gpu_long_gaps._check_factor_exact``: device error
<= 16 x (error of ``O.propagate_orbit``) + 2^-46.  The SHORT edges of the same windows answer to ``dynamics_reference.factor_layer``
with K = max(16, 4 x oracle) as in tests/test_gpu_schur_dyn.py.  One trial answers to ``schur_dyn_cases.BARS``; the oracle's floors
are below a tenth of each step bar (tests/test_schur_dyn_long_host.py).  The state covariance and the trial with the attitude factor
on top answer to the bars of tests/test_gpu_schur_dyn_cov.py and tests/test_gpu_schur_att.py.  Figures on the MI355X: DESIGN 9.12.
"""
import contextlib
import os

import numpy as np
import pytest

import dynamics_reference as R
import exact_orbit as X
import schur_dyn_cases as C
import schur_dyn_long_cases as L
import schur_dyn_oracle as D
from oracle import ba_oracle as O

pytestmark = pytest.mark.gpu

ORBIT = ("xhat_p", "xhat_v", "Phi_p", "Phi_v", "r_orbit")
D6 = L.D6


@contextlib.contextmanager
def serial_fallback():
    """VBA_SCHUR_LONG_SERIAL=1 while a handle is built (read when the factor is enabled)."""
    old = os.environ.get("VBA_SCHUR_LONG_SERIAL")
    os.environ["VBA_SCHUR_LONG_SERIAL"] = "1"
    try:
        yield
    finally:
        if old is None:
            del os.environ["VBA_SCHUR_LONG_SERIAL"]
        else:
            os.environ["VBA_SCHUR_LONG_SERIAL"] = old


def engine(d, long_gaps=True, **kw):
    from vinsat_amd.schur import SchurBA
    kw.setdefault("time_idx", d["time_idx"])
    kw.setdefault("sigma_dyn", d["sigma_dyn"])
    e = SchurBA(d["states0"], d["X0"], d["uv"], d["w"], d["pose_of_row"], d["landmark_of_row"], d["intrinsics"], sigma_prior=d["sigma"],
                long_gaps=long_gaps, **kw)
    e.set_state(d["states0"], d["Xs"])
    return e


def long_edge_ratio(key, d, r, A, what):
    """The long edges of ``r``, ``A`` (made at ``states0``) against the exact chain; the largest error / bar met."""
    e, steps, xe, Pe, ora = L.exact_long_edges(key)
    st = d["states0"]
    x = np.concatenate([st[:, :3], st[:, 7:]], -1)
    gpu = X.edge_errors(x[e + 1] + r[e] / D6, A[e] / D6[None, :, None], xe, Pe)
    worst = 0.0
    for name, eg, eo in zip(("x_hat pos", "x_hat vel", "Phi pos cols", "Phi vel cols"), gpu, ora):
        bar = L.EXACT_FACTOR * eo + L.EXACT_SLACK
        worst = max(worst, float((eg / bar).max()))
        bad = np.nonzero(~(eg <= bar))[0]
        assert not bad.size, (what, name, [(int(e[k]), int(steps[k]), float(eg[k]), float(eo[k])) for k in bad])
    return worst


def orbit_figures(states, time_idx, r, Phi):
    n = states.shape[0]
    cumrot = np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (n, 1))
    Phi_n = np.zeros((n, 6, 6))
    Phi_n[:-1] = Phi
    r7 = np.concatenate([r, np.zeros((n - 1, 1))], 1)
    figs, _exact = R.factor_layer(states, time_idx, cumrot, Phi_n, r7, np.zeros((n, 3)), np.zeros((n, 3, 3, 3)))
    return {k: figs[k] for k in ORBIT}


def check_factor(key, d, e, what):
    """r, A, ecost of the last build of ``e`` (made at ``states0``): long edges against the exact chain, short ones against the
    longdouble chain at the bars of the short-gap mode."""
    st, t = d["states0"], d["time_idx"]
    r, A, ec = e.dynamics_residual(), e.dynamics_jacobian(), e.dynamics_edge_cost()
    assert np.isfinite(r).all() and np.isfinite(A).all()
    worst = long_edge_ratio(key, d, r, A, what)
    ro, Eo, _F = O.orbit_factor(st, t, jacobian=True)
    Phi_o = np.concatenate([Eo[:, :, 0:3], Eo[:, :, 6:9]], -1) / D6[None, :, None]
    lv = R.Levels(R._units(orbit_figures(st, t, ro, Phi_o)))
    v = R.judge(lv, orbit_figures(st, t, r, A / D6[None, :, None]))
    print(f"FACTOR {what}: exact-chain ratio {worst:.3f}; short edges " + " ".join(f"{k}={v.units[k]:.2f}/{lv.units[k]:.2f}" for k in v.units))
    assert v.ok, v.failures
    assert np.abs(ec - d["sigma_dyn"] * (r * r).sum(1)).max() <= 1e-14 * np.abs(ec).max()
    return r, A


def trial_figures(e, ref, lam):
    c0, c1, ok = e.iterate(lam)
    assert e.last_info() == 0
    dc, dl = e.last_step()
    dv = e.last_velocity_step()
    Lg = e.cholesky_factor()
    st, Xl = e.get_state()
    fig = dict(c0=abs(c0 - ref.c0) / ref.c0, c1=abs(c1 - ref.c1) / ref.c1, dc=C.rel(dc, ref.dc), dv=C.rel(dv, ref.dv), dl=C.rel(dl, ref.dl),
               LLt=C.rel(Lg @ Lg.T, ref.Sm), L=C.rel(Lg, ref.Lc), states=max(C.rel(st, ref.st), C.rel(Xl, ref.X)))
    return fig, ok, (c0, c1, dc, dv, dl)


# ------------------------------------------------------------------------------------------------ 1. the factor
@pytest.mark.parametrize("gaps", L.FACTOR_GAPS, ids=["threshold", "mixed", "over-1024", "3000s", "plan-edge"])
def test_factor_of_windows_around_every_rule_of_the_partition(gaps):
    d = L.factor_window(gaps)
    e = engine(d)
    assert list(e.long_edges()) == list(d["long"])
    e.iterate(1e-3)
    check_factor(gaps, d, e, gaps)
    e.close()


@pytest.mark.parametrize("name", L.NAMES)
def test_factor_of_the_trial_cases(name):
    d = L.case(name)
    e = engine(d)
    assert list(e.long_edges()) == list(d["long"])
    e.iterate(1e-3)
    check_factor(name, d, e, name)
    e.close()


# ------------------------------------------------------------------------------------------------ 2. one trial
@pytest.mark.parametrize("lam", L.LAMS)
@pytest.mark.parametrize("name", L.NAMES)
def test_one_trial_matches_the_oracle(name, lam):
    d, ref = L.case(name), L.reference(name, lam)
    e = engine(d)
    fig, ok, (_, _, _, dv, _) = trial_figures(e, ref, lam)
    st, _ = e.get_state()
    e.close()
    print(f"TRIAL {name} lam={lam:g}: " + " ".join(f"{k}={v:.1e}" for k, v in fig.items()))
    assert ok == ref.ok and ok
    bad = {k: v for k, v in fig.items() if not v <= L.BARS[k]}
    assert not bad, bad
    assert np.array_equal(st[:, 7:10], d["states0"][:, 7:10] + dv)


# ------------------------------------------------------------------------------------------------ 3. against the serial fallback
def test_parallel_in_time_against_the_serial_fallback():
    d, ref = L.case("L12"), L.reference("L12", 1e-3)
    par = engine(d)
    with serial_fallback():
        ser = engine(d)
    assert list(par.long_edges()) == list(d["long"]) and ser.long_edges().size == 0
    fp, okp, (c0p, c1p, dcp, dvp, dlp) = trial_figures(par, ref, 1e-3)
    fs, oks, (c0s, c1s, dcs, dvs, dls) = trial_figures(ser, ref, 1e-3)
    rp, Ap = check_factor("L12", d, par, "L12 parallel")
    rs, As = check_factor("L12", d, ser, "L12 serial")             # the serial lanes' long edges meet the same exact-chain bar
    par.close(), ser.close()
    print("SERIAL L12: " + " ".join(f"{k}={v:.1e}" for k, v in fs.items()))
    assert okp and oks
    for fig in (fp, fs):
        bad = {k: v for k, v in fig.items() if not v <= L.BARS[k]}
        assert not bad, bad
    B = L.BARS
    assert abs(c0p - c0s) <= B["c0"] * c0s and abs(c1p - c1s) <= B["c1"] * c1s
    assert C.rel(dcp, dcs) <= B["dc"] and C.rel(dvp, dvs) <= B["dv"] and C.rel(dlp, dls) <= B["dl"]
    short = np.setdiff1d(np.arange(rp.shape[0]), d["long"])
    assert np.array_equal(rp[short], rs[short]) and np.array_equal(Ap[short], As[short])        # bit for bit
    lg = d["long"]
    print(f"SERIAL L12 long edges: r {np.abs(rp[lg] - rs[lg]).max():.2e} A {C.rel(Ap[lg], As[lg]):.2e}")


# ------------------------------------------------------------------------------------------------ 4. no long gap, no change
def _everything(e, d, lam=1e-3):
    e.set_state(d["states0"], d["Xs"])
    c = e.iterate(lam)
    return np.concatenate([np.ravel(np.asarray(v, dtype=np.float64)) for v in
                           (c, *e.last_step(), e.last_velocity_step(), e.cholesky_factor(), *e.get_state(), e.dynamics_residual(),
                            e.dynamics_jacobian(), e.dynamics_edge_cost())])


def test_no_long_gap_no_change():
    d = C.case("29")
    new, old = engine(d), engine(d, long_gaps=False)
    assert new.long_edges().size == 0 and old.long_edges().size == 0
    a, b = _everything(new, d), _everything(old, d)
    new.close(), old.close()
    assert np.array_equal(a, b)


def test_refusals_leave_the_handle_usable():
    from vinsat_amd._lib import VbaError
    d = C.case("12")
    t = d["time_idx"].copy()
    t[5:] += 64                                     # gap 65 between poses 4 and 5
    with pytest.raises(VbaError, match="gap of 65 steps between poses 4 and 5: the dynamics factor of this mode covers gaps of 1 .. 64 steps"):
        engine(d, long_gaps=False, time_idx=t)
    ok65 = engine(d, time_idx=t)                    # ... which the new entry takes
    assert list(ok65.long_edges()) == [4]
    ok65.close()
    t = d["time_idx"].astype(np.int64)
    t[5:] += 2 ** 20                                # gap VBA_MAX_GAP + 1
    with pytest.raises(VbaError, match="between poses 4 and 5: longer than VBA_MAX_GAP"):
        engine(d, time_idx=t)
    t = d["time_idx"].copy()
    t[5] = t[4]
    with pytest.raises(VbaError, match="time_idx must increase"):
        engine(d, time_idx=t)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(VbaError, match="sigma_dyn must be positive and finite"):
            engine(d, sigma_dyn=bad)
    # the C entry on a live handle: refused, and the handle is as usable as before (no factor yet: a plain trial runs, then the factor)
    import ctypes
    from vinsat_amd.schur import SchurBA
    p = SchurBA(d["states0"], d["X0"], d["uv"], d["w"], d["pose_of_row"], d["landmark_of_row"], d["intrinsics"], sigma_prior=d["sigma"])
    p.set_state(d["states0"], d["Xs"])
    bad_t = np.ascontiguousarray(t, dtype=np.int32)
    ptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    assert p.lib.vba_schur_enable_dynamics_long(p.h, ptr(bad_t), 1e4) != 0
    assert p.lib.vba_schur_enable_dynamics_long(p.h, ptr(d["time_idx"]), float("nan")) != 0
    plain = engine(d, long_gaps=False)
    first = plain.iterate(1e-3)
    plain.close()
    assert p.lib.vba_schur_enable_dynamics_long(p.h, ptr(np.ascontiguousarray(d["time_idx"], dtype=np.int32)), d["sigma_dyn"]) == 0
    p.dynamics = True
    p.set_state(d["states0"], d["Xs"])
    assert p.iterate(1e-3) == first
    p.close()


# ------------------------------------------------------------------------------------------------ 5. carried chain
def test_carried_chain_has_the_bits_of_a_recomputed_one():
    d = L.case("L12")
    a = engine(d)
    hist = a.solve(lamda0=1e-4, max_iters=6)
    assert any(h[2] for h in hist)
    st, Xl = a.get_state()
    b = engine(d)
    b.set_state(st, Xl)                             # fresh pools: every chain is walked anew
    ca, cb = a.iterate(1e-3), b.iterate(1e-3)       # a: the seventh iterate, its chains carried from the accepted trials
    assert ca == cb
    assert np.array_equal(a.dynamics_residual(), b.dynamics_residual()) and np.array_equal(a.dynamics_jacobian(), b.dynamics_jacobian())
    assert np.array_equal(a.get_state()[0], b.get_state()[0])
    a.close(), b.close()


def test_two_runs_and_two_handles_give_the_same_bits():
    d = L.case("L12")
    a, b = engine(d), engine(d)
    runs = [_everything(a, d), _everything(a, d), _everything(b, d)]
    a.close(), b.close()
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])


# ------------------------------------------------------------------------------------------------ 6. LM loop
def test_lm_loop_follows_the_oracle_trial_for_trial():
    d = L.case("L29")
    t, sd = d["time_idx"], d["sigma_dyn"]
    e = engine(d)
    hist = e.solve(lamda0=1e-4, max_iters=8)
    st1, _ = e.get_state()
    e.close()
    accepted = [h for h in hist if h[2]]
    assert len(accepted) >= 2
    assert all(h[1] < h[0] for h in accepted)
    assert all(accepted[k + 1][0] == accepted[k][1] for k in range(len(accepted) - 1))     # the next trial starts at the accepted cost
    v_err = lambda s: np.abs(s[:, 7:10] - d["states_gt"][:, 7:10]).max()
    print(f"LM L29: cost {hist[0][0]:.6g} -> {accepted[-1][1]:.6g}, velocity error {v_err(d['states0']):.2e} -> {v_err(st1):.2e} km/s")
    assert v_err(st1) < v_err(d["states0"])
    st, Xl = d["states0"], d["Xs"]
    for k, (c0, c1, ok, lam) in enumerate(hist):
        dc9, dl, _, _ = D.step_schur(*D.normal_equations(st, Xl, *L.args(d), lam, t, sd))
        s1, X1 = D.apply_step(st, Xl, dc9, dl)
        r0, r1 = D.cost(st, Xl, *L.args(d), t, sd), D.cost(s1, X1, *L.args(d), t, sd)
        assert abs(c0 - r0) <= 1e-7 * r0 and abs(c1 - r1) <= 1e-7 * r1, (k, c0, r0, c1, r1)
        if ok:
            st, Xl = s1, X1
    assert C.rel(st1, st) <= 1e-7


# ------------------------------------------------------------------------------------------------ 7. downstream consumers
def test_state_covariance_on_a_long_gap_handle():
    import schur_dyn_cov_cases as V
    d = L.case("L12")
    e = engine(d)
    for lam in (0.0, 1e-3):
        r = L.cov_reference("L12", lam)
        c = e.state_covariance(lam, pairs=True)
        assert c["info"] == 0
        bi, bj, blocks = c["pairs"]
        assert np.array_equal(bi, r.blk_i) and np.array_equal(bj, r.blk_j)
        got = dict(state=c["state"], edges=c["edges"], pairs=blocks, landmark=c["landmark"])
        fig = V.scaled(got, r)
        print(f"FIGURES state cov L12 lam={lam:g} " + " ".join(f"{k}={fig[k]:.2e} (floor {r.floor[k]:.1e}, bar {V.bar(r, k):.1e})" for k in V.FAMILIES))
        for k in V.FAMILIES:
            assert np.all(np.isfinite(got[k])) and fig[k] <= V.bar(r, k), k
    e.close()


@pytest.mark.parametrize("lam", L.LAMS)
def test_one_trial_with_the_attitude_factor_on_top(lam):
    d, ref = L.att_case("L12"), L.att_reference("L12", lam)
    e = engine(d, cumrot=d["cumrot"], sigma_att=d["sigma_att"])
    fig, ok, _ = trial_figures(e, ref, lam)
    e.close()
    print(f"TRIAL att L12 lam={lam:g}: " + " ".join(f"{k}={v:.1e}" for k, v in fig.items()))
    assert ok == ref.ok and ok
    bad = {k: v for k, v in fig.items() if not v <= L.BARS[k]}
    assert not bad, bad
