"""The orbit-dynamics factor of the free-landmark mode on the GPU (``SchurBA(..., time_idx=, sigma_dyn=)``,
``vba_schur_enable_dynamics``, vinsat_amd/csrc/vba_schur_dyn.hip) against tests/schur_dyn_oracle.py.  PARITY UNPINNED as the rest of
the add-on.  Cases and why each is there: tests/schur_dyn_cases.py (12 / 150, 29 / 300, 43 / 450 with a pose without rows,
86 / 900 with four panels and a full tile band).

Bars.  The factor (r, D Phi) answers to tests/dynamics_reference.py exactly as the fixed-landmark path's does in
tests/test_gpu_dynamics_paths.py: ``factor_layer`` against the longdouble chain, K x 2^-53 with K = max(16, 4 x the fp64 NumPy
oracle's figure on the same case).  (``factor_layer`` takes Phi: D Phi is divided by D in fp64 first, half a unit at most.)  One
trial answers to the bars of DESIGN 9, relative to the largest entry: c0 1e-10; c1, dc, dl 1e-7 and dv the bar of dc; Lg Lg^T 1e-11;
Lg 1e-8; states 1e-9.  The oracle's two-route floor is below a tenth of each step bar on every case
(tests/test_schur_dyn_host.py).  Floors and the device's figures on the MI355X: DESIGN 9.5.
"""
import numpy as np
import pytest

import dynamics_reference as R
import schur_dyn_cases as C
import schur_dyn_oracle as D
from oracle import ba_oracle as O

pytestmark = pytest.mark.gpu

ORBIT = ("xhat_p", "xhat_v", "Phi_p", "Phi_v", "r_orbit")
D6 = R.D6


def engine(d, dynamics=True, sigma_dyn=None, time_idx=None, states=None):
    from vinsat_amd.schur import SchurBA
    kw = {}
    if dynamics:
        kw = dict(time_idx=d["time_idx"] if time_idx is None else time_idx, sigma_dyn=d["sigma_dyn"] if sigma_dyn is None else sigma_dyn)
    e = SchurBA(d["states0"] if states is None else states, d["X0"], d["uv"], d["w"], d["pose_of_row"], d["landmark_of_row"], d["intrinsics"],
                sigma_prior=d["sigma"], **kw)
    e.set_state(d["states0"] if states is None else states, d["Xs"])
    return e


def orbit_figures(states, time_idx, r, Phi):
    """The orbit figures of ``dynamics_reference.factor_layer`` (no attitude in this mode: identity rotations, zero attitude terms)."""
    n = states.shape[0]
    cumrot = np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (n, 1))
    Phi_n = np.zeros((n, 6, 6))
    Phi_n[:-1] = Phi
    r7 = np.concatenate([r, np.zeros((n - 1, 1))], 1)
    figs, _exact = R.factor_layer(states, time_idx, cumrot, Phi_n, r7, np.zeros((n, 3)), np.zeros((n, 3, 3, 3)))
    assert np.isfinite(Phi).all() and np.isfinite(r).all()
    return {k: figs[k] for k in ORBIT}


@pytest.mark.parametrize("name", C.NAMES)
def test_factor_against_the_longdouble_chain(name):
    d = C.case(name)
    st, t = d["states0"], d["time_idx"]
    e = engine(d)
    e.iterate(1e-3)
    r, A = e.dynamics_residual(), e.dynamics_jacobian()
    ec = e.dynamics_edge_cost()
    e.close()
    ro, Eo, _F = O.orbit_factor(st, t, jacobian=True)
    Phi_o = np.concatenate([Eo[:, :, 0:3], Eo[:, :, 6:9]], -1) / D6[None, :, None]
    lv = R.Levels(R._units(orbit_figures(st, t, ro, Phi_o)))
    v = R.judge(lv, orbit_figures(st, t, r, A / D6[None, :, None]))
    print(f"FACTOR {name}: " + " ".join(f"{k}={v.units[k]:.2f}/{lv.units[k]:.2f}" for k in v.units))
    assert v.ok, v.failures
    assert np.abs(ec - d["sigma_dyn"] * (r * r).sum(1)).max() <= 1e-14 * np.abs(ec).max()


@pytest.mark.parametrize("lam", C.LAMS)
@pytest.mark.parametrize("name", C.NAMES)
def test_one_trial_matches_the_oracle(name, lam):
    d, ref = C.case(name), C.reference(name, lam)
    n, B = d["states0"].shape[0], C.BARS
    e = engine(d)
    c0, c1, ok = e.iterate(lam)
    assert e.last_info() == 0
    dc, dl = e.last_step()
    dv = e.last_velocity_step()
    Lg = e.cholesky_factor()
    st, X = e.get_state()
    e.close()
    assert Lg.shape == (9 * n, 9 * n)
    fig = dict(c0=abs(c0 - ref.c0) / ref.c0, c1=abs(c1 - ref.c1) / ref.c1, dc=C.rel(dc, ref.dc), dv=C.rel(dv, ref.dv), dl=C.rel(dl, ref.dl),
               LLt=C.rel(Lg @ Lg.T, ref.Sm), L=C.rel(Lg, ref.Lc), states=max(C.rel(st, ref.st), C.rel(X, ref.X)))
    print(f"TRIAL {name} lam={lam:g}: " + " ".join(f"{k}={v:.1e}" for k, v in fig.items()))
    assert ok == ref.ok and ok
    bad = {k: v for k, v in fig.items() if not v <= B[k]}
    assert not bad, bad
    # the velocities moved by dv, the rest of the state as on a plain handle
    assert np.array_equal(st[:, 7:10], d["states0"][:, 7:10] + dv)


def test_pose_without_rows_is_held_by_the_dynamics():
    """Pose 20 of 43 / 450 has no row: its position and velocity step come from the two edges alone, and are no smaller for it."""
    d, ref = C.case("43"), C.reference("43", 1e-3)
    i = C.EMPTY_POSE["43"]
    assert not np.any(d["pose_of_row"] == i)
    e = engine(d)
    e.iterate(1e-3)
    dc, _ = e.last_step()
    dv = e.last_velocity_step()
    e.close()
    assert np.abs(ref.dc[i, :3]).max() > 0.1 and np.abs(ref.dv[i]).max() > 1e-4        # km, km/s: a real step, not the damping's zero
    assert np.abs(dc[i] - ref.dc[i]).max() <= 1e-7 * np.abs(ref.dc).max() and np.abs(dv[i] - ref.dv[i]).max() <= 1e-7 * np.abs(ref.dv).max()


@pytest.mark.parametrize("name", ("29", "86"))
def test_tiny_sigma_dyn_gives_the_plain_step(name):
    d = C.case(name)
    a, b = engine(d, sigma_dyn=1e-30), engine(d, dynamics=False)
    ra, rb = a.iterate(1e-3), b.iterate(1e-3)
    (dca, dla), (dcb, dlb) = a.last_step(), b.last_step()
    dv = a.last_velocity_step()
    a.close(), b.close()
    print(f"CONTINUITY {name}: dc {C.rel(dca, dcb):.1e} dl {C.rel(dla, dlb):.1e} |dv| {np.abs(dv).max():.1e}")
    assert C.rel(dca, dcb) <= C.BARS["dc"] and C.rel(dla, dlb) <= C.BARS["dl"]
    assert abs(ra[0] - rb[0]) <= 1e-10 * rb[0] and abs(ra[1] - rb[1]) <= 1e-7 * rb[1]


@pytest.mark.parametrize("name", ("29", "86"))
def test_two_iterates_and_two_handles_give_the_same_bits(name):
    d = C.case(name)

    def run(e):
        e.set_state(d["states0"], d["Xs"])
        c = e.iterate(1e-3)
        return c, e.last_step(), e.last_velocity_step(), e.cholesky_factor(), e.get_state(), e.dynamics_residual(), e.dynamics_jacobian()

    a, b = engine(d), engine(d)
    runs = [run(a), run(a), run(b)]
    a.close(), b.close()

    def flat(x):
        return np.concatenate([np.ravel(np.asarray(v, dtype=np.float64)) for v in (x[0], *x[1], x[2], x[3], *x[4], x[5], x[6])])

    for other in runs[1:]:
        assert np.array_equal(flat(runs[0]), flat(other))


def test_lm_loop_follows_the_oracle_trial_for_trial():
    """29 / 300: an arc of 400 s.  (On the 11 s arc of 12 / 150 the velocity is not observable to the 2 m/s of the start's
    perturbation -- a pixel is 130 m on the ground -- and the fit ends further from the truth than it started, oracle and device alike.)"""
    d = C.case("29")
    t, sd = d["time_idx"], d["sigma_dyn"]
    e = engine(d)
    hist = e.solve(lamda0=1e-4, max_iters=8)
    st1, _ = e.get_state()
    accepted = [h for h in hist if h[2]]
    assert len(accepted) >= 2
    assert all(h[1] < h[0] for h in accepted)
    assert all(accepted[k + 1][0] == accepted[k][1] for k in range(len(accepted) - 1))     # the next trial starts at the accepted cost
    v_err = lambda s: np.abs(s[:, 7:10] - d["states_gt"][:, 7:10]).max()
    print(f"LM 29: cost {hist[0][0]:.6g} -> {accepted[-1][1]:.6g}, velocity error {v_err(d['states0']):.2e} -> {v_err(st1):.2e} km/s")
    assert v_err(st1) < v_err(d["states0"])
    # the oracle's loop at the device's own damping sequence and accept decisions, trial for trial
    st, X = d["states0"], d["Xs"]
    for k, (c0, c1, ok, lam) in enumerate(hist):
        dc9, dl, _, _ = D.step_schur(*D.normal_equations(st, X, *C.args(d), lam, t, sd))
        s1, X1 = D.apply_step(st, X, dc9, dl)
        r0, r1 = D.cost(st, X, *C.args(d), t, sd), D.cost(s1, X1, *C.args(d), t, sd)
        assert abs(c0 - r0) <= 1e-7 * r0 and abs(c1 - r1) <= 1e-7 * r1, (k, c0, r0, c1, r1)
        if ok:                                      # the device's decision moves both: a tie at convergence cannot fork the comparison
            st, X = s1, X1
    assert C.rel(st1, st) <= 1e-7
    # the robust loop runs on a dynamics handle: rows only
    e.set_state(d["states0"], d["Xs"])
    rh = e.solve(lamda0=1e-4, max_iters=4, robust=dict(outer=2))
    assert sum(1 for h in rh if h[0] == "reweight") == 2 and any(h[2] for h in rh if h[0] != "reweight")
    assert e.weights().shape == d["w"].shape and np.isfinite(e.get_state()[0]).all()
    e.close()


def test_refusals_leave_the_handle_usable():
    from vinsat_amd._lib import VbaError
    d = C.case("12")
    e = engine(d)
    first = e.iterate(1e-3)
    for call in (lambda: e.covariance(), lambda: e.reliability(), lambda: e.snoop(), lambda: e.solve(max_iters=1, snoop=dict(rounds=1))):
        with pytest.raises(VbaError, match="not available on a handle with the dynamics factor"):
            call()
    e.set_state(d["states0"], d["Xs"])
    assert e.iterate(1e-3) == first
    e.close()
    n = d["states0"].shape[0]
    t = d["time_idx"].copy()
    t[5:] += 64                                     # gap 65 between poses 4 and 5
    with pytest.raises(VbaError, match="gap of 65 steps"):
        engine(d, time_idx=t)
    t = d["time_idx"].copy()
    t[5] = t[4]                                     # gap 0
    with pytest.raises(VbaError, match="time_idx must increase"):
        engine(d, time_idx=t)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(VbaError, match="sigma_dyn must be positive and finite"):
            engine(d, sigma_dyn=bad)
    from vinsat_amd.schur import SchurBA
    a = (d["states0"], d["X0"], d["uv"], d["w"], d["pose_of_row"], d["landmark_of_row"], d["intrinsics"])
    with pytest.raises(ValueError, match="both or neither"):
        SchurBA(*a, time_idx=d["time_idx"])
    with pytest.raises(ValueError, match="both or neither"):
        SchurBA(*a, sigma_dyn=1.0)
    with pytest.raises(ValueError, match="one entry per pose"):
        SchurBA(*a, time_idx=d["time_idx"][:-1], sigma_dyn=1.0)
    # one pose: nothing to tie
    keep = d["pose_of_row"] == 0
    with pytest.raises(VbaError, match="at least two poses"):
        SchurBA(d["states0"][:1], d["X0"], d["uv"][keep], d["w"][keep], d["pose_of_row"][keep], d["landmark_of_row"][keep], d["intrinsics"][:1],
                time_idx=d["time_idx"][:1], sigma_dyn=1.0)
    # ... and a handle built after all that works
    e = engine(d)
    assert e.iterate(1e-3) == first
    e.close()


def test_plain_handle_keeps_its_sizes_and_layouts():
    from vinsat_amd._lib import VbaError
    d = C.case("12")
    n, L = d["states0"].shape[0], d["X0"].shape[0]
    e = engine(d, dynamics=False)
    e.iterate(1e-3)
    assert e.cholesky_factor().shape == (6 * n, 6 * n)
    dc, dl = e.last_step()
    assert dc.shape == (n, 6) and dl.shape == (L, 3)
    st, _ = e.get_state()
    assert np.array_equal(st[:, 7:10], d["states0"][:, 7:10])          # velocities carried through
    for fetch in (e.last_velocity_step, e.dynamics_residual, e.dynamics_jacobian):
        with pytest.raises(VbaError, match="dynamics factor is not enabled"):
            fetch()
    assert e.covariance()["info"] == 0
    e.close()
