"""The Gauss-Newton attitude factor of the free-landmark mode on the GPU (``SchurBA(..., cumrot=, sigma_att=)``,
``vba_schur_enable_attitude``, vinsat_amd/csrc/vba_schur_att.hip) against tests/schur_att_oracle.py.  PARITY UNPINNED as the rest of
the add-on.  Cases: tests/schur_att_cases.py (those of the orbit factor, and the sign variant ``12s`` with d < 0 on two edges).

Bars.  a, J and the edge costs answer componentwise to ``max(16, 4 x the float64 oracle's own error against its longdouble
restatement)`` units of 2^-53 of the largest entry (``schur_att_cases.edge_bars``; the oracle's figures are recorded in
tests/test_schur_att_host.py), as DESIGN 9.5 derives the orbit factor's.  One trial answers to ``schur_dyn_cases.BARS``.  The
oracle's two-route floor is below a tenth of each step bar on every case (tests/test_schur_att_host.py).  The state covariance
answers to the bar of tests/test_gpu_schur_dyn_cov.py: ``max(100 x floor, 1e-11)`` per family, every entry scaled by the reference
sigmas of its row and column.  Floors and the device's figures on the MI355X: DESIGN 9.9.
"""
import ctypes

import numpy as np
import pytest

import schur_att_cases as C
import schur_att_oracle as A
import schur_dyn_cov_cases as V

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def engine(d, attitude=True, sigma_att=None, cumrot=None, states=None):
    from vinsat_amd.schur import SchurBA
    kw = dict(time_idx=d["time_idx"], sigma_dyn=d["sigma_dyn"])
    if attitude:
        kw.update(cumrot=d["cumrot"] if cumrot is None else cumrot, sigma_att=d["sigma_att"] if sigma_att is None else sigma_att)
    st = d["states0"] if states is None else states
    e = SchurBA(st, d["X0"], d["uv"], d["w"], d["pose_of_row"], d["landmark_of_row"], d["intrinsics"], sigma_prior=d["sigma"], **kw)
    e.set_state(st, d["Xs"])
    return e


def trial(e, lam):
    """Everything one iterate leaves, flat."""
    c = e.iterate(lam)
    parts = [c, *e.last_step(), e.last_velocity_step(), e.cholesky_factor(), *e.get_state()]
    return np.concatenate([np.ravel(np.asarray(p, dtype=np.float64)) for p in parts])


@pytest.mark.parametrize("name", C.NAMES)
def test_edges_against_the_oracle_componentwise(name):
    d = C.case(name)
    a_o, J_o, ec_o, units = C.edge_reference(name)
    bars = C.edge_bars(name)
    e = engine(d)
    e.iterate(1e-3)
    got = dict(a=e.attitude_residual(), J=e.attitude_jacobian(), ecost=e.attitude_edge_cost())
    e.close()
    ref = dict(a=a_o, J=J_o, ecost=ec_o)
    fig = {k: float(np.abs(got[k] - ref[k]).max() / np.abs(ref[k]).max() / U) for k in ref}
    print(f"EDGES {name}: " + " ".join(f"{k}={fig[k]:.1f}/{bars[k]:.0f} (oracle {units[k]:.1f})" for k in fig))
    assert got["a"].shape == a_o.shape and got["J"].shape == J_o.shape and got["ecost"].shape == ec_o.shape
    assert all(np.isfinite(v).all() for v in got.values())
    bad = {k: v for k, v in fig.items() if not v <= bars[k]}
    assert not bad, bad
    # the edge cost is sigma_att |a|^2 of the device's own a
    assert np.abs(got["ecost"] - d["sigma_att"] * (got["a"] ** 2).sum(1)).max() <= 1e-14 * np.abs(got["ecost"]).max()


@pytest.mark.parametrize("lam", C.LAMS)
@pytest.mark.parametrize("name", C.NAMES)
def test_one_trial_matches_the_oracle(name, lam):
    """The sign variant included: its step is that of 12 / 150 (q and -q are one rotation), through s = -1 on edges 0 and 1."""
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


def test_sign_variant_takes_the_negative_branch():
    d, plain = C.case(C.SIGN_VARIANT), C.case("12")
    e, f = engine(d), engine(plain)
    e.iterate(1e-3), f.iterate(1e-3)
    a, J, (dc, dl) = e.attitude_residual(), e.attitude_jacobian(), e.last_step()
    a0, J0, (dc0, dl0) = f.attitude_residual(), f.attitude_jacobian(), f.last_step()
    e.close(), f.close()
    a_o, J_o, _ = A.edge_terms(d["states0"][:, 3:7], d["cumrot"])
    # the oracle's a and J of the variant are those of 12 / 150 up to rounding (s e is even in q_1) ...
    assert np.abs(a - a0).max() <= 1e-12 * np.abs(a0).max() and np.abs(J - J0).max() <= 1e-12
    assert np.abs(a - a_o).max() <= 1e-12 * np.abs(a_o).max() and np.abs(J - J_o).max() <= 1e-12
    # ... and so is the step
    assert C.rel(dc, dc0) <= C.BARS["dc"] and C.rel(dl, dl0) <= C.BARS["dl"]


@pytest.mark.parametrize("name", ("29", "86"))
def test_two_iterates_and_two_handles_give_the_same_bits(name):
    d = C.case(name)

    def run(e):
        e.set_state(d["states0"], d["Xs"])
        t = trial(e, 1e-3)
        return np.concatenate([t, e.attitude_residual().ravel(), e.attitude_jacobian().ravel(), e.attitude_edge_cost()])

    a, b = engine(d), engine(d)
    runs = [run(a), run(a), run(b)]
    a.close(), b.close()
    for other in runs[1:]:
        assert np.array_equal(runs[0], other)


@pytest.mark.parametrize("name", ("29", "86"))
def test_handle_without_the_call_is_the_dynamics_handle(name):
    """Two dynamics handles that never enable the factor give equal bits for a trial and for the state covariance, and neither has
    attitude arrays; sigma_att = 1e-30 carries the plain dynamics handle's step."""
    from vinsat_amd._lib import VbaError
    d = C.case(name)
    a, b, t = engine(d, attitude=False), engine(d, attitude=False), engine(d, sigma_att=1e-30)
    ta, tb = trial(a, 1e-3), trial(b, 1e-3)
    assert np.array_equal(ta, tb)
    a.set_state(d["states0"], d["Xs"]), b.set_state(d["states0"], d["Xs"])
    ca, cb = a.state_covariance(1e-3), b.state_covariance(1e-3)
    for k in ("state", "edges", "landmark"):
        assert np.array_equal(ca[k], cb[k])
    for fetch in (a.attitude_residual, a.attitude_jacobian, a.attitude_edge_cost):
        with pytest.raises(VbaError, match="attitude factor is not enabled"):
            fetch()
    a.set_state(d["states0"], d["Xs"])
    ra, rt = a.iterate(1e-3), t.iterate(1e-3)
    (dca, dla), (dct, dlt) = a.last_step(), t.last_step()
    dva, dvt = a.last_velocity_step(), t.last_velocity_step()
    a.close(), b.close(), t.close()
    fig = (C.rel(dct, dca), C.rel(dvt, dva), C.rel(dlt, dla))
    print(f"CONTINUITY {name}: dc {fig[0]:.1e} dv {fig[1]:.1e} dl {fig[2]:.1e}")
    assert max(fig) <= 1e-7
    assert abs(ra[0] - rt[0]) <= 1e-10 * ra[0] and abs(ra[1] - rt[1]) <= 1e-7 * ra[1]


def test_pose_without_rows_has_a_covariance_at_zero_damping():
    """43 / 450 at lamda = 0.  Without the factor: info != 0 and NaN -- a result, not a fault.  With it: info = 0, finite, symmetric,
    and within the bar of tests/test_gpu_schur_dyn_cov.py of the dense inverse of the oracle's system."""
    d = C.case("43")
    i = C.EMPTY_POSE["43"]
    p = engine(d, attitude=False)
    cp = p.state_covariance(0.0, strict=False)
    p.close()
    assert cp["info"] == 6 * i + 3 + 1 and np.all(np.isnan(cp["state"])) and np.all(np.isnan(cp["edges"]))
    r = C.covariance_reference("43", 0.0)
    e = engine(d)
    c = e.state_covariance(0.0, pairs=True)
    e.close()
    assert c["info"] == 0
    got = dict(state=c["state"], edges=c["edges"], pairs=c["pairs"][2], landmark=c["landmark"])
    assert all(np.isfinite(v).all() for v in got.values())
    assert np.array_equal(c["state"], np.swapaxes(c["state"], 1, 2)) and np.array_equal(c["landmark"], np.swapaxes(c["landmark"], 1, 2))
    assert np.array_equal(c["pairs"][0], r.blk_i) and np.array_equal(c["pairs"][1], r.blk_j)
    fig = V.scaled(got, r)
    print("FIGURES att state cov 43 lam=0 " + " ".join(f"{k}={fig[k]:.2e} (floor {r.floor[k]:.1e}, bar {V.bar(r, k):.1e})" for k in V.FAMILIES))
    for k in V.FAMILIES:
        assert fig[k] <= V.bar(r, k), k
    assert np.all(np.diagonal(c["state"][i])[3:6] > 0)


def test_covariance_query_leaves_the_last_iterate_on_record():
    d = C.case("29")
    e = engine(d)
    e.iterate(1e-3)                                 # accepted: the resident state moves on
    before = [e.attitude_residual(), e.attitude_jacobian(), e.attitude_edge_cost()]
    assert e.state_covariance(1e-3)["info"] == 0    # builds at the NEW state, into arrays of its own
    after = [e.attitude_residual(), e.attitude_jacobian(), e.attitude_edge_cost()]
    e.close()
    a_o, _, _ = A.edge_terms(d["states0"][:, 3:7], d["cumrot"])
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    assert np.abs(before[0] - a_o).max() <= 1e-12 * np.abs(a_o).max()


def test_lm_loop_follows_the_oracle_trial_for_trial():
    d = C.case("29")
    f = C.factors(d)
    e = engine(d)
    hist = e.solve(lamda0=1e-4, max_iters=8)
    st1, _ = e.get_state()
    e.close()
    accepted = [h for h in hist if h[2]]
    assert len(accepted) >= 2
    assert all(h[1] < h[0] for h in accepted)
    assert all(accepted[k + 1][0] == accepted[k][1] for k in range(len(accepted) - 1))

    def att_err(s):                                 # angle between the estimate and the truth, per pose (sign of q immaterial)
        w = np.abs((s[:, 3:7] * d["states_gt"][:, 3:7]).sum(1))
        return float((2 * np.arccos(np.minimum(w, 1.0))).max())

    print(f"LM 29: cost {hist[0][0]:.6g} -> {accepted[-1][1]:.6g}, attitude error {att_err(d['states0']):.2e} -> {att_err(st1):.2e} rad")
    assert att_err(st1) < att_err(d["states0"])
    st, X = d["states0"], d["Xs"]
    for k, (c0, c1, ok, lam) in enumerate(hist):
        dc9, dl, _, _ = A.step_schur(*A.normal_equations(st, X, *C.args(d), lam, *f))
        s1, X1 = A.apply_step(st, X, dc9, dl)
        r0, r1 = A.cost(st, X, *C.args(d), *f), A.cost(s1, X1, *C.args(d), *f)
        assert abs(c0 - r0) <= 1e-7 * r0 and abs(c1 - r1) <= 1e-7 * r1, (k, c0, r0, c1, r1)
        if ok:
            st, X = s1, X1
    assert C.rel(st1, st) <= 1e-7


def test_refusals_leave_the_handle_usable():
    from vinsat_amd._lib import VbaError, load
    from vinsat_amd.schur import SchurBA
    d = C.case("12")
    e = engine(d)
    first = e.iterate(1e-3)
    for call in (lambda: e.state_reliability(), lambda: e.state_snoop(), lambda: e.state_outlier_power(),
                 lambda: e.solve(max_iters=1, state_snoop=dict(rounds=1))):
        with pytest.raises(VbaError, match="not available on a handle with the attitude factor"):
            call()
    lib = load()
    c = np.ascontiguousarray(d["cumrot"])
    pc = c.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert lib.vba_schur_enable_attitude(e.h, pc, 1.0) == 4 and b"already enabled" in lib.vba_schur_last_error()     # VBA_ESTATE
    assert lib.vba_schur_enable_attitude(e.h, None, 1.0) == 1 and lib.vba_schur_enable_attitude(None, pc, 1.0) == 1     # VBA_EINVAL
    e.set_state(d["states0"], d["Xs"])
    assert e.iterate(1e-3) == first
    assert e.reweight(1.5)["status"] == 0 and e.weights().shape == d["w"].shape     # rows only: unchanged
    e.close()
    # without the dynamics factor
    p = SchurBA(d["states0"], d["X0"], d["uv"], d["w"], d["pose_of_row"], d["landmark_of_row"], d["intrinsics"], sigma_prior=d["sigma"])
    assert lib.vba_schur_enable_attitude(p.h, pc, 1.0) == 4 and b"needs the dynamics factor" in lib.vba_schur_last_error()
    p.close()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(VbaError, match="sigma_att must be positive and finite"):
            engine(d, sigma_att=bad)
    for row, value in ((3, np.nan), (0, np.inf)):
        c = d["cumrot"].copy()
        c[row, 1] = value
        with pytest.raises(VbaError, match=f"cumrot row {row} is not a unit quaternion"):
            engine(d, cumrot=c)
    c = d["cumrot"].copy()
    c[5] *= 1 + 3e-6
    with pytest.raises(VbaError, match="cumrot row 5 is not a unit quaternion"):
        engine(d, cumrot=c)
    c = d["cumrot"].copy()
    c[-1] = np.nan                                   # the last row is ignored
    c[5] *= 1 + 3e-7                                 # within 1e-6: taken as given
    g = engine(d, cumrot=c)
    assert g.iterate(1e-3)[2]
    g.close()
    with pytest.raises(ValueError, match="one quaternion per pose"):
        engine(d, cumrot=d["cumrot"][:-1])
    e = engine(d)
    assert e.iterate(1e-3) == first
    e.close()
