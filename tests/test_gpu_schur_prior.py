"""The state prior factor of the free-landmark mode and the window hand-off on the GPU (``SchurBA(..., state_prior=)``,
``vba_schur_enable_state_prior``, ``SchurBA.handoff``, ``vba_schur_handoff``; vinsat_amd/csrc/vba_schur_prior.hip) against
tests/schur_prior_oracle.py.  PARITY UNPINNED as the rest of the add-on.  Cases and prior sets: tests/schur_prior_cases.py.

Bars.  e, J and the cost shares answer componentwise to ``max(16, 4 x the float64 oracle's own error against its longdouble
restatement)`` units of 2^-53 of the largest entry, the rule of DESIGN 9.5 / 9.9.  One trial answers to ``schur_dyn_cases.BARS``; the
oracle's two-route floor is below a tenth of each of them on every combination (tests/test_schur_prior_host.py).  The state covariance
answers to ``max(100 x floor, 1e-11)`` per family, every entry scaled by the reference sigmas of its row and column.  The
hand-off's anchor answers to the exact chain under the bar of ``test_gpu_long_gaps._check_factor_exact`` (16 x the fp64 serial walk's
own error + 2^-46); its information matrix, scaled by the sigmas of its row and column, to ``max(100 x the oracle's fp64-against-
longdouble floor, 1e-11)``.  Floors and the device's figures on the MI355X: DESIGN 9.13.
"""
import ctypes

import numpy as np
import pytest

import exact_orbit as X
import schur_dyn_cov_cases as V
import schur_prior_cases as C
import schur_prior_oracle as P
import schur_query_harness as H
from oracle import ba_oracle as O

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
EXACT_SLACK, EXACT_FACTOR = 2.0 ** -46, 16.0
PAIRS = tuple(dict.fromkeys((n, s) for n, s, _ in C.COMBOS))


def engine(d, prior=None, att=True, long_gaps=False, states=None):
    from vinsat_amd.schur import SchurBA
    kw = dict(time_idx=d["time_idx"], sigma_dyn=d["sigma_dyn"], long_gaps=long_gaps, state_prior=prior)
    if att:
        kw.update(cumrot=d["cumrot"], sigma_att=d["sigma_att"])
    st = d["states0"] if states is None else states
    e = SchurBA(st, d["X0"], d["uv"], d["w"], d["pose_of_row"], d["landmark_of_row"], d["intrinsics"], sigma_prior=d["sigma"], **kw)
    e.set_state(st, d["Xs"])
    return e


def case_engine(name, pset, att):
    return engine(C.case(name), None if pset is None else C.prior(name, pset), att, C.long_gaps(name))


def trial(e, lam):
    """Everything one iterate leaves, flat."""
    c = e.iterate(lam)
    parts = [c, *e.last_step(), e.last_velocity_step(), e.cholesky_factor(), *e.get_state()]
    return np.concatenate([np.ravel(np.asarray(p, dtype=np.float64)) for p in parts])


@pytest.mark.parametrize("name,pset", PAIRS)
def test_terms_against_the_oracle_componentwise(name, pset):
    e_o, J_o, sh_o, units = C.terms_reference(name, pset)
    bars = C.terms_bars(name, pset)
    e = case_engine(name, pset, pset != "gap")
    e.iterate(1e-3)
    got = dict(e=e.prior_residual(), J=e.prior_jacobian(), share=e.prior_cost())
    e.close()
    ref = dict(e=e_o, J=J_o, share=sh_o)
    fig = {k: float(np.abs(got[k] - ref[k]).max() / np.abs(ref[k]).max() / U) for k in ref}
    print(f"TERMS {name} {pset}: " + " ".join(f"{k}={fig[k]:.1f}/{bars[k]:.0f} (oracle {units[k]:.1f})" for k in fig))
    assert all(got[k].shape == ref[k].shape and np.isfinite(got[k]).all() for k in ref)
    bad = {k: v for k, v in fig.items() if not v <= bars[k]}
    assert not bad, bad


@pytest.mark.parametrize("name,pset", PAIRS)
def test_one_trial_matches_the_oracle(name, pset):
    """Both dampings, with and without the attitude factor (``gap``: without only), on one handle each."""
    d, B = C.case(name), C.BARS
    n = d["states0"].shape[0]
    for att in ((False,) if pset == "gap" else (False, True)):
        e = case_engine(name, pset, att)
        for lam in C.LAMS:
            ref = C.reference(name, pset, lam, att)
            e.set_state(d["states0"], d["Xs"])
            c0, c1, ok = e.iterate(lam)
            assert e.last_info() == 0
            dc, dl = e.last_step()
            dv, Lg = e.last_velocity_step(), e.cholesky_factor()
            st, Xl = e.get_state()
            fig = dict(c0=abs(c0 - ref.c0) / ref.c0, c1=abs(c1 - ref.c1) / ref.c1, dc=C.rel(dc, ref.dc), dv=C.rel(dv, ref.dv), dl=C.rel(dl, ref.dl),
                       LLt=C.rel(Lg @ Lg.T, ref.Sm), L=C.rel(Lg, ref.Lc), states=max(C.rel(st, ref.st), C.rel(Xl, ref.X)))
            print(f"TRIAL {name} {pset} att={att} lam={lam:g}: " + " ".join(f"{k}={v:.1e}" for k, v in fig.items()))
            assert Lg.shape == (9 * n, 9 * n) and ok == ref.ok
            bad = {k: v for k, v in fig.items() if not v <= B[k]}
            assert not bad, (att, lam, bad)
        e.close()


def test_pose_without_rows_has_a_covariance_with_the_prior():
    """43 / 450 ``gap`` at lamda = 0, no attitude factor.  Without the prior: info = 124 and NaN.  With it: info = 0, finite, exactly
    symmetric, within the bar of DESIGN 9.6 of the dense inverse of the oracle's system."""
    i = C.GAP_POSE
    p = case_engine(C.GAP_CASE, None, False)
    cp = p.state_covariance(0.0, strict=False)
    p.close()
    assert cp["info"] == 6 * i + 3 + 1 == 124 and np.all(np.isnan(cp["state"]))
    r = C.covariance_reference(C.GAP_CASE, "gap", 0.0, False)
    e = case_engine(C.GAP_CASE, "gap", False)
    c = e.state_covariance(0.0, pairs=True)
    e.close()
    assert c["info"] == 0
    got = dict(state=c["state"], edges=c["edges"], pairs=c["pairs"][2], landmark=c["landmark"])
    assert all(np.isfinite(v).all() for v in got.values())
    assert np.array_equal(c["state"], np.swapaxes(c["state"], 1, 2))
    fig = V.scaled(got, r)
    print("FIGURES prior state cov 43 gap lam=0 " + " ".join(f"{k}={fig[k]:.2e} (floor {r.floor[k]:.1e}, bar {V.bar(r, k):.1e})" for k in V.FAMILIES))
    for k in V.FAMILIES:
        assert fig[k] <= V.bar(r, k), k


@pytest.mark.parametrize("name,pset", (("43", "gap"), ("29", "all"), ("12", "posonly")))
def test_the_prior_raises_no_variance(name, pset):
    """Adding a positive semidefinite term cannot raise a variance: on a handle with the attitude factor (so that both systems are
    positive definite at lamda = 0), no diagonal entry of state_cov with the prior exceeds its value without it by more than the bar."""
    r = C.covariance_reference(name, pset, 0.0, True)
    a, b = case_engine(name, pset, True), case_engine(name, None, True)
    with_, without = a.state_covariance(0.0)["state"], b.state_covariance(0.0)["state"]
    a.close(), b.close()
    dw, d0 = np.diagonal(with_, axis1=1, axis2=2), np.diagonal(without, axis1=1, axis2=2)
    excess = float(((dw - d0) / d0).max())
    print(f"VARIANCES {name} {pset}: largest relative excess {excess:.2e} (bar {V.bar(r, 'state'):.1e}); largest drop {float((1 - dw / d0).max()):.3f}")
    assert excess <= V.bar(r, "state")
    assert (1 - dw / d0).max() > 1e-3                # ... and it lowers some


@pytest.fixture(scope="module")
def solved_29():
    """29 / 300 with the attitude factor after solve(max_iters=6): the handle, its resident last state and its marginal."""
    d = C.case("29")
    e = engine(d)
    e.solve(max_iters=6)
    st, _ = e.get_state()
    cov = e.state_covariance(0.0)["state"][-1]
    yield e, st[-1], cov
    e.close()


@pytest.mark.parametrize("noise", (None, C.HANDOFF_NOISE))
@pytest.mark.parametrize("steps", C.HANDOFF_STEPS)
def test_handoff_against_the_exact_chain_and_the_dense_inverse(solved_29, steps, noise):
    e, last, Sigma = solved_29
    out = e.handoff(steps, C.HANDOFF_CUMROT, noise)
    assert out["status"] == 0 and np.isfinite(out["anchor"]).all() and np.isfinite(out["info"]).all()
    assert np.array_equal(out["info"], out["info"].T)
    # anchor: (p, v) against the exact chain, relative to the fp64 serial walk's own error
    x0 = np.concatenate([last[:3], last[7:10]])[None]
    xe = X.propagate(x0, np.array([steps]), stm=False)
    xo, _ = O.propagate_orbit(x0, np.array([steps]))
    got = np.concatenate([out["anchor"][:3], out["anchor"][7:10]])[None].astype(np.longdouble)
    for sl, what in ((slice(0, 3), "pos"), (slice(3, 6), "vel")):
        eg = float(np.abs(got[:, sl] - xe[:, sl]).max() / np.abs(xe[:, sl]).max())
        eo = float(np.abs(xo[:, sl] - xe[:, sl]).max() / np.abs(xe[:, sl]).max())
        print(f"HANDOFF anchor {what} steps={steps}: device {eg:.2e} oracle {eo:.2e}")
        assert eg <= EXACT_FACTOR * eo + EXACT_SLACK, (what, eg, eo)
    q = O.qmul(last[None, 3:7], C.HANDOFF_CUMROT[None])[0]
    assert np.abs(out["anchor"][3:7] - q / np.linalg.norm(q)).max() <= 4 * U
    # info: against the oracle's hand-off of the device's own marginal
    _, ref = P.handoff(Sigma, last, steps, C.HANDOFF_CUMROT, noise, dtype=np.longdouble)
    floor = C.handoff_floor(Sigma, last, steps, noise)
    bar = max(100 * floor, 1e-11)
    fig = P.scaled_info_error(out["info"], ref)
    print(f"HANDOFF info steps={steps} noise={noise is not None}: {fig:.2e} (floor {floor:.1e}, bar {bar:.1e}) {e.last_handoff_ms():.3f} ms")
    assert fig <= bar
    assert e.last_handoff_ms() > 0


def test_handoff_changes_nothing_and_repeats_its_bits(solved_29):
    e, _, _ = solved_29
    before = [e.attitude_residual(), e.dynamics_residual(), *e.get_state(), e.state_covariance(0.0)["state"]]
    a = e.handoff(935, C.HANDOFF_CUMROT, C.HANDOFF_NOISE)
    b = e.handoff(935, C.HANDOFF_CUMROT, C.HANDOFF_NOISE)
    after = [e.attitude_residual(), e.dynamics_residual(), *e.get_state(), e.state_covariance(0.0)["state"]]
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    assert np.array_equal(a["anchor"], b["anchor"]) and np.array_equal(a["info"], b["info"])


def test_two_windows_end_to_end():
    """Window A = poses 0 .. 14 of 29 / 300, B the rest: solve A, hand its last pose across the gap to B's pose 0, run B with that
    prior.  B's LM loop follows the oracle's at the device's damping sequence and accept decisions within 1e-7 of every cost, and the
    position and velocity sigmas of B's pose 0 are below those of B without the prior."""
    from vinsat_amd.schur import prior_for_first_pose, state_sigmas
    A_, B_ = C.split_windows("29", 15)
    a = engine(A_)
    a.solve(max_iters=6)
    ho = a.handoff(B_["gap"], B_["cumrot_gap"], C.HANDOFF_NOISE)
    a.close()
    assert ho["status"] == 0
    pr = prior_for_first_pose(ho)
    b, plain = engine(B_, pr), engine(B_)
    hist = b.solve(lamda0=1e-4, max_iters=6)
    plain.solve(lamda0=1e-4, max_iters=6)
    st1, _ = b.get_state()
    sb, sp = state_sigmas(b.state_covariance(0.0)), state_sigmas(plain.state_covariance(0.0))
    b.close(), plain.close()
    print(f"END TO END: pose 0 of B position sigma {sp[0][0].max():.3e} -> {sb[0][0].max():.3e} km, velocity {sp[2][0].max():.3e} -> {sb[2][0].max():.3e} km/s")
    assert np.all(sb[0][0] < sp[0][0]) and np.all(sb[2][0] < sp[2][0])
    f = C.factors(B_, pr, True)
    st, Xl = B_["states0"], B_["Xs"]
    assert sum(h[2] for h in hist) >= 2
    for k, (c0, c1, ok, lam) in enumerate(hist):
        dc9, dl, _, _ = P.step_schur(*P.normal_equations(st, Xl, *C.args(B_), lam, *f))
        s1, X1 = P.apply_step(st, Xl, dc9, dl)
        r0, r1 = P.cost(st, Xl, *C.args(B_), *f), P.cost(s1, X1, *C.args(B_), *f)
        assert abs(c0 - r0) <= 1e-7 * r0 and abs(c1 - r1) <= 1e-7 * r1, (k, c0, r0, c1, r1)
        if ok:
            st, Xl = s1, X1
    assert C.rel(st1, st) <= 1e-7


@pytest.mark.parametrize("name", ("29", "L12"))
def test_handle_without_the_call_keeps_its_bits(name):
    """Two handles that never enable the prior give equal bits for a trial and for the state covariance, and have no prior arrays."""
    from vinsat_amd._lib import VbaError
    d = C.case(name)
    a, b = case_engine(name, None, True), case_engine(name, None, True)
    assert np.array_equal(trial(a, 1e-3), trial(b, 1e-3))
    a.set_state(d["states0"], d["Xs"]), b.set_state(d["states0"], d["Xs"])
    assert H._same_cov(a.state_covariance(1e-3), b.state_covariance(1e-3))
    for fetch in (a.prior_residual, a.prior_jacobian, a.prior_cost):
        with pytest.raises(VbaError, match="state prior is not enabled"):
            fetch()
    a.close(), b.close()


@pytest.mark.parametrize("name,pset", (("29", "all"), ("L12", "ends")))
def test_two_runs_and_two_handles_give_the_same_bits(name, pset):
    d = C.case(name)

    def run(e):
        e.set_state(d["states0"], d["Xs"])
        t = trial(e, 1e-3)
        cov = e.state_covariance(1e-3)["state"].ravel()
        return np.concatenate([t, e.prior_residual().ravel(), e.prior_jacobian().ravel(), e.prior_cost(), cov])

    a, b = case_engine(name, pset, True), case_engine(name, pset, True)
    runs = [run(a), run(a), run(b)]
    a.close(), b.close()
    for other in runs[1:]:
        assert np.array_equal(runs[0], other)


def test_covariance_query_leaves_the_last_iterate_on_record():
    d = C.case("29")
    e = case_engine("29", "all", True)
    e.iterate(1e-3)                                 # accepted: the resident state moves on
    before = [e.prior_residual(), e.prior_jacobian(), e.prior_cost()]
    assert e.state_covariance(1e-3)["info"] == 0    # builds at the NEW state, into arrays of its own
    after = [e.prior_residual(), e.prior_jacobian(), e.prior_cost()]
    e.close()
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    assert np.abs(before[0] - C.terms_reference("29", "all")[0]).max() <= 1e-12 * np.abs(before[0]).max()


def test_refused_queries_leave_the_iterates_their_bits():
    """The six _dyn / _att reliability, snoop and outlier power entries return VBA_ESTATE naming the state prior; an iterate afterwards
    has the bits it would have had."""
    from vinsat_amd._lib import VbaError
    d = C.case("12")
    clean = case_engine("12", "first", True)
    want = trial(clean, 1e-3)
    clean.close()
    e, p = case_engine("12", "first", True), case_engine("12", "first", False)
    for h, suffix in ((e, "_att"), (p, "_dyn")):
        for base in ("vba_schur_reliability", "vba_schur_snoop", "vba_schur_outlier_power"):
            rc = H.raw_query(h, base + suffix, 0.0)[0]
            assert rc == 4 and H.last_error(h).startswith(base + suffix + " is not available on a handle with the state prior"), H.last_error(h)
    for call in (e.attitude_reliability, e.attitude_snoop, e.attitude_outlier_power, p.state_reliability, p.state_snoop, p.state_outlier_power):
        with pytest.raises(VbaError, match="not available on a handle with the state prior"):
            call()
    # the checks in front of it keep their order: an _att handle asked through a _dyn entry hears of the attitude factor
    assert H.raw_query(e, "vba_schur_reliability_dyn", 0.0)[0] == 4 and "attitude factor" in H.last_error(e)
    assert np.array_equal(trial(e, 1e-3), want)
    assert e.reweight(1.5)["status"] == 0 and e.weights().shape == d["w"].shape
    e.close(), p.close()


def test_refusals_leave_the_handle_usable():
    from vinsat_amd._lib import PD, VbaError, load
    from vinsat_amd.schur import SchurBA
    lib = load()
    d = C.case("12")
    n = d["states0"].shape[0]
    idx, an, L = (np.array(a) for a in C.prior("12", "ends"))
    PI = ctypes.POINTER(ctypes.c_int)

    def enable(h, count, i, a, l):
        ptr = lambda x, t: None if x is None else np.ascontiguousarray(x).ctypes.data_as(t)
        rc = lib.vba_schur_enable_state_prior(h, count, ptr(i, PI), ptr(a, PD), ptr(l, PD))
        return rc, (lib.vba_schur_last_error() or b"").decode()

    e = engine(d)
    first = trial(e, 1e-3)

    def mod(arr, where, value):
        out = arr.copy()
        out[where] = value
        return out

    asym = L.copy()
    asym[1, 7, 8] *= 1 + 1e-7               # (a velocity entry: the block's largest are there)
    refused = [
        ((2, None, an, L), "null"), ((2, idx, None, L), "null"), ((2, idx, an, None), "null"),
        ((0, idx, an, L), "count must be in 1 .. n"), ((n + 1, idx, an, L), "count must be in 1 .. n"),
        ((2, mod(idx, 1, n), an, L), "pose_idx entry 1 is outside"), ((2, mod(idx, 0, -1), an, L), "pose_idx entry 0 is outside"),
        ((2, mod(idx, 1, 0), an, L), "pose_idx entry 1 repeats pose 0"),
        ((2, idx, mod(an, (1, 8), np.nan), L), "anchor 1 is not finite"), ((2, idx, mod(an, (0, 2), np.inf), L), "anchor 0 is not finite"),
        ((2, idx, mod(an, (1, slice(3, 7)), an[1, 3:7] * (1 + 3e-6)), L), "quaternion of anchor 1 is not a unit quaternion"),
        ((2, idx, an, mod(L, (1, 4, 4), np.nan)), "info block 1 is not finite"), ((2, idx, an, asym), "info block 1 is not symmetric"),
        ((2, idx, an, mod(L, (0, 7, 7), -1.0)), "info block 0 has a negative diagonal"),
    ]
    for args, text in refused:
        rc, msg = enable(e.h, *args)
        assert rc == 1 and text in msg, (text, rc, msg)                     # VBA_EINVAL
    e.set_state(d["states0"], d["Xs"])
    assert np.array_equal(trial(e, 1e-3), first)
    # a norm within 1e-6 and an asymmetry within 1e-12 are taken as given; then the prior is there, and a second one is refused
    ok_an = mod(an, (1, slice(3, 7)), an[1, 3:7] * (1 + 3e-7))
    ok_L = L.copy()
    ok_L[1, 7, 8] *= 1 + 1e-14
    assert enable(e.h, 2, idx, ok_an, ok_L)[0] == 0
    rc, msg = enable(e.h, 2, idx, an, L)
    assert rc == 4 and "already enabled" in msg                             # VBA_ESTATE
    e.set_state(d["states0"], d["Xs"])
    assert e.iterate(1e-3)[2]
    e.close()
    # without the dynamics factor, and through the constructor
    p = SchurBA(d["states0"], d["X0"], d["uv"], d["w"], d["pose_of_row"], d["landmark_of_row"], d["intrinsics"], sigma_prior=d["sigma"])
    rc, msg = enable(p.h, 2, idx, an, L)
    assert rc == 4 and "needs the dynamics factor" in msg
    p.close()
    with pytest.raises(VbaError, match="pose_idx entry 1 repeats pose 0"):
        engine(d, (mod(idx, 1, 0), an, L))
    with pytest.raises(ValueError, match="one anchor"):
        engine(d, (idx, an[:1], L))
    # an indefinite Lambda is accepted and shows as a non-positive pivot
    neg = L.copy()
    neg[0] = -1e6 * neg[0]
    neg[0][np.diag_indices(9)] = np.abs(np.diag(neg[0]))
    g = engine(d, (idx, an, neg))
    c0, c1, ok = g.iterate(1e-6)
    assert not ok and c1 == c0 and g.last_info() != 0
    g.close()


def test_handoff_refusals_leave_the_handle_usable(solved_29):
    from vinsat_amd._lib import PD, load
    from vinsat_amd.schur import SchurBA
    lib = load()
    e, _, _ = solved_29
    want = e.handoff(7, C.HANDOFF_CUMROT)
    c, q = C.HANDOFF_CUMROT.copy(), np.array(C.HANDOFF_NOISE)
    an, inf, word = np.empty(10), np.empty(81), ctypes.c_int(-7)
    ptr = lambda x: None if x is None else x.ctypes.data_as(PD)

    def call(h, lam, steps, c_, q_, a_=an, i_=inf, w_=word):
        rc = lib.vba_schur_handoff(h, lam, steps, ptr(c_), ptr(q_), ptr(a_), ptr(i_), None if w_ is None else ctypes.byref(w_))
        return rc, (lib.vba_schur_last_error() or b"").decode()

    bad_c = c * (1 + 3e-6)
    for args, text in (((e.h, 0.0, 0, c, q), "steps must be in 1 .. VBA_MAX_GAP"), ((e.h, 0.0, (1 << 20) + 1, c, q), "steps must be in 1"),
                       ((e.h, 0.0, 5, bad_c, q), "cumrot_gap is not a unit quaternion"), ((e.h, 0.0, 5, c * np.nan, q), "cumrot_gap is not a unit"),
                       ((e.h, 0.0, 5, c, q * -1), "process_noise must be non-negative"), ((e.h, 0.0, 5, c, q * np.inf), "process_noise must be"),
                       ((e.h, -1.0, 5, c, q), "lamda must be >= 0"), ((e.h, float("nan"), 5, c, q), "lamda must be >= 0"),
                       ((e.h, 0.0, 5, None, q), "null"), ((None, 0.0, 5, c, q), "null")):
        rc, msg = call(*args)
        assert rc == 1 and text in msg, (text, rc, msg)
    assert call(e.h, 0.0, 5, c, q, a_=None)[0] == 1 and call(e.h, 0.0, 5, c, q, i_=None)[0] == 1 and call(e.h, 0.0, 5, c, q, w_=None)[0] == 1
    again = e.handoff(7, C.HANDOFF_CUMROT)
    assert np.array_equal(want["info"], again["info"]) and np.array_equal(want["anchor"], again["anchor"])
    # without the dynamics factor
    d = C.case("12")
    p = SchurBA(d["states0"], d["X0"], d["uv"], d["w"], d["pose_of_row"], d["landmark_of_row"], d["intrinsics"], sigma_prior=d["sigma"])
    rc, msg = call(p.h, 0.0, 5, c, q)
    assert rc == 4 and "dynamics factor is not enabled" in msg
    p.close()
    # a system that is not positive definite: the query's info, NaN, VBA_OK
    g = case_engine(C.GAP_CASE, None, False)
    out = g.handoff(5, c, strict=False)
    assert out["status"] == 124 and np.all(np.isnan(out["anchor"])) and np.all(np.isnan(out["info"]))
    g.close()
