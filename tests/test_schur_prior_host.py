"""The CPU side of the state prior factor of the free-landmark mode and of the window hand-off (no GPU): the oracle of
tests/schur_prior_oracle.py against itself -- its Jacobian, the conjugation identity behind the hand-off's R, its two routes, the
mistakes it must be able to tell -- and the host build of vinsat_amd/csrc/vba_schur_prior_math.h under the sanitizers as a stand-alone
program.  DESIGN 9.13 has the tables of what is measured here.

Two-route floors.  ``lamda = 0`` on 43 / 450 without the attitude factor has no step unless the prior set holds pose 20 (``gap``,
``all``): the reduced system is not positive definite (the very thing ``test_pose_without_rows_needs_the_prior`` asserts), so those
combinations have no floor and are left out; every other combination is asserted.
"""
import os
import subprocess

import numpy as np
import pytest

import exact_orbit as X
import schur_prior_cases as C
import schur_prior_oracle as P
from oracle import ba_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cases_are_what_their_names_say():
    for name in C.NAMES:
        n = C.case(name)["states0"].shape[0]
        assert list(C.prior(name, "ends")[0]) == [0, n - 1] and C.prior(name, "all")[0].size == n
        idx, an, infos = C.prior(name, "flip")
        e, J = P.prior_terms(C.case(name)["states0"][idx], an)
        w = O.qmul(P.A.conj(an[:, 3:7]), C.case(name)["states0"][idx][:, 3:7])
        assert w[0, 3] < 0 < w[1, 3]
        # the flipped anchor is the same rotation: e and J are those of ``ends``
        e0, J0 = P.prior_terms(C.case(name)["states0"][idx], C.prior(name, "ends")[1])
        assert np.abs(e - e0).max() <= 1e-15 and np.abs(J - J0).max() <= 1e-15
        L = C.prior(name, "posonly")[2]
        assert np.count_nonzero(L[:, 3:, :]) == 0 and np.count_nonzero(L[:, :, 3:]) == 0 and np.linalg.matrix_rank(L[0]) == 3
        for s in C.SETS:
            Ls = C.prior(name, s)[2]
            assert np.array_equal(Ls, np.swapaxes(Ls, 1, 2))
    assert list(C.prior(C.GAP_CASE, "gap")[0]) == [C.GAP_POSE]
    full = C.prior("29", "all")[2]
    assert np.all(np.abs(full[:, 6:9, 0:6]) > 0)             # full blocks: the velocity-pose block is there to be transposed


@pytest.mark.parametrize("pset", ("all", "flip"))
@pytest.mark.parametrize("name", C.NAMES)
def test_jacobian_by_central_differences(name, pset):
    d = C.case(name)
    idx, an, _ = C.prior(name, pset)
    st = d["states0"][idx]
    _, J = P.prior_terms(st, an)
    h = 1e-6
    worst = 0.0
    for c in range(3):
        dp = np.zeros((st.shape[0], 9))
        dp[:, 3 + c] = h
        ep, _ = P.prior_terms(O.retract(st, dp), an)
        em, _ = P.prior_terms(O.retract(st, -dp), an)
        worst = max(worst, float(np.abs((ep - em)[:, 3:6] / (2 * h) - J[:, :, c]).max()))
        # position and velocity rows do not move with the attitude, and move one to one with their own unknowns
        assert np.abs((ep - em)[:, [0, 1, 2, 6, 7, 8]]).max() == 0.0
    print(f"JACOBIAN {name} {pset}: {worst:.2e}")
    assert worst <= 1e-9
    # J = I at q = +-qbar
    same = st.copy()
    same[:, 3:7] = an[:, 3:7] * np.where(np.arange(st.shape[0]) % 2 == 0, 1.0, -1.0)[:, None]
    e, J = P.prior_terms(same, an)
    assert np.abs(J - np.eye(3)).max() <= 1e-15 and np.abs(e[:, 3:6]).max() <= 1e-15


def test_conjugation_identity_of_the_gap_rotation():
    """(q (x) qexp(d)) (x) c = (q (x) c) (x) qexp(R d): both sides through ``ba_oracle.retract``, by finite differences of size 1e-6
    and at a finite rotation."""
    rng = np.random.default_rng(5)
    q = rng.normal(0, 1, (6, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    c = C.HANDOFF_CUMROT
    R = P.gap_rotation_matrix(c)
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-15
    st = np.zeros((6, 10))
    st[:, 3:7] = q
    stc = st.copy()
    stc[:, 3:7] = O.qmul(q, np.broadcast_to(c, q.shape))
    for scale in (1e-6, 0.3):
        dth = rng.normal(0, scale, (6, 3))
        d9, d9r = np.zeros((6, 9)), np.zeros((6, 9))
        d9[:, 3:6], d9r[:, 3:6] = dth, dth @ R.T
        lhs = O.qmul(O.retract(st, d9)[:, 3:7], np.broadcast_to(c, q.shape))
        rhs = O.retract(stc, d9r)[:, 3:7]
        assert np.abs(lhs - rhs).max() <= 1e-15, scale
        wrong = np.zeros((6, 9))
        wrong[:, 3:6] = dth @ R                        # R transposed
        assert np.abs(lhs - O.retract(stc, wrong)[:, 3:7]).max() >= 1e-2 * scale


_FLOOR_COMBOS = [(n, s, a, lam) for (n, s, a) in C.COMBOS for lam in (1e-3, 1e-6, 0.0)
                 if not (n == C.GAP_CASE and not a and lam == 0.0 and s not in ("gap", "all"))]


@pytest.mark.parametrize("name,pset,att,lam", _FLOOR_COMBOS)
def test_two_routes_agree_below_a_tenth_of_the_bars(name, pset, att, lam):
    r = C.reference(name, pset, lam, att, full=True)
    print(f"FLOOR {name} {pset} att={att} lam={lam:g}: " + " ".join(f"{k}={v:.1e}" for k, v in r.floor.items()))
    bad = {k: v for k, v in r.floor.items() if not v <= 0.1 * C.BARS[k]}
    assert not bad, bad


def test_pose_without_rows_needs_the_prior():
    """43 / 450 at lamda = 0 without the attitude factor: not positive definite without the prior, positive definite with ``gap``."""
    assert not C.positive_definite(C.GAP_CASE, None, 0.0, False)
    assert not C.positive_definite(C.GAP_CASE, "first", 0.0, False)
    assert C.positive_definite(C.GAP_CASE, "gap", 0.0, False)


_FAULT_CASES = {"vp_transposed": ("29", "all"), "no_J": ("29", "all"), "no_s": ("12", "flip"), "lam_T": ("29", "all"), "wrong_pose": ("29", "ends"),
                "no_cost": ("29", "all")}


@pytest.mark.parametrize("fault", sorted(_FAULT_CASES))
def test_planted_faults_are_past_the_bars(fault):
    """Each mistake, on the case named for it, moves some figure of a trial at least 100 bars."""
    name, pset = _FAULT_CASES[fault]
    good, bad = C.reference(name, pset, 1e-3, True), C.reference(name, pset, 1e-3, True, fault=fault)
    fig = dict(c0=abs(bad.c0 - good.c0) / good.c0, c1=abs(bad.c1 - good.c1) / good.c1, dc=C.rel(bad.dc, good.dc), dv=C.rel(bad.dv, good.dv),
               dl=C.rel(bad.dl, good.dl))
    worst = max(v / C.BARS[k] for k, v in fig.items())
    print(f"FAULT {fault} on {name} {pset}: {worst:.1e} bars " + " ".join(f"{k}={v:.1e}" for k, v in fig.items()))
    assert worst >= 100


def _handoff_inputs(name="29"):
    d = C.case(name)
    Sigma = np.linalg.inv(C.prior(name, "all")[2][3])
    return Sigma, d["states_gt"][-1]


@pytest.mark.parametrize("fault", ("handoff_GtSG", "handoff_Rt"))
def test_planted_handoff_faults_are_past_the_bar(fault):
    Sigma, st = _handoff_inputs()
    _, good = P.handoff(Sigma, st, 65, C.HANDOFF_CUMROT, C.HANDOFF_NOISE)
    _, bad = P.handoff(Sigma, st, 65, C.HANDOFF_CUMROT, C.HANDOFF_NOISE, fault=fault)
    off = P.scaled_info_error(bad, good)
    print(f"FAULT {fault}: {off:.1e} sigmas")
    assert off >= 100 * 1e-11 and off >= 1e-3


@pytest.mark.parametrize("noise", (None, C.HANDOFF_NOISE))
@pytest.mark.parametrize("steps", C.HANDOFF_STEPS)
def test_handoff_floor_against_longdouble(steps, noise):
    """The fp64 hand-off of the oracle against its longdouble run, in sigmas of the information matrix: the floor behind the bar of
    the GPU test, max(100 x floor, 1e-11).  Measured: at most 8.8e-15, at 935 steps."""
    Sigma, st = _handoff_inputs()
    fl = C.handoff_floor(Sigma, st, steps, noise)
    a64, i64 = P.handoff(Sigma, st, steps, C.HANDOFF_CUMROT, noise)
    print(f"HANDOFF FLOOR steps={steps} noise={noise is not None}: {fl:.2e}")
    assert fl <= 1e-11
    assert np.array_equal(i64, i64.T) or np.abs(i64 - i64.T).max() <= 1e-12 * np.abs(i64).max()
    assert abs(np.linalg.norm(a64[3:7]) - 1) <= 1e-15
    # more noise, less information
    _, more = P.handoff(Sigma, st, steps, C.HANDOFF_CUMROT, tuple(10 * np.asarray(C.HANDOFF_NOISE)))
    _, less = P.handoff(Sigma, st, steps, C.HANDOFF_CUMROT, None)
    assert np.all(np.diag(np.linalg.inv(more)) > np.diag(np.linalg.inv(less)))


def test_constructor_wants_the_prior_on_a_dynamics_handle():
    from vinsat_amd.schur import SchurBA, prior_for_first_pose
    d = C.case("12")
    with pytest.raises(ValueError, match="state prior is only valid together with time_idx"):
        SchurBA(d["states0"], d["X0"], d["uv"], d["w"], d["pose_of_row"], d["landmark_of_row"], d["intrinsics"], state_prior=C.prior("12", "first"))
    idx, an, L = prior_for_first_pose(dict(anchor=np.arange(10.0), info=np.eye(9)))
    assert idx.dtype == np.int32 and list(idx) == [0] and an.shape == (1, 10) and L.shape == (1, 9, 9)


def _write_case(path, name, pset, steps):
    d = C.case(name)
    st = d["states0"]
    pr = C.prior(name, pset)
    H, g, e, J = P.prior_blocks(st, pr)
    Sigma, last = _handoff_inputs(name)
    x0 = np.concatenate([last[:3], last[7:10]])[None]
    _, Phi = X.propagate(x0, np.array([steps]))
    _, info = P.handoff(Sigma, last, steps, C.HANDOFF_CUMROT, C.HANDOFF_NOISE)
    parts = [[st.shape[0], pr[0].size, 1e-10, steps], st, pr[0], pr[1], pr[2], e, J, [P.prior_cost(st, pr)], np.tril(H), g, C.HANDOFF_CUMROT,
             C.HANDOFF_NOISE, Phi[0].astype(np.float64), Sigma, info]
    np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in parts]).tofile(path)


def test_host_build_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """vba_schur_prior_math.h compiled for the host: the per-prior body and every work item of the scatter on 12 / 150 ``flip`` (a
    prior with d < 0, idx not 0, 1) and on 29 / 300 ``all`` against the oracle's e, J, cost, and the lower triangle and right-hand side
    of the factor; the hand-off's congruence and Cholesky inverse against the oracle's dense inverse."""
    src = os.path.join(ROOT, "tests", "hostcheck", "sanitize_schur_prior_main.cpp")
    exe = str(tmp_path / "sanitize_schur_prior_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    for name, pset, steps in (("12", "flip", 65), ("29", "all", 7)):
        path = str(tmp_path / f"case_{name}.bin")
        _write_case(path, name, pset, steps)
        p = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
        print(p.stdout, p.stderr)
        assert p.returncode == 0, p.stdout + p.stderr
        assert "sanitize_schur_prior_main ok" in p.stdout and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
        if pset == "flip":
            assert "(1 with d < 0)" in p.stdout
