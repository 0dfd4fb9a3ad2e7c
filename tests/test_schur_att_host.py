"""The CPU side of the Gauss-Newton attitude factor of the free-landmark mode (no GPU): the oracle of tests/schur_att_oracle.py
against itself -- its Jacobians, its relation to the reference's term, its two routes, the mistakes it must be able to tell -- and
the host build of vinsat_amd/csrc/vba_schur_att_math.h under the sanitizers as a stand-alone program.

Measured here (DESIGN 9.9 has the tables):

  Jacobians against central differences through ``ba_oracle.retract`` at step 1e-6: at most 1.9e-10 (86 / 900); asserted below 1e-9
  (the truncation of the difference is h^2 / 6 |a'''| ~ 1e-13, its rounding 2^-53 |a| / h ~ 2e-13 per entry; 1e-9 leaves both far
  below and is four orders under the smallest Jacobian entry that matters, 0.5).

  Floors (largest disagreement of the refined full solve and the Schur route, relative to the largest entry) over the five cases,
  lamda in (1e-3, 1e-6, 0) and sigma_att in (5e5, 5e7): at most 4.3e-10, on dv of 12 / 150 at lamda = 1e-6, sigma_att = 5e7,
  against a tenth of the bar = 1e-8.

  The float64 oracle's own error against its longdouble restatement, units of 2^-53 of the largest entry (the bars of
  tests/test_gpu_schur_att.py are max(16, 4 x these)):

    case        a       J      ecost
    12 / 150    189     1.9    128
    29 / 300    193     1.7    110
    43 / 450    195     2.1    118
    86 / 900    223     2.2    174

  (a is a difference of products of entries ~1 that leaves ~2e-3: the units are relative to that.)
"""
import os
import subprocess

import numpy as np
import pytest

import schur_att_cases as C
import schur_att_oracle as A
import schur_dyn_oracle as D
from oracle import ba_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMAS = (C.SIGMA_ATT, 100 * C.SIGMA_ATT)


def test_cases_are_what_their_names_say():
    assert C.SIGMA_ATT == 5e5
    for name in C.NAMES:
        d = C.case(name)
        # at the truth the attitude residual is rounding
        a, _, dd = A.edge_terms(d["states_gt"][:, 3:7], d["cumrot"])
        assert np.abs(a).max() < 1e-15 and np.all(dd > 0)
        assert np.abs(np.linalg.norm(d["cumrot"], axis=1) - 1).max() < 1e-15
        _, _, d0 = A.edge_terms(d["states0"][:, 3:7], d["cumrot"])
        assert list(np.nonzero(d0 < 0)[0]) == ([0, 1] if name == C.SIGN_VARIANT else [])
    assert not np.any(C.case("43")["pose_of_row"] == C.EMPTY_POSE["43"])


@pytest.mark.parametrize("name", C.NAMES)
def test_jacobians_by_central_differences(name):
    d = C.case(name)
    st, c = d["states0"], d["cumrot"]
    n = st.shape[0]
    _, J, _ = A.edge_terms(st[:, 3:7], c)
    h, err = 1e-6, 0.0
    for i in range(n):
        for k in range(3):
            r = []
            for sgn in (1.0, -1.0):
                d9 = np.zeros((n, 9))
                d9[i, 3 + k] = sgn * h
                r.append(A.edge_terms(O.retract(st, d9)[:, 3:7], c)[0])
            num = (r[0] - r[1]) / (2 * h)
            if i < n - 1:
                err = max(err, np.abs(num[i] - J[i, 0][:, k]).max())
            if i > 0:
                err = max(err, np.abs(num[i - 1] - J[i - 1, 1][:, k]).max())
            other = np.delete(num, [e for e in (i - 1, i) if 0 <= e < n - 1], 0)
            assert not other.size or np.abs(other).max() == 0.0         # an attitude moves its two edges only
    print(f"JACOBIAN {name}: {err:.1e}")
    assert err < 1e-9, err


@pytest.mark.parametrize("name", C.NAMES)
def test_relation_to_the_reference_term(name):
    """sigma QUAT_COEFF (1 - |d|) (1 + |d|) / 2 = sigma_att |a|^2 with sigma_att = sigma QUAT_COEFF / 2, the reference's term from
    ``ba_oracle.attitude_factor``.  Both sides are ~40 and lose 1 - d^2 ~ 4e-6 of 1: 2^-53 / 4e-6 ~ 3e-11 relative."""
    d = C.case(name)
    st, c = d["states0"], d["cumrot"]
    f = O.attitude_factor(st, c, jacobian=False)
    _, _, dd = A.edge_terms(st[:, 3:7], c)
    mine = A.edge_cost(st, c, d["sigma_att"])
    err = np.abs(C.SIGMA_DYN * f * (1 + np.abs(dd)) / 2 - mine).max() / mine.max()
    print(f"IDENTITY {name}: {err:.1e}")
    assert err < 1e-9, err


@pytest.mark.parametrize("sigma_att", SIGMAS)
@pytest.mark.parametrize("lam", (1e-3, 1e-6, 0.0))
@pytest.mark.parametrize("name", C.NAMES)
def test_two_routes_agree_below_a_tenth_of_the_bars(name, lam, sigma_att):
    r = C.reference(name, lam, sigma_att=sigma_att, full=True)
    print(f"FLOOR {name} lam={lam:g} sigma_att={sigma_att:g}: " + " ".join(f"{k}={v:.1e}" for k, v in r.floor.items()))
    assert r.ok
    for k, v in r.floor.items():
        assert v < 0.1 * C.BARS[k], (k, v)


def test_oracle_error_against_its_longdouble_restatement():
    """The figures the device's bars are derived from (``schur_att_cases.edge_bars``), recorded in this file's header."""
    for name in C.NAMES:
        u = C.edge_reference(name)[3]
        print(f"ORACLE UNITS {name}: " + " ".join(f"{k}={v:.1f}" for k, v in u.items()))
        assert all(np.isfinite(v) and v < 1e4 for v in u.values()), u
        assert all(b >= 16.0 for b in C.edge_bars(name).values())


def test_pose_without_rows_needs_the_factor_at_zero_damping():
    """43 / 450 at lamda = 0: pose 20 has no row, so without the attitude factor its three attitude unknowns have an empty row and
    column and the reduced system is not positive definite; with the factor it is."""
    d = C.case("43")
    st, X = d["states0"], d["Xs"]
    with pytest.raises(np.linalg.LinAlgError):
        D.step_schur(*D.normal_equations(st, X, *C.args(d), 0.0, d["time_idx"], d["sigma_dyn"]))
    dc9, _, Sm, _ = A.step_schur(*A.normal_equations(st, X, *C.args(d), 0.0, *C.factors(d)))
    assert np.linalg.eigvalsh(Sm).min() > 0 and np.isfinite(dc9).all()


@pytest.mark.parametrize("fault", A.FAULTS)
@pytest.mark.parametrize("name", ("12", "29", "12s"))
def test_planted_faults_are_past_the_bars(name, fault):
    """Each mistake moves the step past its bar (or leaves a system that is not positive definite: a rejected trial on the device).
    ``no_s`` changes nothing where every d is positive -- that is what the sign variant is for, and only there it must show."""
    good = C.reference(name, 1e-3)
    try:
        bad = C.reference(name, 1e-3, fault=fault)
    except np.linalg.LinAlgError:
        print(f"FAULT {name} {fault}: not positive definite")
        return
    off = {k: C.rel(getattr(bad, k), getattr(good, k)) for k in ("dc", "dv", "dl")}
    print(f"FAULT {name} {fault}: " + " ".join(f"{k}={v:.1e}" for k, v in off.items()))
    if fault == "no_s" and name != C.SIGN_VARIANT:
        assert max(off.values()) == 0.0
        return
    assert max(off[k] / C.BARS[k] for k in off) > 2.0, off


def test_constructor_wants_cumrot_and_sigma_att_together_and_on_a_dynamics_handle():
    from vinsat_amd.schur import SchurBA
    d = C.case("12")
    a = (d["states0"], d["X0"], d["uv"], d["w"], d["pose_of_row"], d["landmark_of_row"], d["intrinsics"])
    dyn = dict(time_idx=d["time_idx"], sigma_dyn=d["sigma_dyn"])
    with pytest.raises(ValueError, match="both or neither"):
        SchurBA(*a, cumrot=d["cumrot"], **dyn)
    with pytest.raises(ValueError, match="both or neither"):
        SchurBA(*a, sigma_att=1.0, **dyn)
    with pytest.raises(ValueError, match="only valid together with time_idx"):
        SchurBA(*a, cumrot=d["cumrot"], sigma_att=1.0)


def _write_case(path, d):
    st, c, sa = d["states0"], d["cumrot"], d["sigma_att"]
    H, g, a, J = A.attitude_blocks(st, c, sa)
    parts = [[st.shape[0], sa, 1e-10], st, c[:-1], a, J, [sa * (a * a).sum()], np.tril(H), g]
    np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in parts]).tofile(path)


def test_host_build_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """vba_schur_att_math.h compiled for the host: the per-edge body and every work item of the scatter on the sign variant of
    12 / 150 (two edges with d < 0) and on 29 / 300 against the oracle's a, J, cost, and the lower triangle and right-hand side of
    the factor."""
    src = os.path.join(ROOT, "tests", "hostcheck", "sanitize_schur_att_main.cpp")
    exe = str(tmp_path / "sanitize_schur_att_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    for name in (C.SIGN_VARIANT, "29"):
        path = str(tmp_path / f"case_{name}.bin")
        _write_case(path, C.case(name))
        p = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
        print(p.stdout, p.stderr)
        assert p.returncode == 0, p.stdout + p.stderr
        assert "sanitize_schur_att_main ok" in p.stdout and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
        if name == C.SIGN_VARIANT:
            assert "(2 edges with d < 0)" in p.stdout
