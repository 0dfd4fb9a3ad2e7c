"""The CPU side of the dynamics factor of the free-landmark mode (no GPU): the oracle of tests/schur_dyn_oracle.py against itself
-- its two routes, its gradient, the mistakes it must be able to tell -- and the host build of vinsat_amd/csrc/vba_schur_dyn_math.h
under the sanitizers as a stand-alone program.

Floors (largest disagreement of the refined full solve and the Schur route, relative to the largest entry), at
``schur_dyn_cases.SIGMA_DYN`` = 1e4, measured here:

  case        lam     dc        dv        dl
  12 / 150    1e-3    3.2e-11   4.6e-10   4.7e-12
  12 / 150    1e-6    4.2e-12   3.7e-11   3.6e-12
  29 / 300    1e-3    4.2e-12   1.2e-11   4.2e-12
  29 / 300    1e-6    3.6e-12   1.6e-11   2.3e-12
  43 / 450    1e-3    1.0e-12   4.4e-12   2.3e-12
  43 / 450    1e-6    1.5e-12   1.2e-11   3.6e-12
  86 / 900    1e-3    1.2e-12   5.9e-12   7.2e-12
  86 / 900    1e-6    1.4e-12   1.0e-11   2.4e-12

every one below a tenth of the bar of 1e-7 (at sigma_dyn = 1e6, the other end of the fixed-landmark path's schedule, the largest
is 8.3e-10: the condition holds there too).
"""
import os
import subprocess

import numpy as np
import pytest

import schur_dyn_cases as C
import schur_dyn_oracle as D
from oracle import ba_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("lam", C.LAMS)
@pytest.mark.parametrize("name", C.NAMES)
def test_two_routes_agree_below_a_tenth_of_the_bars(name, lam):
    r = C.reference(name, lam, full=True)
    print(f"FLOOR {name} lam={lam:g}: " + " ".join(f"{k}={v:.1e}" for k, v in r.floor.items()))
    assert r.ok
    for k, v in r.floor.items():
        assert v < 0.1 * C.BARS[k], (k, v)


def test_cases_are_what_their_names_say():
    for name, (n, _) in C._SHAPES.items():
        d = C.case(name)
        gaps = np.diff(d["time_idx"])
        assert d["states0"].shape[0] == n and gaps.min() >= 1 and gaps.max() <= 64
        # at the truth the dynamics residual is rounding
        assert np.abs(O.orbit_factor(d["states_gt"], d["time_idx"], jacobian=False)).max() < 1e-8
    assert set(np.diff(C.case("12")["time_idx"])) == {1}
    g = np.diff(C.case("29")["time_idx"])
    assert {1, 5, 64} == set(g) and any(g[k] == 64 and g[k + 1] == 1 for k in range(g.size - 1))
    assert not np.any(C.case("43")["pose_of_row"] == C.EMPTY_POSE["43"])
    panels = lambda N: (N + 255) // 256
    assert (panels(6 * 29), panels(9 * 29)) == (1, 2) and (panels(6 * 43), panels(9 * 43)) == (2, 2) and panels(9 * 86) == 4 and panels(9 * 12) == 1


def test_gradient_of_the_cost_by_central_differences():
    """v9 and wl of the normal equations are minus half the gradient of the cost, in position, attitude, velocity and landmark.
    Attitude: the reference's Jacobian is that of ``q (x) [delta; 1]`` (``attitude_jacobian``) while its retraction is the half-angle
    exponential (``qexp``: ``[delta / 2; 1]`` to first order), so along the retraction the cost moves half as fast as the Jacobian
    says -- the reference's own convention, kept by both oracles and the device: the difference quotient is doubled for that group."""
    d = C.case("12")
    st, X, t, sd = d["states0"], d["Xs"], d["time_idx"], d["sigma_dyn"]
    n, L = st.shape[0], X.shape[0]
    _, _, _, v9, wl = D.normal_equations(st, X, *C.args(d), 0.0, t, sd)
    grad = np.concatenate([v9, wl])
    idx = D.unknown_index(n)
    groups = dict(position=(idx[[0, 5, n - 1], :3].ravel(), 1e-4), attitude=(idx[[0, 5, n - 1], 3:6].ravel(), 1e-7),
                  velocity=(idx[[0, 5, n - 1], 6:].ravel(), 1e-6), landmark=(9 * n + np.array([0, 1, 2, 3 * (L // 2) + 1, 3 * L - 1]), 1e-4))
    for gname, (unknowns, h) in groups.items():
        num = []
        for u in unknowns:
            c = []
            for sgn in (1.0, -1.0):
                step = np.zeros(9 * n + 3 * L)
                step[u] = sgn * h
                s1, X1 = D.apply_step(st, X, step[:9 * n], step[9 * n:])
                c.append(D.cost(s1, X1, *C.args(d), t, sd))
            num.append(-(c[0] - c[1]) / (2 * h) / 2 * (2.0 if gname == "attitude" else 1.0))
        err = np.abs(np.array(num) - grad[unknowns]).max() / np.abs(grad[unknowns]).max()
        print(f"GRADIENT {gname}: {err:.1e}")
        assert err < 1e-5, (gname, err)


@pytest.mark.parametrize("fault", D.FAULTS)
@pytest.mark.parametrize("name", ("12", "29"))
def test_planted_faults_are_past_the_bars(name, fault):
    """Each mistake moves the step past its bar (or leaves a system that is not positive definite: a rejected trial on the device).
    The smallest: the untransposed (p_{i+1}, v_i) block on gaps of one second, where that block is -sigma D Phi_pv ~ -sigma I and
    symmetric to 1e-7 -- dv is 2.4 bars off there and 1.5e4 bars on the mixed gaps of 29 / 300."""
    good = C.reference(name, 1e-3)
    try:
        bad = C.reference(name, 1e-3, fault=fault)
    except np.linalg.LinAlgError:
        print(f"FAULT {name} {fault}: not positive definite")
        return
    off = {k: C.rel(getattr(bad, k), getattr(good, k)) for k in ("dc", "dv", "dl")}
    print(f"FAULT {name} {fault}: " + " ".join(f"{k}={v:.1e}" for k, v in off.items()))
    assert max(off[k] / C.BARS[k] for k in off) > 2.0, off


def test_constructor_wants_time_idx_and_sigma_dyn_together():
    from vinsat_amd.schur import SchurBA
    d = C.case("12")
    a = (d["states0"], d["X0"], d["uv"], d["w"], d["pose_of_row"], d["landmark_of_row"], d["intrinsics"])
    with pytest.raises(ValueError, match="both or neither"):
        SchurBA(*a, time_idx=d["time_idx"])
    with pytest.raises(ValueError, match="both or neither"):
        SchurBA(*a, sigma_dyn=1.0)


def _write_case(path, d, lam):
    st, t, sd = d["states0"], d["time_idx"], d["sigma_dyn"]
    n = st.shape[0]
    H, g, r, E = D.dynamics_blocks(st, t, sd)
    H[6 * n:, 6 * n:] += lam * np.eye(3 * n)
    A = np.concatenate([E[:, :, 0:3], E[:, :, 6:9]], -1)
    parts = [[n, sd, lam, 1e-10], st, np.diff(t), r, A, [sd * (r * r).sum()], np.tril(H), g]
    np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in parts]).tofile(path)


def test_host_build_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """vba_schur_dyn_math.h compiled for the host: the per-edge body and every work item of the scatter on 12 / 150 and 29 / 300
    (gaps of 1, 5 and 64 steps) against the oracle's r, D Phi, cost, and the lower triangle and right-hand side of the factor."""
    src = os.path.join(ROOT, "tests", "hostcheck", "sanitize_schur_dyn_main.cpp")
    exe = str(tmp_path / "sanitize_schur_dyn_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    for name in ("12", "29"):
        path = str(tmp_path / f"case_{name}.bin")
        _write_case(path, C.case(name), 1e-3)
        p = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
        print(p.stdout, p.stderr)
        assert p.returncode == 0, p.stdout + p.stderr
        assert "sanitize_schur_dyn_main ok" in p.stdout and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
