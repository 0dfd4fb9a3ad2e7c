"""The CPU side of the long gaps of the dynamics factor of the free-landmark mode (no GPU): the conditions the cases of
tests/schur_dyn_long_cases.py were chosen for, the floors of the oracles the GPU tests compare against, the mistakes those oracles
must be able to tell, and the host build of vinsat_amd/csrc/vba_schur_dyn_long.h (the plan) with the scatter of
vba_schur_dyn_math.h under the sanitizers as a stand-alone program.

Floors (largest disagreement of the refined full solve and the Schur route, relative to the largest entry) at ``SIGMA_DYN`` = 1e4,
measured here:

  case   lam     dc        dv        dl
  L12    1e-3    4.0e-12   1.9e-12   3.8e-12
  L12    1e-6    1.4e-11   8.3e-12   8.4e-12
  L29    1e-3    1.3e-11   1.7e-11   1.6e-11
  L29    1e-6    7.1e-12   9.6e-12   9.7e-12

every one below a tenth of the bar of 1e-7 (at sigma_dyn = 1e6 the largest is 8.2e-10).  Downstream on L12: the state covariance's
two routes agree to 9.6e-12 (scaled, lam 0 and 1e-3; its bar is 100 x that, at least 1e-11), the trial with the attitude factor on
top to 2.7e-11 at lam 1e-3 and 1.7e-11 at 1e-6 -- the existing schedules (``schur_dyn_cov_cases`` dampings 0 and 1e-3, ``LAMS``,
``schur_att_cases.SIGMA_ATT``) stand.

Planted in the long edges of L12 / L29 at lam 1e-3, each mistake is far past a bar: Phi multiplied in reversed order moves dc by 0.3
of its largest entry, the residual against the start pose by 2e3, a long edge left out of the cost moves c0 by a third.
"""
import os
import subprocess

import numpy as np
import pytest

import schur_dyn_long_cases as L
import schur_dyn_oracle as D
from oracle import ba_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("lam", L.LAMS)
@pytest.mark.parametrize("name", L.NAMES)
def test_two_routes_agree_below_a_tenth_of_the_bars(name, lam):
    r = L.reference(name, lam, full=True)
    print(f"FLOOR {name} lam={lam:g}: " + " ".join(f"{k}={v:.1e}" for k, v in r.floor.items()))
    assert r.ok                                     # every trial is accepted
    for k, v in r.floor.items():
        assert v < 0.1 * L.BARS[k], (k, v)


def test_cases_are_what_their_names_say():
    d12, d29 = L.case("L12"), L.case("L29")
    g12, g29 = np.diff(d12["time_idx"]), np.diff(d29["time_idx"])
    assert list(g12) == [1, 5, 65, 1, 64, 935, 1, 3, 510, 1, 2] and list(d12["long"]) == [2, 5, 8]
    assert any(g12[k] > 64 and np.all(g12[k + 1:] <= 64) for k in range(g12.size - 1))      # a long edge is the last before short ones
    assert g29.size == 28 and g29.max() == 1024 and list(d29["long"]) == [k for k in range(28) if g29[k] in (66, 1024, 129)]
    assert max(g12.max(), g29.max()) <= 1024        # trial cases: the chain is within rounding of the serial walk
    for d in (d12, d29):
        n = d["states0"].shape[0]
        assert np.bincount(d["pose_of_row"], minlength=n).min() > 0         # every pose has rows
        assert np.abs(O.orbit_factor(d["states_gt"], d["time_idx"], jacobian=False)).max() < 1e-7   # the truth is the exact chain
    panels = lambda N: (N + 255) // 256
    assert panels(9 * 12) == 1 and panels(9 * 29) == 2
    for gaps in L.FACTOR_GAPS:
        d = L.factor_window(gaps)
        assert list(np.diff(d["time_idx"])) == [5] + list(gaps) + [4] and list(d["long"]) == [1 + k for k, g in enumerate(gaps) if g > 64]
    # the plans (L, P, sub, nsubL, G) at the threshold, the two-pass gap and either side of 1024: one wavefront's chunks, <= 128 sub-chunks
    assert L.long_plan(65) == (8, 9, 8, 1, 9) and L.long_plan(935) == (27, 35, 9, 3, 104)
    assert L.long_plan(1024) == (28, 37, 10, 3, 110) and L.long_plan(1025) == (28, 37, 10, 3, 110)
    for s in (65, 66, 129, 510, 935, 1024, 1025, 2000, 3000, 2 ** 20):
        _, P, _, _, G = L.long_plan(s)
        assert 1 <= P <= 64 and G <= 128, s


@pytest.mark.parametrize("fault", L.FAULTS)
@pytest.mark.parametrize("name", L.NAMES)
def test_planted_faults_in_long_edges_are_past_the_bars(name, fault):
    good = L.reference(name, 1e-3)
    try:
        bad = L.reference(name, 1e-3, fault=fault)
    except np.linalg.LinAlgError:
        print(f"FAULT {name} {fault}: not positive definite")
        return
    off = {k: L.rel(getattr(bad, k), getattr(good, k)) for k in ("dc", "dv", "dl")}
    off["c0"], off["c1"] = abs(bad.c0 - good.c0) / good.c0, abs(bad.c1 - good.c1) / good.c1
    print(f"FAULT {name} {fault}: " + " ".join(f"{k}={v:.1e}" for k, v in off.items()))
    assert max(off[k] / L.BARS[k] for k in off) > 2.0, off


def test_downstream_oracle_floors_on_L12():
    """The state covariance and the trial with the attitude factor on top, before the GPU tests use them on L12: both floors below a
    tenth of the bars those tests hold.  (``schur_dyn_cov_cases.bar`` is 100 x the floor, at least 1e-11: a tenth of it is above the
    floor by construction, so the floor is also held below 1e-10 -- a well-conditioned system, as on the cases of DESIGN 9.6.)"""
    import schur_dyn_cov_cases as V
    for lam in (0.0, 1e-3):
        r = L.cov_reference("L12", lam)
        print(f"FLOOR cov L12 lam={lam:g}: " + " ".join(f"{k}={v:.1e}" for k, v in r.floor.items()))
        for k in V.FAMILIES:
            assert r.floor[k] < 0.1 * V.bar(r, k) and r.floor[k] < 1e-10, (lam, k)
    for lam in L.LAMS:
        r = L.att_reference("L12", lam, full=True)
        print(f"FLOOR att L12 lam={lam:g}: " + " ".join(f"{k}={v:.1e}" for k, v in r.floor.items()))
        assert r.ok
        for k, v in r.floor.items():
            assert v < 0.1 * L.BARS[k], (k, v)


def test_constructor_wants_the_dynamics_arguments_with_long_gaps():
    from vinsat_amd.schur import SchurBA
    d = L.case("L12")
    a = (d["states0"], d["X0"], d["uv"], d["w"], d["pose_of_row"], d["landmark_of_row"], d["intrinsics"])
    with pytest.raises(ValueError, match="long_gaps is an option of the dynamics factor"):
        SchurBA(*a, long_gaps=True)


def _write_case(path, d, lam):
    st, t, sd = d["states0"], d["time_idx"], d["sigma_dyn"]
    n = st.shape[0]
    H, g, r, E = D.dynamics_blocks(st, t, sd)
    H[6 * n:, 6 * n:] += lam * np.eye(3 * n)
    A = np.concatenate([E[:, :, 0:3], E[:, :, 6:9]], -1)
    parts = [[n, sd, lam, 1e-10], np.diff(t), r, A, np.tril(H), g]
    np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in parts]).tofile(path)


def test_host_build_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The plan of vba_schur_dyn_long.h and the scatter of vba_schur_dyn_math.h compiled for the host, on L12, L29 and the window
    with gaps (1025, 2, 2000): marks, slots and pool against their definitions, the lower triangle and right-hand side of the factor
    with long-gap A and r against the oracle's."""
    src = os.path.join(ROOT, "tests", "hostcheck", "sanitize_schur_dyn_long_main.cpp")
    exe = str(tmp_path / "sanitize_schur_dyn_long_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    for key, d in (("L12", L.case("L12")), ("L29", L.case("L29")), ("over-1024", L.factor_window((1025, 2, 2000)))):
        path = str(tmp_path / f"case_{key}.bin")
        _write_case(path, d, 1e-3)
        p = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
        print(p.stdout, p.stderr)
        assert p.returncode == 0, p.stdout + p.stderr
        assert "sanitize_schur_dyn_long_main ok" in p.stdout and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
        assert f"{d['long'].size} long edges" in p.stdout
