"""CPU side of the reliability query of a handle with the dynamics AND the attitude factor (``vba_schur_reliability_att``,
``SchurBA.attitude_reliability``, ``attitude_snoop``, ``attitude_outlier_power``): the reference of tests/schur_att_rel_cases.py
against itself and the conditions it must meet, the leverage table of DESIGN 9.10, the NumPy restatement of the device's attitude edge
pass and the mistakes it must be able to tell, the conditions of the planted faults the GPU test relies on, and the host build of
vinsat_amd/csrc/vba_schur_att_rel.h under the sanitizers as a stand-alone program.  No GPU.

Floors (disagreement of the reference's two NumPy routes relative to the largest entry of the family) at ``sigma_dyn`` = 1e4,
``sigma_att`` = 5e5, as measured (they move by a few tens of per cent with the BLAS and its thread count; ``12s`` equals ``12``):

  case        lam     leverage  wtest     lm_lev    lm_wtest  edge_lev  att_lev   att_wtest  att leverage min .. max (sum)      min eig I-P_a
  12 / 150    0       1.4e-10   6.2e-12   1.6e-13   2.3e-11   1.4e-10   5.4e-12   2.2e-15    1.137e-3 .. 1.174e-3 (0.01273)    0.99922
  12 / 150    1e-3    4.5e-10   1.0e-11   9.3e-14   8.3e-12   1.3e-10   8.5e-11   2.6e-14    1.137e-3 .. 1.174e-3 (0.01273)    0.99922
  29 / 300    0       4.3e-12   6.0e-13   8.1e-13   1.9e-10   6.0e-12   7.0e-12   9.3e-15    1.587e-3 .. 8.920e-3 (0.09137)    0.99167
  29 / 300    1e-3    6.9e-12   7.3e-13   5.9e-13   3.4e-11   6.9e-12   8.2e-12   1.0e-14    1.587e-3 .. 8.920e-3 (0.09137)    0.99167
  43 / 450    0       8.8e-13   5.1e-14   5.4e-14   2.6e-14   2.2e-12   3.0e-16   4.0e-16    4.56e-4 .. 1.50013 (3.02677)      0.49989
  43 / 450    1e-3    1.0e-12   5.4e-14   3.2e-14   7.0e-14   1.9e-12   1.5e-16   1.3e-16    4.56e-4 .. 1.50013 (3.02677)      0.49989
  86 / 900    0       1.8e-13   5.9e-15   1.5e-14   3.1e-14   7.1e-13   3.7e-14   7.0e-17    3.79e-4 .. 1.157e-3 (0.04192)     0.99896
  86 / 900    1e-3    1.4e-13   3.8e-15   1.7e-14   6.6e-14   6.8e-13   5.4e-14   < 1e-16    3.79e-4 .. 1.157e-3 (0.04192)     0.99896

A bar of the GPU tests is ``max(100 x floor, 1e-11)``: the floors are held below 1e-8 here so that no bar can silently grow.  No row
is left out; 2 of 300 landmarks of 29 / 300 at lamda = 0 (single-pose tracks) are held on ``lm_leverage`` only; NO attitude edge is
left out of either attitude family, and no edge's test is NaN in either route.  On 43 / 450 the two edges around pose 20, which has no
rows, carry 1.5001 each: they alone determine that pose's attitude.

Planted faults of the attitude edge pass on 29 / 300 at lamda = 1e-3 (``test_planted_faults_are_past_the_bars``), in bars of
att_leverage (8.2e-10 relative to the largest entry) / att_wtest (1e-11) / rho (1e-9 of the 1161 unknowns): J_swapped 1.1e+07 /
4.8e+06 / 1.1e+02, edge_transposed 1.1e+07 / 1.2e+06 / 1.1e+02, position_components 2.5e+14 / NaN (I - P_a is no longer positive
definite) / 1.0e+10, no_sigma 1.2e+09 / 1.0e+11 / 7.9e+04, att_not_in_rho 0 / 0 / 7.2e+07.

Planted outliers on the converged 29 / 300 with both factors: row 924 ends at ``wtest`` 52.64 against 4.50 of the runner-up and 17.80
of the largest landmark test; catalogue entry 4 at ``lm_wtest`` 6.64 against 3.82 and 3.75 of the largest row test; the largest
``att_wtest`` is 0.22 in both.  Gyro fault (``schur_att_rel_cases.gyro_fault``: ``cumrot[13]`` turned by 0.03 rad): edge 13 ends at
``att_wtest`` 10.506 against 0.203 of the runner-up (edge 2, not a neighbour: vision holds the attitudes so well -- the edge keeps
2.9966 of its 3 units of redundancy -- that little of the fault reaches edges 12 and 14: 0.103 and 0.056), a margin of 52.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import schur_att_cases as AC
import schur_att_rel_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LM_LEFT_OUT = {("29", 0.0): 2}          # single-pose tracks at lamda = 0: I - P_l exactly singular


@pytest.mark.parametrize("name,lam", T.CASES)
def test_floor_of_the_reference_and_the_conditions(name, lam):
    r, d = T.reference(name, lam), T.case(name)
    n, L, m = r.n, d["X0"].shape[0], d["uv"].shape[0]
    ident = abs(r.identity - r.unknowns) / r.unknowns
    print(f"FIGURES floor {name} lam={lam:g} " + " ".join(f"{k}={r.floor[k]:.2e}" for k in T.FAMILIES) +
          f" mineig {r.mineig.min():.3f} lm left out {int((~r.lm_kept).sum())} identity {r.identity!r} of {r.unknowns} ({ident:.1e}) rho {r.fit['rho']!r}")
    assert all(np.isfinite(r.floor[k]) for k in T.FAMILIES) and max(r.floor.values()) < 1e-8
    assert r.kept.all() and r.mineig.min() >= T.EIG_MIN                     # no row is left out (at most 1 % may be)
    assert int((~r.kept).sum()) <= T.MAX_LEFT_OUT * m
    left = int((~r.lm_kept).sum())
    assert left <= T.MAX_LM_LEFT_OUT * L and left == LM_LEFT_OUT.get((name, lam), 0)
    if left:
        track = np.bincount(d["landmark_of_row"], minlength=L)
        assert np.all(track[~r.lm_kept] == 1)
    # no attitude edge is left out of either attitude family: every value is finite in both routes, T.figures masks nothing
    for a in (r.att_leverage, r.att_leverage2, r.att_wtest, r.att_wtest2):
        assert a.shape == (n - 1,) and np.all(np.isfinite(a))
    assert ident <= 1e-9
    if lam == 0.0:
        assert np.all(d["w"] > 0) and abs(r.fit["rho"] - (2 * m - 9)) <= 1e-9 * r.unknowns
    assert abs(r.fit["omega"] - r.cost) <= 1e-12 * r.cost
    assert r.fit["omega_att"] == r.att_omega.sum() and r.fit["t_att"] == r.att_leverage.sum() and r.fit["max_att_wtest"] == r.att_wtest.max()


@pytest.mark.parametrize("name,lam", T.CASES)
def test_attitude_edges_keep_their_redundancy(name, lam):
    """The leverage table: an attitude edge has a leverage in (0, 3], I - P_a is far from singular on every edge, and the two edges at
    the pose without rows of 43 / 450 carry 1.5 each."""
    r = T.reference(name, lam)
    lev = r.att_leverage
    print(f"FIGURES attitude edges {name} lam={lam:g} leverage {lev.min():.4e} .. {lev.max():.6f} sum {lev.sum():.5f} of {3 * lev.size} "
          f"mineig(I - P_a) {r.att_mineig.min():.5f} w-test {r.att_wtest.min():.3e} .. {r.att_wtest.max():.3e}")
    assert np.all(lev > 0.0) and np.all(lev <= 3.0)
    assert r.att_mineig.min() >= T.ATT_EIG_MIN
    if name == "43":
        p = AC.EMPTY_POSE[name]
        assert abs(lev[p - 1] - 1.5) <= 1e-3 and abs(lev[p] - 1.5) <= 1e-3
        assert np.delete(lev, [p - 1, p]).max() < 0.1
    else:
        assert lev.max() < 0.1


@pytest.mark.parametrize("name,lam", T.CASES)
def test_restatement_of_the_attitude_edge_pass(name, lam):
    """Sigma6 gathered from the attitude components of the 9x9 blocks of the covariance query gives the oracle's own figures."""
    r = T.reference(name, lam)
    lev, wt = T.edge_restated(r.att_J, r.att_a, r.state, r.edges, r.sigma_att)
    fl, fw = T.rel(lev, r.att_leverage), T.rel(wt, r.att_wtest)
    print(f"FIGURES attitude edge restatement {name} lam={lam:g}: leverage {fl:.2e} (bar {T.bar(r, 'att_leverage'):.1e}) wtest {fw:.2e} "
          f"(bar {T.bar(r, 'att_wtest'):.1e})")
    assert fl <= T.bar(r, "att_leverage") and fw <= T.bar(r, "att_wtest")


@pytest.mark.parametrize("fault", T.EDGE_FAULTS)
def test_planted_faults_are_past_the_bars(fault):
    """Each mistake the attitude edge pass or its totals could make moves att_leverage, att_wtest or rho by more than 100 bars."""
    r, d = T.reference("29", 1e-3), T.case("29")
    lev, wt = T.edge_restated(r.att_J, r.att_a, r.state, r.edges, r.sigma_att, fault=fault)
    bars_lev = T.rel(lev, r.att_leverage) / T.bar(r, "att_leverage")
    with np.errstate(invalid="ignore"):
        bars_wt = T.rel(wt, r.att_wtest) / T.bar(r, "att_wtest")
    o = type(r)(**{**r.__dict__, "att_leverage": lev, "att_wtest": np.nan_to_num(wt)})
    rho = T.fit_of(d, d["Xs"], r.residual, o, r.n, fault=fault)["rho"]
    bars_rho = abs(rho - r.fit["rho"]) / (1e-9 * r.unknowns)                # (the identity's tolerance: rho is a sum of the traces)
    print(f"FAULT {fault}: att_leverage {bars_lev:.1e} bars, att_wtest {bars_wt:.1e} bars, rho {bars_rho:.1e} bars")
    assert np.nanmax([bars_lev, bars_wt, bars_rho]) > 100.0


def test_planted_row_ranks_first_in_the_oracle():
    d, r = T.planted_outlier(), T.planted_reference("row")
    order = np.argsort(-r.wtest)
    row = d["planted_row"]
    per_pose = np.bincount(d["pose_of_row"], minlength=r.n)
    print(f"FIGURES planted row {row}: first {order[:3]} {r.wtest[order[:3]]} largest landmark test {r.fit['max_lm_wtest']:.3f} "
          f"largest attitude test {r.fit['max_att_wtest']:.3f} s0sq {r.fit['s0sq']:.3f}")
    assert order[0] == row and r.wtest[order[0]] >= T.PLANT_MARGIN * max(r.wtest[order[1]], r.fit["max_lm_wtest"])
    assert per_pose[d["pose_of_row"][row]] > 6 + 1                          # the snoop's min_rows leaves room to reject it


def test_displaced_catalogue_entry_ranks_first_in_the_oracle():
    d, r = T.displaced_landmark(), T.planted_reference("landmark")
    order = np.argsort(-r.lm_wtest)
    l = d["displaced_lm"]
    track = np.bincount(d["landmark_of_row"], minlength=d["X0"].shape[0])
    print(f"FIGURES displaced landmark {l} (track {track[l]}): first {order[:3]} {r.lm_wtest[order[:3]]} largest row test {r.fit['max_wtest']:.3f}")
    assert order[0] == l and r.lm_wtest[order[0]] >= T.PLANT_MARGIN * max(r.lm_wtest[order[1]], r.fit["max_wtest"])
    assert track[l] >= 3
    per_pose = np.bincount(d["pose_of_row"], minlength=r.n)
    assert np.all(per_pose[d["pose_of_row"][d["landmark_of_row"] == l]] > 6)  # none of its poses is short


def test_gyro_fault_ranks_first_in_the_oracle():
    """The reference alone ranks the turned gap first by PLANT_MARGIN over the runner-up attitude test, and a critical value of 3.29
    separates the two with room on both sides -- scaled by s0 or not."""
    d, r = T.gyro_fault(), T.planted_reference("gyro")
    order = np.argsort(-r.att_wtest)
    e = d["gyro_edge"]
    s0 = np.sqrt(r.fit["s0sq"])
    print(f"FIGURES gyro fault edge {e}, {T.GYRO_ANGLE} rad: first {order[:3]} {r.att_wtest[order[:3]]} neighbours {r.att_wtest[[e - 1, e + 1]]} "
          f"att_leverage {r.att_leverage[e]:.4e} s0 {s0:.4f}")
    assert np.all(np.isfinite(r.att_wtest))
    assert order[0] == e and r.att_wtest[e] >= T.PLANT_MARGIN * r.att_wtest[order[1]]
    assert r.att_wtest[e] / s0 >= T.PLANT_MARGIN * 3.29 and r.att_wtest[order[1]] * T.PLANT_MARGIN <= 3.29 * min(s0, 1.0)
    assert abs(np.linalg.norm(d["cumrot"][e]) - 1.0) <= 1e-12               # (vba_schur_enable_attitude takes it)


def test_power_reference_meets_its_conditions():
    """The conditions of DESIGN 9.8 on the power reference fed with the Sigma of both factors: floors below 1e-8, at most 1 % of the rows
    and of the landmarks left out."""
    import schur_power_cases as PW
    for name, lam in T.POWER_CASES:
        r, d = T.power_reference(name, lam), T.case(name)
        print(f"FIGURES power floor {name} lam={lam:g} " + " ".join(f"{k}={r.floor[k]:.2e}" for k in PW.FAMILIES) +
              f" rows left out {r.left_out}, landmarks {r.lm_left_out}")
        assert all(np.isfinite(v) for v in r.floor.values()) and max(r.floor.values()) < 1e-8
        assert r.left_out <= PW.MAX_LEFT_OUT * d["w"].size and r.lm_left_out <= T.MAX_LM_LEFT_OUT * d["X0"].shape[0]


def test_ctypes_prototypes_and_header_agree():
    from vinsat_amd import _lib
    from vinsat_amd import schur
    sig, PD, PI = _lib.SIGNATURES, _lib.PD, ctypes.POINTER(ctypes.c_int)
    assert sig["vba_schur_reliability_att"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double] + [PD] * 12 + [PI])
    assert sig["vba_schur_snoop_att"] == sig["vba_schur_snoop_dyn"] and sig["vba_schur_outlier_power_att"] == sig["vba_schur_outlier_power_dyn"]
    for name in ("vba_schur_last_reliability_att_ms", "vba_schur_last_snoop_att_ms", "vba_schur_last_outlier_power_att_ms"):
        assert sig[name] == (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)])
    assert schur.FIT_NAMES_ATT == T.FIT_NAMES and schur.FIT_NAMES_ATT[:10] == schur.FIT_NAMES_DYN
    with open(os.path.join(ROOT, "include", "vinsat_ba.h")) as f:
        hdr = f.read()
    assert re.search(r"int vba_schur_reliability_att\(vba_schur_handle h, double lamda, double\* leverage[^;]*double\* wtest[^;]*double\* lm_leverage"
                     r"[^;]*double\* lm_wtest[^;]*double\* lm_stats[^;]*double\* pose_stats[^;]*double\* edge_leverage[^;]*double\* edge_omega"
                     r"[^;]*double\* att_leverage[^;]*double\* att_wtest[^;]*double\* att_omega[^;]*double\* fit /\*\[13\][^;]*int\* info\);", hdr)
    assert re.search(r"int vba_schur_snoop_att\(vba_schur_handle h, double lamda, double crit, int scaled, int min_rows, int min_track, int\* counts"
                     r"[^;]*double\* crit_used[^;]*int\* info\);", hdr)
    assert re.search(r"int vba_schur_outlier_power_att\(vba_schur_handle h, double lamda, double ncp, double crit, double\* mdb[^;]*double\* fit /\*\[17\]"
                     r"[^;]*int\* info\);", hdr)
    if os.path.exists(_lib.LIB_PATH):               # the built library exports them (it is loaded without a device)
        lib = ctypes.CDLL(_lib.LIB_PATH)
        for name in ("vba_schur_reliability_att", "vba_schur_snoop_att", "vba_schur_outlier_power_att", "vba_schur_last_reliability_att_ms",
                     "vba_schur_last_snoop_att_ms", "vba_schur_last_outlier_power_att_ms"):
            assert getattr(lib, name)


def test_gyro_suspects_reads_the_attitude_tests():
    from vinsat_amd.schur import gyro_suspects
    rel = dict(att_wtest=np.array([0.5, 4.0, np.nan, 9.0]), fit=dict(s0sq=4.0))
    assert np.array_equal(gyro_suspects(rel, 3.29), [1, 3])
    assert np.array_equal(gyro_suspects(rel, 3.29, scaled=True), [3])       # 4.0 / s0 = 2.0
    assert gyro_suspects(rel, float("inf")).size == 0


def test_host_build_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """vba_schur_att_rel.h compiled for the host and run edge by edge for n = 2 (the first edge of 12 / 150), 12 and 29; the leverages
    and tests it prints against the oracle's, to the bar of the case."""
    picks, recs = (("12", 2), ("12", None), ("29", None)), []
    for name, n_take in picks:
        r = T.reference(name, 1e-3)
        n = r.n if n_take is None else n_take
        recs.append(np.concatenate([[float(n), r.sigma_att], r.att_J[:n - 1].ravel(), r.att_a[:n - 1].ravel(), r.state[:n].ravel(),
                                    r.edges[:n - 1].ravel()]))
    path = str(tmp_path / "cases.bin")
    np.concatenate(recs).astype(np.float64).tofile(path)
    src = os.path.join(ROOT, "tests", "hostcheck", "sanitize_schur_att_rel_main.cpp")
    exe = str(tmp_path / "sanitize_schur_att_rel_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    p = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    print(p.stdout[-2000:], p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "sanitize_schur_att_rel_main ok (3 cases)" in p.stdout and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
    blocks = p.stdout.split("case ")[1:]
    assert len(blocks) == len(picks)
    for (name, n_take), block in zip(picks, blocks):
        r = T.reference(name, 1e-3)
        n = r.n if n_take is None else n_take
        rows = np.array([[float(x) for x in line.split()[2:4]] for line in block.splitlines() if line.startswith("edge ")])
        assert rows.shape == (n - 1, 2) and int(block.split()[0]) == n
        fl = np.abs(rows[:, 0] - r.att_leverage[:n - 1]).max() / r.att_leverage.max()
        fw = np.abs(rows[:, 1] - r.att_wtest[:n - 1]).max() / r.att_wtest.max()
        print(f"FIGURES host build {name} n={n}: leverage {fl:.2e} (bar {T.bar(r, 'att_leverage'):.1e}) wtest {fw:.2e} (bar {T.bar(r, 'att_wtest'):.1e})")
        assert fl <= T.bar(r, "att_leverage") and fw <= T.bar(r, "att_wtest")
