"""CPU side of the reliability query of a handle with the dynamics factor (``vba_schur_reliability_dyn``,
``SchurBA.state_reliability``, ``SchurBA.state_snoop``): the reference of tests/schur_dyn_rel_cases.py against itself, the NumPy
restatement of the device's edge pass and the mistakes it must be able to tell, the conditions of the planted outliers the GPU test
relies on, and the host build of vinsat_amd/csrc/vba_schur_dyn_rel.h under the sanitizers as a stand-alone program.  No GPU.

Floors (disagreement of the reference's two NumPy routes relative to the largest entry of the family) at
``schur_dyn_cases.SIGMA_DYN`` = 1e4, as measured (they move by a few tens of per cent with the BLAS and its thread count):

  case        lam     leverage  wtest     lm_lev    lm_wtest  edge_lev  min eig I-P_k  identity (of 9n+3L)
  12 / 150    0       2.7e-10   7.2e-12   2.0e-13   1.5e-11   1.5e-10   0.908          1.9e-12
  12 / 150    1e-3    1.5e-10   3.9e-12   1.1e-13   1.7e-11   1.2e-10   0.908          1.8e-12
  29 / 300    0       5.9e-12   6.0e-13   2.0e-13   3.1e-10   2.5e-12   0.659          6.8e-14
  29 / 300    1e-3    2.2e-12   1.6e-13   8.2e-14   1.1e-10   1.1e-11   0.659          5.8e-14
  43 / 450    1e-3    1.4e-12   8.0e-14   3.0e-14   2.5e-14   1.2e-12   0.896          9.8e-15
  86 / 900    0       1.5e-13   4.5e-15   1.1e-14   3.7e-14   7.5e-13   0.915          2.4e-15
  86 / 900    1e-3    2.6e-13   4.7e-15   8.0e-15   1.7e-14   5.0e-13   0.915          3.9e-16

A bar of the GPU tests is ``max(100 x floor, 1e-11)``: the floors are held below 1e-8 here so that no bar can silently grow.  No row
is left out; 2 of 300 landmarks of 29 / 300 at lamda = 0 (single-pose tracks) are held on ``lm_leverage`` only.

Why there is no w-test of an edge (``test_edges_have_a_leverage_and_no_test``, ``test_routes_disagree_on_the_edge_wtest``): the edge leverages lie between 5.894 and 5.9987 of 6
(redundancy of all edges together: 0.18 of 66 on 12 / 150, 0.41 of 168 on 29 / 300, 2.2 of 252 on 43 / 450, 7.4 of 510 on 86 / 900), the
smallest eigenvalue of ``I - P_e`` per case between -4.7e-10 and 1.0e-11, and the two routes' ``sqrt(sigma r^T (I - P_e)^-1 r)``
disagree, per edge and relative to the larger of the two, by 7.9e-3 (NaN on 2 edges), 0.83 (1), 0.52, 1.4e-3, 1.8e-3, 9.9e-8 (NaN on
2 edges) and 3.5e-3 on the seven pairs in the order above.  Those figures are rounding noise: with another BLAS thread count 29 / 300
at 1e-3 gave 8.6e-4.  So the eigenvalue is held per pair and the disagreement of more than 1e-3 over the seven pairs together
(``test_routes_disagree_on_the_edge_wtest``).

Planted faults of the edge pass on 29 / 300 at lamda = 1e-3 (``test_planted_faults_are_past_the_bars``), in bars of edge_leverage
(1.1e-9 relative to 6) and of rho (1e-9 of the 1161 unknowns): edge_transposed 4.3e+10 / 1.5e+09, no_velocity_columns 2.0e+10 /
6.3e+08, same_state 1.1e+11 / 8.9e+07, no_sigma 8.8e+08 / 1.4e+08, edges_not_in_rho 0 / 3.5e+05.

Planted outliers on the converged 29 / 300: row 924 (pose 19, 69 rows) ends at ``wtest`` 52.6 against 4.50 of the runner-up and 17.8 of
the largest landmark test (its own landmark, which absorbs part of it); catalogue entry 4 at ``lm_wtest`` 6.64 against 3.82 and 3.75
of the largest row test (why entry 4 and not the seeded choice: ``schur_dyn_rel_cases.displaced_landmark``).
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import schur_dyn_rel_cases as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LM_LEFT_OUT = {("29", 0.0): 2}          # single-pose tracks at lamda = 0: I - P_l exactly singular


@pytest.mark.parametrize("name,lam", Q.CASES)
def test_floor_of_the_reference(name, lam):
    r, d = Q.reference(name, lam), Q.case(name)
    n, L, m = r.n, d["X0"].shape[0], d["uv"].shape[0]
    ident = abs(r.identity - r.unknowns) / r.unknowns
    print(f"FIGURES floor {name} lam={lam:g} " + " ".join(f"{k}={r.floor[k]:.2e}" for k in Q.FAMILIES) +
          f" mineig {r.mineig.min():.3f} lm left out {int((~r.lm_kept).sum())} identity {r.identity!r} of {r.unknowns} ({ident:.1e}) rho {r.fit['rho']!r}")
    assert all(np.isfinite(r.floor[k]) for k in Q.FAMILIES) and max(r.floor.values()) < 1e-8
    assert r.kept.all() and r.mineig.min() >= Q.EIG_MIN                     # no row is left out
    left = int((~r.lm_kept).sum())
    assert left <= Q.MAX_LM_LEFT_OUT * L and left == LM_LEFT_OUT.get((name, lam), 0)
    if left:
        track = np.bincount(d["landmark_of_row"], minlength=L)
        assert np.all(track[~r.lm_kept] == 1)
    assert ident <= 1e-9
    if lam == 0.0:
        assert np.all(d["w"] > 0) and abs(r.fit["rho"] - (2 * m - 3 * n - 6)) <= 1e-9 * r.unknowns
    assert abs(r.fit["omega"] - r.cost) <= 1e-12 * r.cost
    assert r.fit["omega_edges"] == r.edge_omega.sum() and r.fit["t_edges"] == r.edge_leverage.sum()


def _edge_wtest_disagreement(r):
    """(largest disagreement of the two routes' edge w-tests per edge, relative to the larger of the two; edges where one is NaN)"""
    with np.errstate(invalid="ignore"):
        both = np.isfinite(r.edge_wtest) & np.isfinite(r.edge_wtest2)
        a, b = r.edge_wtest[both], r.edge_wtest2[both]
        dis = float((np.abs(a - b) / np.maximum(np.abs(a), np.abs(b))).max()) if both.any() else float("inf")
    return dis, int((~both).sum())


@pytest.mark.parametrize("name,lam", Q.CASES)
def test_edges_have_a_leverage_and_no_test(name, lam):
    """The leverage of an edge is well conditioned and close to 6 (the edges carry next to no redundancy); its w-test divides by
    what is left of I - P_e, whose smallest eigenvalue is rounding (1e-11 at the most, of either sign, against entries of order 1)."""
    r = Q.reference(name, lam)
    lev = r.edge_leverage
    dis, nans = _edge_wtest_disagreement(r)
    print(f"FIGURES edges {name} lam={lam:g} leverage {lev.min():.4f} .. {lev.max():.6f} redundancy {6 * lev.size - lev.sum():.3f} of {6 * lev.size} "
          f"mineig(I - P_e) {r.edge_mineig.min():.1e} .. {r.edge_mineig.max():.1e} edge w-test: routes disagree by {dis:.1e}, NaN on {nans} edges")
    assert np.all(lev > 5.8) and np.all(lev < 6.0)
    assert r.edge_mineig.min() < 1e-9               # an inverse through it keeps 7 of 16 digits at the most


def test_routes_disagree_on_the_edge_wtest():
    """The recorded reason for leaving the edge w-test out: the two routes' values disagree by more than 1e-3.  Held over the seven
    pairs together: the figure of one pair is rounding noise (29 / 300 at 1e-3 gave 1.4e-3 with one BLAS thread count and 8.6e-4 with
    another), the worst of them is not (0.5 to 0.8 on 12 / 150 at 1e-3 and 29 / 300 at 0, NaN on edges of three pairs)."""
    figs = {c: _edge_wtest_disagreement(Q.reference(*c)) for c in Q.CASES}
    print("FIGURES edge w-test, routes disagree by (NaN edges): " + ", ".join(f"{n} lam={l:g}: {d:.1e} ({k})" for (n, l), (d, k) in figs.items()))
    assert max(d for d, _ in figs.values()) > 1e-3
    assert sum(d > 1e-3 or k > 0 for d, k in figs.values()) >= 4        # ... and on most pairs, not on one


@pytest.mark.parametrize("name,lam", Q.CASES)
def test_restatement_of_the_edge_pass(name, lam):
    """Sigma12 gathered from the 9x9 blocks of the covariance query and J = [D Phi | -D] give the oracle's own edge leverage."""
    r = Q.reference(name, lam)
    got = Q.edge_restated(r.edge_A, r.state, r.edges, r.sigma_dyn)
    fig = Q.rel(got, r.edge_leverage)
    print(f"FIGURES edge restatement {name} lam={lam:g}: {fig:.2e} (bar {Q.bar(r, 'edge_leverage'):.1e})")
    assert fig <= Q.bar(r, "edge_leverage")


@pytest.mark.parametrize("fault", Q.EDGE_FAULTS)
def test_planted_faults_are_past_the_bars(fault):
    """Each mistake the edge pass or its totals could make moves edge_leverage or rho by at least ten bars on 29 / 300."""
    r, d = Q.reference("29", 1e-3), Q.case("29")
    got = Q.edge_restated(r.edge_A, r.state, r.edges, r.sigma_dyn, fault=fault)
    bars_lev = Q.rel(got, r.edge_leverage) / Q.bar(r, "edge_leverage")
    o = type(r)(**{**r.__dict__, "edge_leverage": got})
    rho = Q.fit_of(d, d["Xs"], r.residual, o, r.n, fault=fault)["rho"]
    bars_rho = abs(rho - r.fit["rho"]) / (1e-9 * r.unknowns)                # (the identity's tolerance: rho is a sum of the traces)
    print(f"FAULT {fault}: edge_leverage {bars_lev:.1e} bars, rho {bars_rho:.1e} bars")
    assert max(bars_lev, bars_rho) >= 10.0


def test_planted_row_ranks_first_in_the_oracle():
    d, r = Q.planted_outlier(), Q.planted_reference("row")
    order = np.argsort(-r.wtest)
    row = d["planted_row"]
    per_pose = np.bincount(d["pose_of_row"], minlength=r.n)
    print(f"FIGURES planted row {row} (pose {d['pose_of_row'][row]} with {per_pose[d['pose_of_row'][row]]} rows): first {order[:3]} "
          f"{r.wtest[order[:3]]} largest landmark test {r.fit['max_lm_wtest']:.3f} s0sq {r.fit['s0sq']:.3f}")
    assert order[0] == row and r.wtest[order[0]] >= Q.PLANT_MARGIN * max(r.wtest[order[1]], r.fit["max_lm_wtest"])
    assert per_pose[d["pose_of_row"][row]] > 6 + 1                          # the snoop's min_rows leaves room to reject it


def test_displaced_catalogue_entry_ranks_first_in_the_oracle():
    d, r = Q.displaced_landmark(), Q.planted_reference("landmark")
    order = np.argsort(-r.lm_wtest)
    l = d["displaced_lm"]
    track = np.bincount(d["landmark_of_row"], minlength=d["X0"].shape[0])
    print(f"FIGURES displaced landmark {l} (track {track[l]}): first {order[:3]} {r.lm_wtest[order[:3]]} largest row test {r.fit['max_wtest']:.3f}")
    assert order[0] == l and r.lm_wtest[order[0]] >= Q.PLANT_MARGIN * max(r.lm_wtest[order[1]], r.fit["max_wtest"])
    assert track[l] >= 3
    per_pose = np.bincount(d["pose_of_row"], minlength=r.n)
    assert np.all(per_pose[d["pose_of_row"][d["landmark_of_row"] == l]] > 6)  # none of its poses is short


def test_ctypes_prototypes_and_header_agree():
    from vinsat_amd import _lib
    from vinsat_amd import schur
    sig, PD, PI = _lib.SIGNATURES, _lib.PD, ctypes.POINTER(ctypes.c_int)
    assert sig["vba_schur_reliability_dyn"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double] + [PD] * 9 + [PI])
    assert sig["vba_schur_snoop_dyn"] == sig["vba_schur_snoop"]
    for name in ("vba_schur_last_reliability_dyn_ms", "vba_schur_last_snoop_dyn_ms"):
        assert sig[name] == (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)])
    assert schur.FIT_NAMES_DYN == Q.FIT_NAMES and schur.FIT_NAMES_DYN[:8] == schur.FIT_NAMES
    with open(os.path.join(ROOT, "include", "vinsat_ba.h")) as f:
        hdr = f.read()
    assert re.search(r"int vba_schur_reliability_dyn\(vba_schur_handle h, double lamda, double\* leverage[^;]*double\* wtest[^;]*double\* lm_leverage"
                     r"[^;]*double\* lm_wtest[^;]*double\* lm_stats[^;]*double\* pose_stats[^;]*double\* edge_leverage[^;]*double\* edge_omega"
                     r"[^;]*double\* fit /\*\[10\][^;]*int\* info\);", hdr)
    assert re.search(r"int vba_schur_snoop_dyn\(vba_schur_handle h, double lamda, double crit, int scaled, int min_rows, int min_track, int\* counts"
                     r"[^;]*double\* crit_used[^;]*int\* info\);", hdr)
    if os.path.exists(_lib.LIB_PATH):               # the built library exports them (it is loaded without a device)
        lib = ctypes.CDLL(_lib.LIB_PATH)
        assert lib.vba_schur_reliability_dyn and lib.vba_schur_snoop_dyn and lib.vba_schur_last_reliability_dyn_ms and lib.vba_schur_last_snoop_dyn_ms


def test_host_build_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """vba_schur_dyn_rel.h compiled for the host and run lane by lane for n = 2 (the first edge of 12 / 150), 12 and 29 against the
    oracle's edge leverages, to the bar of the case, and against the dense product the program forms itself."""
    recs = []
    for name, n_take in (("12", 2), ("12", None), ("29", None)):
        r = Q.reference(name, 1e-3)
        n = r.n if n_take is None else n_take
        recs.append(np.concatenate([[float(n), r.sigma_dyn, Q.bar(r, "edge_leverage")], r.edge_A[:n - 1].ravel(), r.state[:n].ravel(),
                                    r.edges[:n - 1].ravel(), r.edge_leverage[:n - 1]]))
    path = str(tmp_path / "cases.bin")
    np.concatenate(recs).astype(np.float64).tofile(path)
    src = os.path.join(ROOT, "tests", "hostcheck", "sanitize_schur_dyn_rel_main.cpp")
    exe = str(tmp_path / "sanitize_schur_dyn_rel_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    p = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "sanitize_schur_dyn_rel_main ok (3 cases)" in p.stdout and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
