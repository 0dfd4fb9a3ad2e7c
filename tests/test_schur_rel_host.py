"""CPU side of the free-landmark reliability query (``vba_schur_reliability``): the reference of tests/schur_rel_cases.py against
itself, the identities it must satisfy, the planted faults, and the closed forms of vinsat_amd/csrc/vba_schur_rel_math.h compiled
for the host against LAPACK.  No GPU.

Floors (disagreement of the reference's two NumPy routes, relative to the largest entry of the family), as measured:

  case                          lam    leverage   wtest      lm_leverage  lm_wtest   left out (rows / landmarks)
  12 / 150                      0      5.6e-13    4.1e-14    1.6e-14      6.5e-14    0 / 0
  12 / 150                      1e-3   1.1e-12    7.4e-14    1.8e-14      7.2e-14    0 / 0
  43 / 450                      1e-3   5.1e-13    7.1e-14    4.6e-15      4.7e-14    0 / 0
  129 / 1300                    1e-3   4.9e-13    4.5e-14    7.3e-15      4.0e-14    0 / 0
  wide                          1e-3   9.1e-14    1.2e-14    8.5e-15      4.6e-14    0 / 0
  pose_without_rows             1e-3   4.2e-13    3.0e-14    8.5e-15      3.7e-14    0 / 0
  more_landmarks_than_rows      0      2.2e-13    6.6e-14    5.6e-15      6.1e-13    0 / 37 of 400 (the tracks of one row)
  more_poses_than_landmarks     1e-3   7.2e-12    5.9e-12    2.6e-13      3.6e-12    0 / 0
  zero_weights                  1e-3   1.6e-13    2.4e-14    2.8e-15      7.8e-14    0 / 0
  behind_the_camera             1e4    2.3e-11    1.5e-14    6.9e-10      1.4e-11    5 of 1474 (the clamped rows) / 0

(they move by a few tens of per cent with the BLAS and its thread count).  A bar of the GPU tests is ``max(100 x floor, 1e-11)``.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import schur_rel_cases as R
from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "hostcheck", "hostcheck_schur_rel.cpp")
LIB = os.path.join(ROOT, "tests", "hostcheck", "libhostcheck_schur_rel.so")
P = ctypes.POINTER(ctypes.c_double)
EPS = np.finfo(np.float64).eps
SMALL = ("12", "43", "pose_without_rows", "more_landmarks_than_rows", "more_poses_than_landmarks", "zero_weights", "behind_the_camera")


@pytest.mark.parametrize("name,lam", R.CASES)
def test_floor_of_the_reference(name, lam):
    r = R.reference(name, lam)
    out, lm_out = int((~r.kept).sum()), int((~r.lm_kept).sum())
    print(f"FIGURES rel floor {name} lam={lam:g} " + " ".join(f"{k}={r.floor[k]:.2e}" for k in R.FAMILIES) +
          f" left out {out} of {r.kept.size} rows, {lm_out} of {r.lm_kept.size} landmarks; smallest eigenvalue kept {r.mineig[r.kept].min():.2e}")
    assert all(np.isfinite(r.floor[k]) and r.floor[k] < 1e-8 for k in R.FAMILIES)
    assert out <= R.MAX_LEFT_OUT * r.kept.size
    if name == "behind_the_camera":
        assert out == 5 and r.leverage.max() > 1.9999
    else:
        assert out == 0 and r.mineig.min() >= 0.19
    assert lm_out == (37 if name == "more_landmarks_than_rows" else 0)
    assert np.all(np.isfinite(r.wtest[r.kept])) and np.all(np.isfinite(r.lm_wtest[r.lm_kept]))


@pytest.mark.parametrize("name,lam", [c for c in R.CASES if c[0] in SMALL])
def test_identities_of_the_reference(name, lam):
    r, d = R.reference(name, lam), R.problem(name)
    ident = r.fit["t_rows"] + r.fit["t_prior"] + lam * r.trace_Hinv
    print(f"FIGURES rel identity {name} lam={lam:g}: {ident!r} of {r.unknowns}; leverage {r.leverage.min():.3e} .. {r.leverage.max():.6f}, "
          f"lm_leverage {r.lm_leverage.min():.3e} .. {r.lm_leverage.max()!r}, rho {r.fit['rho']!r}")
    assert abs(ident - r.unknowns) <= (3e-12 if lam == 0.0 else 1e-9) * r.unknowns
    assert np.all(r.leverage >= 0.0) and np.all(r.leverage < 2.0)
    assert np.all(r.lm_leverage > 0.0) and np.all(r.lm_leverage <= 3.0 * (1.0 + 4.0 * EPS))       # (3 itself for a landmark without rows, to rounding)
    if lam == 0.0 and np.all(d["w"] > 0.0):
        m, n = d["uv"].shape[0], d["states0"].shape[0]
        assert abs(r.fit["rho"] - (2 * m - 6 * n)) <= 3e-12 * r.unknowns
    assert np.array_equal(r.leverage[d["w"] == 0.0], np.zeros(int((d["w"] == 0.0).sum())))


def test_identity_sums_as_the_issue_states_them():
    assert R.reference("12", 0.0).unknowns == 522 and R.reference("43", 1e-3).unknowns == 1608
    assert R.reference("more_landmarks_than_rows", 0.0).unknowns == 1272


def test_planted_outlier_ranks_first_in_the_oracle():
    d, r = R.planted_outlier(), R.planted_reference("row")
    order = np.argsort(-r.wtest)
    print(f"FIGURES rel planted row {d['planted_row']}: first {order[:3]} {r.wtest[order[:3]]}, raw residual rank "
          f"{int((np.abs(r.residual).max(1) > np.abs(r.residual[d['planted_row']]).max()).sum())}")
    assert order[0] == d["planted_row"] and r.wtest[order[0]] > 5.0 * r.wtest[order[1]]
    from vinsat_amd.schur import suspects
    rows, lms = suspects(dict(wtest=r.wtest, lm_wtest=r.lm_wtest, fit=r.fit), 0.5 * (r.wtest[order[0]] + r.wtest[order[1]]))
    assert np.array_equal(rows, [d["planted_row"]]) and lms.size == 0


def test_displaced_catalogue_entry_ranks_first_in_the_oracle():
    d, r = R.displaced_landmark(), R.planted_reference("lm")
    order = np.argsort(-r.lm_wtest)
    print(f"FIGURES rel displaced landmark {d['displaced_lm']}: first {order[:3]} {r.lm_wtest[order[:3]]}, largest row test {r.fit['max_wtest']:.3f}")
    assert order[0] == d["displaced_lm"] and r.lm_wtest[order[0]] > r.fit["max_wtest"]
    from vinsat_amd.schur import suspects
    rel = dict(wtest=r.wtest, lm_wtest=r.lm_wtest, fit=r.fit)
    rows, lms = suspects(rel, 0.5 * (r.lm_wtest[order[0]] + max(r.lm_wtest[order[1]], r.fit["max_wtest"])))
    assert rows.size == 0 and np.array_equal(lms, [d["displaced_lm"]])
    s = np.sqrt(r.fit["s0sq"])
    rows2, lms2 = suspects(rel, 5.0 / s, scaled=True)
    rows3, lms3 = suspects(rel, 5.0)
    assert np.array_equal(rows2, rows3) and np.array_equal(lms2, lms3)


# ------------------------------------------------------------------------------------------------ the math header on the host
@pytest.fixture(scope="module")
def hc():
    hdrs = [os.path.join(ROOT, "vinsat_amd", "csrc", f) for f in ("vba_schur_rel_math.h", "vba_math.h")]
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in [SRC] + hdrs):
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", LIB, SRC])
    return ctypes.CDLL(LIB)


def _p(a):
    return a.ctypes.data_as(P)


def _sym(rng, k, eig):
    """Symmetric ``k x k`` with the given eigenvalues and a random frame."""
    Q, _ = np.linalg.qr(rng.normal(size=(k, k)))
    return (Q * np.asarray(eig)) @ Q.T


def test_closed_form_2x2_against_lapack(hc):
    """``rel_wtest2`` against ``sqrt(w r^T solve(I - P, r))``: I - P with eigenvalues down to 1e-6 (the clamp rows reach 4e-6).  The
    adjugate over the determinant loses cond(I - P) ulps in the quadratic form, LAPACK's solve as many: bar 16 eps cond on the
    square root.  Measured: 0.6 eps cond at the worst."""
    rng = np.random.default_rng(21)
    n = 4000
    Pm, r, w, ref, cond = np.empty((n, 3)), rng.normal(0, 3.0, (n, 2)), rng.uniform(0.1, 1.0, n), np.empty(n), np.empty(n)
    for k in range(n):
        lo = 10.0 ** rng.uniform(-6, 0)
        M = _sym(rng, 2, (lo, rng.uniform(lo, 1.0)))
        Pk = np.eye(2) - M
        Pk = 0.5 * (Pk + Pk.T)
        Pm[k] = Pk[0, 0], Pk[0, 1], Pk[1, 1]
        M = np.eye(2) - Pk                          # what the function is given: P rounded, not M
        ref[k] = np.sqrt(w[k] * r[k] @ np.linalg.solve(M, r[k]))
        cond[k] = np.linalg.cond(M)
    out = np.empty(n)
    hc.hc_rel_wtest2(ctypes.c_int64(n), _p(Pm), _p(r), _p(w), _p(out))
    err = np.abs(out - ref) / ref / (EPS * cond)
    print(f"FIGURES rel_wtest2: worst error {err.max():.2f} eps cond(I - P)")
    assert np.all(np.isfinite(out)) and err.max() <= 16.0


def test_closed_form_3x3_against_lapack(hc):
    """``rel_wtest3`` against ``sqrt(scale e^T solve(M, e))``: one eigenvalue of M down to 1e-5 (the fixtures reach 9e-5 in a landmark
    of two rows), the others in [0.1, 1].  Cofactors carry errors of eps |M|^2 against a form of size det / mu_max: bar
    16 eps mu_max^2 / (mu_min mu_mid) on the square root, LAPACK's own error included."""
    rng = np.random.default_rng(22)
    n = 4000
    M6, e, sc, ref, amp = np.empty((n, 6)), rng.normal(0, 0.01, (n, 3)), np.full(n, 400.0), np.empty(n), np.empty(n)
    for k in range(n):
        eig = np.sort([10.0 ** rng.uniform(-5, 0), rng.uniform(0.1, 1.0), rng.uniform(0.1, 1.0)])
        M = _sym(rng, 3, eig)
        M = 0.5 * (M + M.T)
        M6[k] = M[0, 0], M[0, 1], M[0, 2], M[1, 1], M[1, 2], M[2, 2]
        ref[k] = np.sqrt(sc[k] * e[k] @ np.linalg.solve(M, e[k]))
        amp[k] = eig[2] ** 2 / (eig[0] * eig[1])
    out = np.empty(n)
    hc.hc_rel_wtest3(ctypes.c_int64(n), _p(M6), _p(e), _p(sc), _p(out))
    err = np.abs(out - ref) / ref / (EPS * amp)
    print(f"FIGURES rel_wtest3: worst error {err.max():.2f} eps mu_max^2 / (mu_min mu_mid)")
    assert np.all(np.isfinite(out)) and err.max() <= 16.0


def test_closed_forms_degenerate_input(hc):
    def one(f, *args):
        out = np.empty(1)
        f(ctypes.c_int64(1), *[_p(np.asarray(x, dtype=np.float64)) for x in args], _p(out))
        return out[0]

    r = [3.0, -4.0]
    assert one(hc.hc_rel_wtest2, [0.0, 0.0, 0.0], r, [1.0]) == 5.0                  # P = 0: the weighted residual itself
    assert one(hc.hc_rel_wtest2, [0.0, 0.0, 0.0], r, [0.0]) == 0.0
    assert np.isnan(one(hc.hc_rel_wtest2, [1.0, 0.0, 0.5], r, [1.0]))               # det(I - P) = 0
    assert np.isnan(one(hc.hc_rel_wtest2, [1.5, 0.0, 0.5], r, [1.0]))               # det < 0
    assert np.isnan(one(hc.hc_rel_wtest2, [1.5, 0.0, 1.5], r, [1.0]))               # det > 0, form negative
    assert np.isnan(one(hc.hc_rel_wtest2, [0.0, 0.0, 0.0], r, [-1.0]))              # negative weight: negative form
    e = [1.0, 2.0, 2.0]
    assert one(hc.hc_rel_wtest3, [1.0, 0.0, 0.0, 1.0, 0.0, 1.0], e, [4.0]) == 6.0   # identity: sqrt(scale) |e|
    assert one(hc.hc_rel_wtest3, [1.0, 0.0, 0.0, 1.0, 0.0, 1.0], [0.0, 0.0, 0.0], [4.0]) == 0.0
    assert np.isnan(one(hc.hc_rel_wtest3, [1.0, 0.0, 0.0, 1.0, 0.0, 0.0], e, [4.0]))        # singular
    assert np.isnan(one(hc.hc_rel_wtest3, [1.0, 0.0, 0.0, 1.0, 0.0, -1.0], e, [4.0]))       # det < 0
    assert np.isnan(one(hc.hc_rel_wtest3, [-1.0, 0.0, 0.0, -1.0, 0.0, 1.0], [1.0, 1.0, 0.0], [4.0]))    # det > 0, form negative


def test_ctypes_prototypes_and_header_agree():
    import re
    from vinsat_amd import _lib
    sig = _lib.SIGNATURES
    assert sig["vba_schur_reliability"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double] + [_lib.PD] * 7 + [ctypes.POINTER(ctypes.c_int)])
    assert sig["vba_schur_last_reliability_ms"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)])
    with open(os.path.join(ROOT, "include", "vinsat_ba.h")) as f:
        hdr = f.read()
    assert re.search(r"int vba_schur_reliability\(vba_schur_handle h, double lamda, double\* leverage[^;]*double\* wtest[^;]*double\* lm_leverage[^;]*"
                     r"double\* lm_wtest[^;]*double\* lm_stats[^;]*double\* pose_stats[^;]*double\* fit[^;]*int\* info\);", hdr)
    assert re.search(r"int vba_schur_last_reliability_ms\(vba_schur_handle h, float\* ms\);", hdr)
    if os.path.exists(_lib.LIB_PATH):               # the built library exports both (it is loaded without a device)
        lib = ctypes.CDLL(_lib.LIB_PATH)
        assert lib.vba_schur_reliability and lib.vba_schur_last_reliability_ms
