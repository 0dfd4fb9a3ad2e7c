"""CPU side of the free-landmark outlier power query (``vba_schur_outlier_power``): the reference of tests/schur_power_cases.py
against itself, the planted faults, and the closed forms of vinsat_amd/csrc/vba_schur_power_math.h compiled for the host against
LAPACK and against the reference.  No GPU.

Floors (disagreement of the reference's two NumPy routes relative to the largest entry of the family) at ``ncp = 17.075``, as
measured; the largest and smallest of the nine families per case, rows / landmarks left out:

  case                          lam    smallest   largest (family)        left out (rows / landmarks)
  12 / 150                      0      1.0e-13    9.8e-13 (ext_att)       0 / 0
  12 / 150                      1e-3   1.0e-13    8.8e-13 (del_pos)       0 / 0
  43 / 450                      1e-3   5.5e-14    7.1e-13 (ext_pos)       0 / 0
  129 / 1300                    1e-3   7.5e-14    1.2e-12 (lm_del_pos)    0 / 0
  wide                          1e-3   5.1e-14    1.4e-12 (lm_del_pos)    0 / 0
  pose_without_rows             1e-3   6.9e-14    5.4e-13 (ext_att)       0 / 0
  more_landmarks_than_rows      0      9.2e-14    1.2e-12 (lm_del_pos)    0 / 37 of 400 (the tracks of one row; 266 without rows)
  more_poses_than_landmarks     1e-3   5.5e-12    6.6e-11 (lm_del_pos)    0 / 0
  zero_weights                  1e-3   3.3e-14    3.6e-13 (lm_del_pos)    0 / 0
  behind_the_camera             1e4    6.6e-16    2.1e-09 (lm_del_pos)    5 of 1474 (the clamped rows) / 0
  dynamics 12 / 150             0      1.2e-11    1.4e-09 (lm_del_pos)    0 / 0
  dynamics 12 / 150             1e-3   1.0e-11    1.0e-09 (lm_del_pos)    0 / 0
  dynamics 29 / 300             0      1.3e-13    1.3e-09 (lm_del_pos)    0 / 2 of 300
  dynamics 29 / 300             1e-3   5.3e-14    1.3e-10 (lm_mdb)        0 / 0

(they move by a few tens of per cent with the BLAS and its thread count).  No case breaks a condition, so none is dropped.  A bar of
the GPU tests is ``max(100 x floor, 1e-11)``.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import schur_power_cases as PW
import schur_rel_cases as R
from conftest import ROOT
from oracle import schur_oracle as S

HC = os.path.join(ROOT, "tests", "hostcheck")
SRC = os.path.join(HC, "hostcheck_schur_power.cpp")
LIB = os.path.join(HC, "libhostcheck_schur_power.so")
P = ctypes.POINTER(ctypes.c_double)
EPS = np.finfo(np.float64).eps
ALL = [(n, l, False) for n, l in PW.CASES] + [(n, l, True) for n, l in PW.DYN_CASES]


@pytest.mark.parametrize("name,lam,dyn", ALL)
def test_floor_of_the_reference(name, lam, dyn):
    r = PW.reference(name, lam, dyn)
    print(f"FIGURES power floor {'dynamics ' if dyn else ''}{name} lam={lam:g} " + " ".join(f"{k}={r.floor[k]:.2e}" for k in PW.FAMILIES) +
          f" left out {r.left_out} of {r.kept.size} rows, {r.lm_left_out} of {r.lm_kept.size} landmarks")
    assert all(np.isfinite(r.floor[k]) and r.floor[k] < 1e-8 for k in PW.FAMILIES)
    assert r.left_out <= PW.MAX_LEFT_OUT * r.kept.size
    assert r.left_out == (5 if name == "behind_the_camera" else 0)
    assert r.lm_left_out == (37 if name == "more_landmarks_than_rows" else 2 if (dyn and name == "29" and lam == 0.0) else 0)
    for k in PW.ROW_FAMILIES:
        assert np.all(np.isfinite(getattr(r, k)[r.kept]))
    for k in PW.LM_FAMILIES:
        assert np.all(np.isfinite(getattr(r, k)[r.lm_kept]))


def test_closed_form_rules_of_the_reference():
    r, d = PW.reference("zero_weights", 1e-3), R.problem("zero_weights")
    off = d["w"] == 0.0
    assert off.sum() > 100 and np.all(np.isposinf(r.mdb[off]))
    for k in PW.ROW_FAMILIES[1:]:
        assert np.array_equal(getattr(r, k)[off], np.zeros(off.sum()))
    r, d = PW.reference("more_landmarks_than_rows", 0.0), R.problem("more_landmarks_than_rows")
    u = d["unobserved"]
    assert u.size > 200 and np.array_equal(np.nonzero(~r.seen)[0], np.sort(u))
    assert np.all(r.q[u] == 0.0)                                    # P_l = I exactly: the rule comes before any inversion
    assert np.all(np.isposinf(r.lm_mdb[u])) and np.array_equal(r.lm_ext[u], np.zeros(u.size)) and np.array_equal(r.lm_del_pos[u], np.zeros(u.size))


def test_figures_have_the_sizes_they_should():
    """Sanity of the definitions on 12 / 150: a detectable bias is at least sqrt(ncp / w) pixels (mu_min <= 1) and the detectable
    catalogue error at least sigma sqrt(ncp); an undetected catalogue error moves the landmark by less than itself times p / (1 - p)."""
    r, d = PW.reference("12", 0.0), R.problem("12")
    assert np.all(r.mdb >= np.sqrt(PW.NCP / d["w"]) * (1 - 1e-12))
    assert np.all(r.lm_mdb >= d["sigma"] * np.sqrt(PW.NCP) * (1 - 1e-12))
    assert np.all(r.lm_ext <= r.lm_mdb * (1.0 - r.q) / r.q * (1 + 1e-9))
    assert np.all(r.ext_pos > 0) and np.all(r.ext_att > 0) and np.all(r.ext_lm > 0)


@pytest.mark.parametrize("fault", PW.FAULTS)
def test_planted_faults_cross_a_bar(fault):
    r, d = PW.reference("12", 0.0), R.problem("12")
    bad = PW.evaluate(d, d["states0"], d["Xs"], 0.0, second_route=False, fault=fault)
    fig = PW.figures({k: getattr(bad, k) for k in PW.FAMILIES}, r)
    over = [k for k in PW.FAMILIES if not fig[k] <= PW.bar(r, k)]
    print(f"FIGURES power fault {fault}: over the bar {over} " + " ".join(f"{k}={fig[k]:.1e}" for k in over))
    assert over


def test_linearisation_errors_of_the_oracle_are_the_origin_of_the_gpu_margins():
    """The deletion figures against the oracle's own re-settled fits: 5.5e-4 (``del_pos``), 2.9e-5 (``del_lm``), 2.0e-3 (``lm_del_pos``).
    The GPU tests hold the device to about three times the first and the last, 2e-3 and 6e-3: here those margins are held to be at
    least twice the oracle's own error."""
    e_pos, e_lm, e_prior = PW.oracle_linearisation()
    print(f"FIGURES power oracle linearisation del_pos {e_pos:.2e} del_lm {e_lm:.2e} lm_del_pos {e_prior:.2e}")
    assert e_pos <= 2e-3 / 2 and e_lm <= 2e-3 / 2 and e_prior <= 6e-3 / 2


# ------------------------------------------------------------------------------------------------ the math header on the host
@pytest.fixture(scope="module")
def hc():
    hdrs = [os.path.join(ROOT, "vinsat_amd", "csrc", f) for f in ("vba_schur_power_math.h", "vba_power_math.h", "vba_math.h")]
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in [SRC] + hdrs):
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", LIB, SRC])
    return ctypes.CDLL(LIB)


def _p(a):
    return a.ctypes.data_as(P)


def _six(M):
    return np.ascontiguousarray(np.stack([M[..., 0, 0], M[..., 0, 1], M[..., 0, 2], M[..., 1, 1], M[..., 1, 2], M[..., 2, 2]], -1))


def _sym3(rng, eig):
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    M = (Q * np.asarray(eig)) @ Q.T
    return 0.5 * (M + M.T)


def _mu_max(hc, Ms):
    out = np.empty(Ms.shape[0])
    hc.hc_sym3_mu_max(ctypes.c_int64(Ms.shape[0]), _p(_six(Ms)), _p(out))
    return out


def test_sym3_mu_max_against_lapack(hc):
    """Jacobi's diagonal carries an absolute error of a few ulps of the norm, as ``eigvalsh`` does: bar 8 eps |M| on the sum of both.
    Random SPD, coincident eigenvalues (a multiple of I, two equal), P within 1e-12 of I, diagonal input."""
    rng = np.random.default_rng(31)
    Ms = [_sym3(rng, 10.0 ** rng.uniform(-6, 0, 3)) for _ in range(3000)]
    Ms += [_sym3(rng, (a, a, a)) for a in 10.0 ** rng.uniform(-6, 0, 200)] + [a * np.eye(3) for a in (1e-5, 0.3, 1.0)]
    Ms += [_sym3(rng, (a, b, b)) for a, b in 10.0 ** rng.uniform(-4, 0, (300, 2))] + [_sym3(rng, (b, b, a)) for a, b in 10.0 ** rng.uniform(-4, 0, (300, 2))]
    Ms += [_sym3(rng, 1.0 - 1e-12 * rng.uniform(0, 1, 3)) for _ in range(500)]
    Ms += [_sym3(rng, (1.0 - 10.0 ** rng.uniform(-12, -1), rng.uniform(0, 0.5), rng.uniform(0, 0.5))) for _ in range(500)]
    Ms += [np.diag(rng.uniform(0, 1, 3)) for _ in range(200)]
    Ms = np.stack(Ms)
    ref = np.linalg.eigvalsh(Ms)[:, -1]
    out = _mu_max(hc, Ms)
    err = np.abs(out - ref) / (EPS * np.abs(ref))
    print(f"FIGURES sym3_mu_max: worst error {err.max():.2f} eps |M| over {Ms.shape[0]} matrices")
    assert np.all(np.isfinite(out)) and err.max() <= 8.0
    d = np.diag([0.25, 0.75, 0.5])
    assert _mu_max(hc, d[None])[0] == 0.75 and _mu_max(hc, (0.3 * np.eye(3))[None])[0] == 0.3    # diagonal input comes back as it is
    assert np.isnan(_mu_max(hc, np.full((1, 3, 3), np.nan))[0])


def _row_inputs(name, lam):
    """What the row pass holds in registers for every row of a case, from the dense inverse: w, P_k, r, T = Sigma_k J_k^T, and the
    landmark side (first three rows of Sigma_il, P_l, e_l)."""
    d = R.problem(name)
    st, X = d["states0"], d["Xs"]
    r, Jc, Jl = S.linearise(st, X, d["uv"], d["w"], d["pose_of_row"], d["landmark_of_row"], d["intrinsics"])
    (Spp, Spl, Sll), _ = PW._routes_plain(d, st, X, lam)
    pr, lr, w = d["pose_of_row"], d["landmark_of_row"], d["w"]
    a6, a3 = np.arange(6), np.arange(3)
    Sii = Spp[(6 * pr)[:, None, None] + a6[None, :, None], (6 * pr)[:, None, None] + a6[None, None, :]]
    Sil = Spl[(6 * pr)[:, None, None] + a6[None, :, None], (3 * lr)[:, None, None] + a3[None, None, :]]
    Sl = 0.5 * (Sll + Sll.transpose(0, 2, 1))
    Sig = np.concatenate([np.concatenate([Sii, Sil], 2), np.concatenate([Sil.transpose(0, 2, 1), Sl[lr]], 2)], 1)
    J = np.concatenate([Jc, Jl], 2)
    T = Sig @ J.transpose(0, 2, 1)
    Pk = w[:, None, None] * (J @ T)
    Pk = 0.5 * (Pk + Pk.transpose(0, 2, 1))
    P3 = np.ascontiguousarray(np.stack([Pk[:, 0, 0], Pk[:, 0, 1], Pk[:, 1, 1]], 1))
    return d, w, P3, np.ascontiguousarray(r), np.ascontiguousarray(T), np.ascontiguousarray(Sil[:, 0:3, :]), Sl / d["sigma"] ** 2, X - d["X0"]


def test_row_and_prior_closed_forms_against_the_reference(hc):
    """The VBA_HD bodies on 12 / 150 at lamda 0, fed from route 1, against the reference's LAPACK eigenproblems on the same route: the
    difference is the closed forms' own (2x2 by square roots, Jacobi, adjugates).  Bar: the GPU tests' bar of the family."""
    ref = PW.reference("12", 0.0)
    d, w, P3, r, T, S3, Pl, e = _row_inputs("12", 0.0)
    m, L, lr = w.size, Pl.shape[0], d["landmark_of_row"]
    rows = np.empty((m, 6))
    hc.hc_pow_row(ctypes.c_int64(m), _p(w), _p(P3), _p(r), _p(T), ctypes.c_double(PW.NCP), _p(rows))
    pri = np.empty((L, 2))
    hc.hc_pow_prior(ctypes.c_int64(L), _p(_six(Pl)), ctypes.c_double(d["sigma"]), ctypes.c_double(PW.NCP), _p(pri))
    pull, det = np.empty(m), np.empty(m)
    hc.hc_pow_pull(ctypes.c_int64(m), _p(np.ascontiguousarray(S3)), _p(_six(Pl[lr])), _p(np.ascontiguousarray(e[lr])), ctypes.c_double(1.0 / d["sigma"] ** 2),
                   _p(pull), _p(det))
    lm_del = np.zeros(L)
    np.maximum.at(lm_del, lr, pull)
    got = dict(zip(PW.ROW_FAMILIES, rows.T), lm_mdb=pri[:, 0], lm_ext=pri[:, 1], lm_del_pos=lm_del)
    fig = PW.figures(got, ref)
    print("FIGURES power closed forms on 12 / 150: " + " ".join(f"{k}={fig[k]:.1e} (bar {PW.bar(ref, k):.1e})" for k in PW.FAMILIES))
    assert np.all(det > 0.0)
    for k in PW.FAMILIES:
        assert fig[k] <= PW.bar(ref, k), k


def test_closed_forms_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """A stand-alone program with its own main (CPU only); any ASan / UBSan finding aborts it with a non-zero code."""
    src = os.path.join(HC, "sanitize_schur_power_main.cpp")
    exe = str(tmp_path / "sanitize_schur_power_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "sanitize_schur_power_main ok" in p.stdout and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


def test_ctypes_prototypes_and_header_agree():
    import re
    from vinsat_amd import _lib
    sig = _lib.SIGNATURES
    want = (ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_double] * 3 + [_lib.PD] * 11 + [ctypes.POINTER(ctypes.c_int)])
    assert sig["vba_schur_outlier_power"] == want and sig["vba_schur_outlier_power_dyn"] == want
    for name in ("vba_schur_last_outlier_power_ms", "vba_schur_last_outlier_power_dyn_ms"):
        assert sig[name] == (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)])
    with open(os.path.join(ROOT, "include", "vinsat_ba.h")) as f:
        hdr = f.read()
    args = "".join(rf"[^;]*double\* {a}" for a in PW.FAMILIES + ("pose_fit", "fit"))
    for name in ("vba_schur_outlier_power", "vba_schur_outlier_power_dyn"):
        assert re.search(rf"int {name}\(vba_schur_handle h, double lamda, double ncp, double crit{args}[^;]*int\* info\);", hdr)
    assert "p^2 / (1 - p) rises on [0, 1)" in hdr and "velocity-pose tiles" in hdr
    if os.path.exists(_lib.LIB_PATH):
        lib = ctypes.CDLL(_lib.LIB_PATH)
        assert lib.vba_schur_outlier_power and lib.vba_schur_outlier_power_dyn
