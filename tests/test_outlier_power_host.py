"""The outlier power query on the CPU: the closed forms of vinsat_amd/csrc/vba_power_math.h, compiled for the host, against LAPACK
(tests/power_oracle.py), and the identities the NumPy restatement must satisfy on the golden windows -- among them the absence of
degenerate rows, which lets tests/test_gpu_outlier_power.py compare every row.

Bars of the closed forms (measured values in the docstrings and in DESIGN.md section 14).  mu_min of a symmetric 2x2 is
conditioned by the LARGER eigenvalue (its absolute error is rounding of numbers of that size): bar 4 ulp of mu_max(R).  The larger
root of the pair (M, R) goes through the Cholesky factor of R, so its relative error grows with cond(R) = mu_max(R) / mu_min(R):
bar 8 ulp x cond(R) of the root itself -- LAPACK's own reduction (dsygv) has the same conditioning."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import power_oracle as PO
from conftest import ROOT, golden_inputs, load_golden
from oracle import ba_oracle as O

SRC = os.path.join(ROOT, "tests", "hostcheck", "hostcheck_power.cpp")
LIB = os.path.join(ROOT, "tests", "hostcheck", "libhostcheck_power.so")
P = ctypes.POINTER(ctypes.c_double)
EPS = np.finfo(np.float64).eps
MU_MIN_ULPS, PAIR_ULPS = 4.0, 8.0


def _p(a):
    return a.ctypes.data_as(P)


@pytest.fixture(scope="module")
def hc():
    hdrs = [os.path.join(ROOT, "vinsat_amd", "csrc", f) for f in ("vba_power_math.h", "vba_math.h")]
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in [SRC] + hdrs):
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", LIB, SRC])
    return ctypes.CDLL(LIB)


def _cases():
    """(M [c,3], R [c,3], kind [c]): random pairs and the named edge cases.  R positive definite, M positive semi-definite."""
    rng = np.random.default_rng(14)
    M, Rm, kind = [], [], []

    def spd(lo, hi):
        th = rng.uniform(0, np.pi)
        c, s = np.cos(th), np.sin(th)
        return c * c * lo + s * s * hi, c * s * (lo - hi), s * s * lo + c * c * hi

    def psd():
        B = rng.normal(size=(3, 2)) * 10.0 ** rng.uniform(-3, 1)
        G = B.T @ B
        return G[0, 0], G[0, 1], G[1, 1]

    for _ in range(4000):                       # what the row pass sees: eigenvalues of R in (0, 1]
        lo = 1.0 - rng.uniform(0, 1) ** 3
        M.append(psd()); Rm.append(spd(lo, rng.uniform(lo, 1.0))); kind.append("random")
    for _ in range(200):                        # b = 0, a = d: coincident eigenvalues
        a = rng.uniform(0.1, 1.0)
        M.append(psd()); Rm.append((a, 0.0, a)); kind.append("coincident")
    for _ in range(200):                        # ... and of the pair: M a multiple of R
        r = spd(rng.uniform(0.2, 0.5), rng.uniform(0.5, 1.0))
        f = rng.uniform(0.1, 10)
        M.append(tuple(f * x for x in r)); Rm.append(r); kind.append("M = f R")
    for _ in range(200):                        # R within 1e-12 of singular
        M.append(psd()); Rm.append(spd(rng.uniform(1e-13, 1e-12), rng.uniform(0.5, 1.0))); kind.append("near singular")
    for _ in range(200):                        # M of rank 1
        v = rng.normal(size=2)
        M.append((v[0] * v[0], v[0] * v[1], v[1] * v[1])); Rm.append(spd(rng.uniform(0.2, 0.9), 1.0)); kind.append("rank 1")
    for _ in range(50):                         # M = 0
        M.append((0.0, 0.0, 0.0)); Rm.append(spd(rng.uniform(0.2, 0.9), 1.0)); kind.append("zero")
    return np.array(M), np.array(Rm), np.array(kind)


def test_closed_forms_against_lapack(hc):
    """Measured here (x86-64, g++ -O2, 4850 cases): mu_min at most 1.71 ulp of mu_max(R) (random), 0 (coincident); the pair's
    larger root at most 2.48 ulp x cond(R) of itself (random 2.48, coincident 1.61, M = f R 1.06, near singular 0.36, rank 1
    1.26), exactly 0 for M = 0; R^-1 r within 1.92 ulp x cond(R).  Bars: 4, 8 and 8 -- a few ulp of each form's conditioning."""
    M, Rm, kind = _cases()
    c = M.shape[0]
    lo = np.zeros(c)
    hc.hc_sym2_mu_min(ctypes.c_int64(c), _p(np.ascontiguousarray(Rm)), _p(lo))
    ev = np.linalg.eigvalsh(np.stack([np.stack([Rm[:, 0], Rm[:, 1]], -1), np.stack([Rm[:, 1], Rm[:, 2]], -1)], -2))
    assert np.array_equal(PO.mu_min_sym2(Rm[:, 0], Rm[:, 1], Rm[:, 2]), ev[:, 0])
    e_min = np.abs(lo - ev[:, 0]) / ev[:, 1] / EPS
    hi = np.zeros(c)
    hc.hc_pair_mu_max(ctypes.c_int64(c), _p(np.ascontiguousarray(M)), _p(np.ascontiguousarray(Rm)), _p(hi))
    ref = np.array([PO.mu_max_pair(np.array([[m[0], m[1]], [m[1], m[2]]]), np.array([[r[0], r[1]], [r[1], r[2]]]))
                    for m, r in zip(M, Rm)])
    assert np.isfinite(ref).all() and np.isfinite(hi).all() and (hi >= 0).all()
    cond = ev[:, 1] / ev[:, 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        e_pair = np.where(ref > 0, np.abs(hi - ref) / ref / (EPS * cond), np.abs(hi - ref))
    rng = np.random.default_rng(3)
    r = rng.normal(size=(c, 2))
    z = np.zeros((c, 2))
    hc.hc_sym2_solve(ctypes.c_int64(c), _p(np.ascontiguousarray(Rm)), _p(np.ascontiguousarray(r)), _p(z))
    zr = np.stack([np.linalg.solve(np.array([[q[0], q[1]], [q[1], q[2]]]), x) for q, x in zip(Rm, r)])
    e_solve = np.abs(z - zr).max(1) / np.abs(zr).max(1) / (EPS * cond)
    for kd in dict.fromkeys(kind):
        s = kind == kd
        print(f"{kd}: mu_min {e_min[s].max():.2f} ulp of mu_max(R); pair mu_max {e_pair[s].max():.2f} ulp x cond(R); "
              f"solve {e_solve[s].max():.2f} ulp x cond(R)")
    assert e_min.max() <= MU_MIN_ULPS
    assert e_pair.max() <= PAIR_ULPS
    assert e_solve.max() <= PAIR_ULPS
    assert (hi[kind == "zero"] == 0.0).all()
    # coincident eigenvalues: the value itself, no tie rule
    s = kind == "coincident"
    assert np.array_equal(lo[s], Rm[s, 0])


def test_an_indefinite_R_gives_no_finite_root(hc):
    M = np.array([[1.0, 0.2, 3.0]])
    Rm = np.array([[1.0, 2.0, 1.0]])
    out = np.zeros(1)
    hc.hc_pair_mu_max(ctypes.c_int64(1), _p(M), _p(Rm), _p(out))
    assert not np.isfinite(out[0])
    hc.hc_sym2_mu_min(ctypes.c_int64(1), _p(Rm), _p(out))
    assert out[0] == -1.0


def test_closed_forms_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """A stand-alone program with its own main (CPU only); any ASan / UBSan finding aborts it with a non-zero code."""
    src = os.path.join(ROOT, "tests", "hostcheck", "sanitize_power_main.cpp")
    exe = str(tmp_path / "sanitize_power_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "sanitize_power_main ok" in p.stdout and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


# ------------------------------------------------------------------------------------------------ the oracle on the fixtures
def _final(name):
    g = load_golden(name)
    inp = golden_inputs(g)
    st, lam = g["states_out_19"][0], float(g["lamda_out"][-1])
    d = {}
    O.ba_iteration(19, st, inp["cumrot"], inp["uv"], inp["xyz"], inp["ii"], inp["time_idx"], inp["K"], inp["conf"], lam,
                   initialize=False, debug=d)
    return d, inp["ii"], lam


def _gap():
    from vinsat_amd import od_pipe, synth
    g = load_golden("gap")
    win = od_pipe.prepare_window(*synth.make_two_pass_sequence())
    st, lam = g["states_out_24"][0], float(g["lamda_in"][25])
    d = {}
    O.ba_iteration(12, st, win.cumrot_last, win.landmarks_uv, win.landmarks_xyz, win.ii, win.time_idx, win.intrinsics,
                   win.confidences, lam, initialize=False, debug=d)
    return d, win.ii, lam


def _reg_c1():
    """The BA_reg window of tests/test_gpu_outlier_power.py: C1 with a random prior, one BA_reg call from perturbed ground-truth states."""
    from vinsat_amd import od_pipe, synth
    win = od_pipe.prepare_window(*synth.make_sequence("C1"))
    n = win.states_gt.shape[0]
    rng = np.random.default_rng(6)
    sp = win.states_gt.copy()
    sp[:, :3] += rng.normal(0, 0.5, (n, 3))
    Hs = np.stack([np.eye(6) * s for s in rng.uniform(0.5, 3.0, n)])
    st = win.states_gt.copy()
    st[:, :3] += rng.normal(0, 2.0, (n, 3))
    args = (win.cumrot_last, win.landmarks_uv, win.landmarks_xyz, win.ii, win.time_idx, win.intrinsics, win.confidences)
    out, lam = O.ba_iteration(12, st, *args, 1e-4, initialize=False, prior=(sp, Hs))[:2]
    d = {}
    O.ba_iteration(12, out, *args, lam, initialize=False, debug=d, prior=(sp, Hs))
    return d, win.ii, lam


def test_oracle_identities_on_c1():
    """Pose leverage sums = tr(S_i H_i); Omega = sum w |r|^2 row by row; rho > 0; s0sq = Omega / rho; the maxima and counts are
    those of the rows; doubling ncp scales mdb and ext_* by sqrt(2) and leaves del_pos."""
    d, ii, lam = _final("c1")
    ref = PO.power(d, ii, crit=2.0)
    tr = np.einsum("iab,iba->i", ref["S"], d["H"])
    err = np.abs(ref["pose_fit"][:, 1] - tr).max() / np.abs(tr).max()
    print(f"c1: pose leverage sums against tr(S H): {err:.2e}")
    assert err < 1e-10
    omega = sum(float(w) * float(r @ r) for w, r in zip(d["w"], d["r_obs"]))
    assert abs(ref["fit"][0] - omega) <= 1e-13 * omega
    assert abs(ref["pose_fit"][:, 0].sum() - omega) <= 1e-13 * omega
    assert ref["fit"][1] == ii.size and ref["fit"][3] > 0 and ref["fit"][3] == 2 * ii.size - ref["fit"][2]
    assert ref["fit"][4] == ref["fit"][0] / ref["fit"][3]
    assert ref["fit"][5] == ref["wtest"].max() and ref["fit"][7] == ref["ext_pos"].max()
    assert ref["fit"][6] == np.count_nonzero(ref["wtest"] > 2.0) == ref["pose_fit"][:, 3].sum() > 0
    two = PO.power(d, ii, ncp=2 * PO.NCP)
    for k in ("mdb", "ext_pos", "ext_att"):
        assert np.allclose(two[k], np.sqrt(2.0) * ref[k], rtol=1e-14, atol=0)
    assert np.array_equal(two["del_pos"], ref["del_pos"])
    # mdb is at least the bias a row of full redundancy would let through
    assert (ref["mdb"] >= np.sqrt(PO.NCP / d["w"]) * (1 - 1e-12)).all()


@pytest.mark.parametrize("name", ["c1", "c2", "gap", "reg_c1"])
def test_no_row_of_non_zero_weight_has_a_degenerate_R(name):
    """The condition that lets the GPU test compare every row without exclusions: det R_k > 0 and mu_min(R_k) > 0 for every row
    of non-zero weight, undamped and damped, and every output finite.  Holds on all four windows (smallest mu_min printed)."""
    d, ii, lam = dict(c1=lambda: _final("c1"), c2=lambda: _final("c2"), gap=_gap, reg_c1=_reg_c1)[name]()
    for lam32 in (0.0, float(np.float32(lam))):
        ref = PO.power(d, ii, lam32)
        live = d["w"] > 0
        print(f"{name} lam32={lam32:g}: min det R {ref['detR'][live].min():.4f}, min mu_min {ref['mu_min'][live].min():.4f}; "
              f"mdb {ref['mdb'].min():.3g} .. {ref['mdb'].max():.3g} px, ext_pos max {ref['ext_pos'].max():.3g} km, "
              f"del_pos max {ref['del_pos'].max():.3g} km, s0sq {ref['fit'][4]:.4g}, dof {ref['fit'][3]:.1f}")
        assert (ref["detR"][live] > 0).all() and (ref["mu_min"][live] > 0).all()
        assert all(np.isfinite(ref[k]).all() for k in ("mdb", "ext_pos", "ext_att", "del_pos"))
        assert ref["fit"][3] > 0 and np.isfinite(ref["fit"]).all()


@pytest.mark.parametrize("name", ["c1", "c2"])
def test_reference_spread_lu_against_cholesky(name):
    """What the 1e-8 bar of the GPU tests rests on: every quantity from the LU inverse against the Cholesky inverse of the same
    system, normalised by the window's largest value.  The bar must hold three times the spread."""
    d, ii, lam = _final(name)
    for lam32 in (0.0, float(np.float32(lam))):
        a, b = PO.power(d, ii, lam32, method="inv"), PO.power(d, ii, lam32, method="chol")
        sp = {k: PO.rel_err_finite(a[k], b[k]) for k in ("mdb", "ext_pos", "ext_att", "del_pos", "pose_fit", "fit")}
        print(f"{name} lam32={lam32:g}: LU vs Cholesky spread: " + ", ".join(f"{k} {v:.2e}" for k, v in sp.items()))
        assert all(3.0 * v < 1e-8 for v in sp.values())


def test_degenerate_rows_are_flagged_in_the_value():
    d, ii, lam = _final("c1")
    d = dict(d)
    w = d["w"].copy()
    w[3] = 0.0
    w[5] *= 1e3         # (not a weight the library produces: P_k beyond the unit ball)
    d["w"] = w
    ref = PO.power(d, ii)
    assert np.isposinf(ref["mdb"][3]) and ref["ext_pos"][3] == ref["ext_att"][3] == ref["del_pos"][3] == 0.0
    assert all(np.isnan(ref[k][5]) for k in ("mdb", "ext_pos", "ext_att", "del_pos"))
    assert ref["fit"][1] == ii.size - 1
