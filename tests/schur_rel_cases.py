"""CPU reference of ``vba_schur_reliability`` shared by tests/test_schur_rel_host.py and tests/test_gpu_schur_rel.py (plain module,
no tests).  Problems are those of tests/schur_cov_cases.py in two variants built here:

* PERTURBED LANDMARKS (every case): the landmark part of the state is the case's ``Xs`` plus a seeded offset of 3 m (1 sigma per
  axis; the catalogue sigma is 50 m).  Several fixtures start at ``X = X0``, where ``lm_wtest`` is identically 0.
* ``zero_weights``: case "12" with every seventh weight set to 0.

Reference (:func:`evaluate`), from ``oracle.schur_oracle.normal_equations`` and ``linearise``: route 1 takes ``P_k`` and ``P_l`` from
the sub-blocks of the dense ``inv(H)``; route 2 is the Schur route the device takes (``S^-1 = W^T W`` with ``W = inv(chol(S))``,
``Sigma_il = -(S^-1 E C^-1)``, ``Sigma_ll = C^-1 + C^-1 E^T S^-1 E C^-1``).  The 2x2 and 3x3 inverses are LAPACK's in both.  The
FLOOR of a family (leverage, wtest, lm_leverage, lm_wtest) is the disagreement of the two routes relative to the largest entry of
the family; the device is held to ``max(100 x floor, 1e-11)`` (:func:`bar`, the rule of ``schur_cov_cases.bar``); the floor never
comes from the device.  Rows whose ``I - P_k`` has a smallest eigenvalue below ``EIG_MIN`` IN THE REFERENCE (``r.kept`` is False)
are held on leverage only: their w-test divides by that eigenvalue.  References are built once per process and must be left
unchanged by their users.
"""
import functools
from types import SimpleNamespace

import numpy as np

import schur_cases as C
import schur_cov_cases as V
from oracle import schur_oracle as S

FAMILIES = ("leverage", "wtest", "lm_leverage", "lm_wtest")
FIT_NAMES = ("omega", "m_eff", "t_rows", "t_prior", "rho", "s0sq", "max_wtest", "max_lm_wtest")
EIG_MIN = 1e-3                  # rows below it (reference's eigenvalue) are left out of the w-test comparison
MAX_LEFT_OUT = 0.01             # ... at most this share of a case's rows
# Landmarks: at lamda = 0 the depth of a landmark seen from ONE pose is held by its prior alone, so its I - P_l is EXACTLY singular
# and the computed smallest eigenvalue is rounding of either sign (-4e-16 .. 4e-16 in more_landmarks_than_rows, 37 such landmarks;
# the next smallest eigenvalue there is 9e-5 and stays in): lm_wtest is 0 / 0, defined by neither route.  Those landmarks alone
# (reference's eigenvalue below LM_EIG_MIN, far from both groups) are held on lm_leverage only.
LM_EIG_MIN = 1e-9
OFFSET_KM = 0.003
# (case, lamda) pairs the GPU tests hold against the reference
CASES = (("12", 0.0), ("12", 1e-3), ("43", 1e-3), ("129", 1e-3), ("wide", 1e-3), ("pose_without_rows", 1e-3),
         ("more_landmarks_than_rows", 0.0), ("more_poses_than_landmarks", 1e-3), ("zero_weights", 1e-3), ("behind_the_camera", 1e4))
# the planted faults: 40 px on one row of "12"; one catalogue entry of "12" moved by 10 sigma
PLANT_SEED, PLANT_PX, DISPLACE_SIGMAS = 5, 40.0, 10.0


@functools.lru_cache(maxsize=None)
def problem(name):
    """The case as a dict of tests/schur_cases.py, ``Xs`` perturbed (module docstring); the arrays of the base case are shared."""
    d = dict(V.case("12" if name == "zero_weights" else name))
    if name == "zero_weights":
        w = d["w"].copy()
        w[::7] = 0.0
        d["w"] = w
    rng = np.random.default_rng(2024)
    d["Xs"] = d["Xs"] + rng.normal(0.0, OFFSET_KM, d["Xs"].shape)
    return d


def _blocks3(M):
    L = M.shape[0] // 3
    return np.stack([M[3 * l:3 * l + 3, 3 * l:3 * l + 3] for l in range(L)])


def _families(d, X, r, Jc, Jl, Spp, Spl, Sll):
    """The four families and what goes with them from the blocks of ``Sigma``: poses ``Spp [6n,6n]``, cross ``Spl [6n,3L]``,
    landmark blocks ``Sll [L,3,3]``."""
    pr, lr, w, sig = d["pose_of_row"], d["landmark_of_row"], d["w"], d["sigma"]
    L = X.shape[0]
    a6, a3 = np.arange(6), np.arange(3)
    ri, ci = (6 * pr)[:, None, None] + a6[None, :, None], (6 * pr)[:, None, None] + a6[None, None, :]
    cl = (3 * lr)[:, None, None] + a3[None, None, :]
    Sii, Sil, Sl = Spp[ri, ci], Spl[ri, cl], Sll[lr]
    Sig = np.concatenate([np.concatenate([Sii, Sil], 2), np.concatenate([Sil.transpose(0, 2, 1), Sl], 2)], 1)
    J = np.concatenate([Jc, Jl], 2)                                     # [m, 2, 9]
    P = w[:, None, None] * (J @ Sig @ J.transpose(0, 2, 1))
    P = 0.5 * (P + P.transpose(0, 2, 1))
    o = SimpleNamespace()
    o.leverage = np.trace(P, axis1=1, axis2=2)
    M = np.eye(2)[None] - P
    o.mineig = np.linalg.eigvalsh(M)[:, 0]
    with np.errstate(all="ignore"):
        t2 = w * np.einsum("ki,kij,kj->k", r, np.linalg.inv(M), r)
        o.wtest = np.where((np.linalg.det(M) > 0.0) & (t2 >= 0.0), np.sqrt(t2), np.nan)
    o.wtest[w == 0.0] = 0.0
    o.leverage[w == 0.0] = 0.0
    Pl = Sll / sig ** 2
    o.lm_leverage = np.trace(Pl, axis1=1, axis2=2)
    e = X - d["X0"]
    seen = np.bincount(lr, minlength=L) > 0
    o.lm_wtest = np.zeros(L)                                            # a landmark without rows is tested by nothing
    Ml = np.eye(3)[None] - Pl[seen]
    o.lm_mineig = np.ones(L)                                            # (1 for a landmark without rows: nothing to invert)
    o.lm_mineig[seen] = np.linalg.eigvalsh(0.5 * (Ml + Ml.transpose(0, 2, 1)))[:, 0]
    with np.errstate(all="ignore"):
        t2 = np.einsum("ki,kij,kj->k", e[seen], np.linalg.inv(Ml), e[seen]) / sig ** 2
        o.lm_wtest[seen] = np.where((np.linalg.det(Ml) > 0.0) & (t2 >= 0.0), np.sqrt(t2), np.nan)
    return o


def stats_of(leverage, wtest, w, index, size):
    """``[size, 3]``: sum of leverage, largest finite wtest (0 if none), rows with ``w > 0`` -- per value of ``index``."""
    out = np.zeros((size, 3))
    out[:, 0] = np.bincount(index, weights=leverage, minlength=size)
    np.maximum.at(out[:, 1], index, np.where(np.isfinite(wtest), wtest, 0.0))
    out[:, 2] = np.bincount(index, weights=(w > 0.0).astype(float), minlength=size)
    return out


def fit_of(d, X, r, o):
    w, L = d["w"], X.shape[0]
    omega = float((w[:, None] * r * r).sum() + ((X - d["X0"]) ** 2).sum() / d["sigma"] ** 2)
    m_eff, t_rows, t_prior = float((w > 0).sum()), float(o.leverage.sum()), float(o.lm_leverage.sum())
    rho = 2.0 * m_eff + 3.0 * L - t_rows - t_prior
    fin = lambda a: float(np.max(a[np.isfinite(a)], initial=0.0))
    return dict(zip(FIT_NAMES, (omega, m_eff, t_rows, t_prior, rho, omega / rho if rho > 0 else float("nan"), fin(o.wtest), fin(o.lm_wtest))))


def rel(a, b, mask=None):
    if mask is not None:
        a, b = a[mask], b[mask]
    return float(np.abs(a - b).max() / np.abs(b).max())


def evaluate(d, st, X, lam, second_route=True):
    """Reference at the state ``(st, X)`` of problem ``d`` and damping ``lam``: route 1, and with ``second_route`` the floors."""
    n6, L = 6 * st.shape[0], X.shape[0]
    B, Cm, E, _, _ = S.normal_equations(st, X, *C.args(d), lam)
    r, Jc, Jl = S.linearise(st, X, d["uv"], d["w"], d["pose_of_row"], d["landmark_of_row"], d["intrinsics"])
    Hinv = np.linalg.inv(np.block([[B, E], [E.T, Cm]]))
    o = _families(d, X, r, Jc, Jl, Hinv[:n6, :n6], Hinv[:n6, n6:], _blocks3(Hinv[n6:, n6:]))
    o.lam, o.residual, o.trace_Hinv, o.unknowns = lam, r, float(np.trace(Hinv)), n6 + 3 * L
    o.kept = ~(o.mineig < EIG_MIN)
    o.lm_kept = ~(o.lm_mineig < LM_EIG_MIN)
    o.lm_stats = stats_of(o.leverage, o.wtest, d["w"], d["landmark_of_row"], L)
    o.pose_stats = stats_of(o.leverage, o.wtest, d["w"], d["pose_of_row"], st.shape[0])
    o.fit = fit_of(d, X, r, o)
    if second_route:
        Cinv = np.linalg.inv(_blocks3(Cm))
        G = np.einsum("alc,lcd->ald", E.reshape(n6, -1, 3), Cinv).reshape(n6, -1)                  # E C^-1
        W = np.linalg.inv(np.linalg.cholesky(B - G @ E.T))
        Sinv = W.T @ W
        SG = Sinv @ G
        o2 = _families(d, X, r, Jc, Jl, Sinv, -SG, Cinv + np.einsum("alc,ald->lcd", G.reshape(n6, -1, 3), SG.reshape(n6, -1, 3)))
        o.floor = dict(leverage=rel(o2.leverage, o.leverage), wtest=rel(o2.wtest, o.wtest, o.kept), lm_leverage=rel(o2.lm_leverage, o.lm_leverage),
                       lm_wtest=rel(o2.lm_wtest, o.lm_wtest, o.lm_kept))
    return o


@functools.lru_cache(maxsize=None)
def reference(name, lam):
    d = problem(name)
    return evaluate(d, d["states0"], d["Xs"], lam)


def bar(r, family):
    return max(100.0 * r.floor[family], 1e-11)


def figures(got, r):
    """Device (or any dict of the four families, caller's row order) against the reference: error per family, wtest over ``r.kept``,
    lm_wtest over ``r.lm_kept``."""
    mask = dict(wtest=r.kept, lm_wtest=r.lm_kept)
    return {k: rel(np.asarray(got[k]), getattr(r, k), mask.get(k)) for k in FAMILIES}


# ------------------------------------------------------------------------------------------------ planted faults
@functools.lru_cache(maxsize=None)
def planted_outlier():
    """Case "12" with ``PLANT_PX`` pixels added to both coordinates of one row (seeded choice among the rows of tracks of 4 and more)."""
    d = dict(V.case("12"))
    rng = np.random.default_rng(PLANT_SEED)
    track = np.bincount(d["landmark_of_row"])[d["landmark_of_row"]]
    row = int(rng.choice(np.nonzero(track >= 4)[0]))
    uv = d["uv"].copy()
    uv[row] += PLANT_PX
    d["uv"], d["planted_row"] = uv, row
    return d


@functools.lru_cache(maxsize=None)
def displaced_landmark():
    """Case "12" with the catalogue entry of one landmark (seeded choice among tracks of 4 and more) moved by ``DISPLACE_SIGMAS`` sigma
    along each axis; the state starts at the displaced catalogue."""
    d = dict(V.case("12"))
    rng = np.random.default_rng(PLANT_SEED + 1)
    l = int(rng.choice(np.nonzero(np.bincount(d["landmark_of_row"], minlength=d["X0"].shape[0]) >= 4)[0]))
    X0 = d["X0"].copy()
    X0[l] += DISPLACE_SIGMAS * d["sigma"] / np.sqrt(3.0) * np.array([1.0, -1.0, 1.0])
    d["X0"], d["Xs"], d["displaced_lm"] = X0, X0, l
    return d


def converge(d, lamda0=1e-4, max_iters=20, tol=1e-10):
    """``SchurBA.solve`` by the oracle: the converged ``(states, X)``."""
    st, X, lam = d["states0"], d["Xs"], lamda0
    for _ in range(max_iters):
        c0, c1, ok, st, X, _, _ = S.lm_trial(st, X, *C.args(d), lam)
        if ok:
            lam = max(lam * 0.1, 1e-9)
            if c0 - c1 <= tol * max(c0, 1e-300):
                break
        else:
            lam *= 10.0
            if lam > 1e8:
                break
    return st, X


@functools.lru_cache(maxsize=None)
def planted_reference(kind):
    d = planted_outlier() if kind == "row" else displaced_landmark()
    st, X = converge(d)
    return evaluate(d, st, X, 0.0, second_route=False)
