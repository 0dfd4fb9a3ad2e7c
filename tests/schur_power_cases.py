"""CPU reference of ``vba_schur_outlier_power`` / ``vba_schur_outlier_power_dyn`` shared by tests/test_schur_power_host.py and
tests/test_gpu_schur_power.py (plain module, no tests).  Problems, states and ``(case, lamda)`` pairs are those of
tests/schur_rel_cases.py and, for a handle with the dynamics factor, of tests/schur_dyn_rel_cases.py.

Reference (:func:`evaluate`): route 1 takes ``Sigma_ii``, ``Sigma_il``, ``Sigma_ll`` from the dense ``inv(H)``, route 2 is the Schur
route the device takes -- the two routes those modules build (``S^-1 = W^T W`` with ``W = inv(chol(S))``, ``Sigma_il = -(S^-1 E C^-1)``,
``Sigma_ll = C^-1 + C^-1 E^T S^-1 E C^-1``).  The 2x2 and 3x3 eigenproblems are LAPACK's: ``eigvalsh``, and for the generalised one
``eigvalsh`` of ``L^-1 M L^-T`` with ``R = L L^T`` by ``numpy.linalg.cholesky``.  The FLOOR of a family is the disagreement of the two
routes relative to the family's largest entry; the device is held to ``max(100 x floor, 1e-11)`` (:func:`bar`, the project's rule); the
floor never comes from the device.  Rows whose reference ``mu_min(R_k)`` is below ``EIG_MIN`` (``kept`` is False) and rows of weight 0
are compared on nothing that divides by it -- every row family does; landmarks with reference ``q < LM_EIG_MIN`` and landmarks without
rows likewise.  The closed-form rules (weight 0, no rows, ``q <= 0``) are applied before anything is inverted.  References are built
once per process and must be left unchanged by their users.

``fault=`` plants one mistake the device could make (:data:`FAULTS`).
"""
import functools
from types import SimpleNamespace

import numpy as np

import schur_cases as C
import schur_dyn_cases as DC
import schur_dyn_oracle as D
import schur_dyn_rel_cases as DR
import schur_rel_cases as R
from oracle import schur_oracle as S

NCP = 17.075
ROW_FAMILIES = ("mdb", "ext_pos", "ext_att", "ext_lm", "del_pos", "del_lm")
LM_FAMILIES = ("lm_mdb", "lm_ext", "lm_del_pos")
FAMILIES = ROW_FAMILIES + LM_FAMILIES
EIG_MIN, LM_EIG_MIN, MAX_LEFT_OUT = R.EIG_MIN, R.LM_EIG_MIN, R.MAX_LEFT_OUT
POWER_FIT_NAMES = ("n_rows_over_crit", "max_ext_pos", "n_lm_over_crit", "max_lm_del_pos")
FAULTS = ("B_l_from_Sigma_ii", "no_factor_2", "p_min", "pull_summed", "Sigma_il_sign")
# the (case, lamda) pairs held against the reference: every pair of schur_rel_cases.CASES (tests/test_schur_power_host.py asserts
# the floors and the left-out shares of each), and for the dynamics factor 12 / 150 and 29 / 300
CASES = R.CASES
DYN_CASES = tuple(c for c in DR.CASES if c[0] in ("12", "29"))


def _gen_mu_max(M, Rm):
    """Largest root of ``det(M - mu R) = 0`` per row, Cholesky-whitened."""
    Lc = np.linalg.cholesky(Rm)
    Li = np.linalg.inv(Lc)
    N = Li @ M @ Li.transpose(0, 2, 1)
    return np.linalg.eigvalsh(0.5 * (N + N.transpose(0, 2, 1)))[:, -1]


def figures_from_blocks(d, X, r, Jc, Jl, Spp, Spl, Sll, ncp=NCP, fault=None):
    """Every family from the blocks of ``Sigma``: poses ``Spp [>=6n, >=6n]`` (the leading 6 n are read), cross ``Spl [>=6n, 3L]``,
    landmark blocks ``Sll [L,3,3]``.  Rows in the caller's order."""
    pr, lr, w, sig = d["pose_of_row"], d["landmark_of_row"], d["w"], d["sigma"]
    m, L = w.size, X.shape[0]
    a6, a3 = np.arange(6), np.arange(3)
    ri, ci = (6 * pr)[:, None, None] + a6[None, :, None], (6 * pr)[:, None, None] + a6[None, None, :]
    cl = (3 * lr)[:, None, None] + a3[None, None, :]
    Sii, Sil, Sl = Spp[ri, ci], Spl[ri, cl], Sll[lr]
    Sl = 0.5 * (Sl + Sl.transpose(0, 2, 1))
    if fault == "Sigma_il_sign":
        Sil = -Sil
    Sig = np.concatenate([np.concatenate([Sii, Sil], 2), np.concatenate([Sil.transpose(0, 2, 1), Sl], 2)], 1)
    J = np.concatenate([Jc, Jl], 2)                                     # [m, 2, 9]
    P = w[:, None, None] * (J @ Sig @ J.transpose(0, 2, 1))
    P = 0.5 * (P + P.transpose(0, 2, 1))
    Rm = np.eye(2)[None] - P
    B = w[:, None, None] * (Sig @ J.transpose(0, 2, 1))                 # [m, 9, 2]
    if fault == "B_l_from_Sigma_ii":
        B = B.copy()
        B[:, 6:9] = w[:, None, None] * (Sii[:, 0:3, :] @ Jc.transpose(0, 2, 1) + Sl @ Jl.transpose(0, 2, 1))
    o = SimpleNamespace()
    o.mineig = np.linalg.eigvalsh(Rm)[:, 0]
    on = w > 0.0
    ok = on & (o.mineig > 0.0) & (np.linalg.det(Rm) > 0.0)
    for k in ROW_FAMILIES:
        setattr(o, k, np.full(m, np.nan))
    o.mdb[~on] = np.inf
    for k in ROW_FAMILIES[1:]:
        getattr(o, k)[~on] = 0.0
    wk, Rk, Bk, rk = w[ok], Rm[ok], B[ok], r[ok]
    o.mdb[ok] = np.sqrt(ncp / (wk * o.mineig[ok]))
    for key, sl, fac in (("ext_pos", slice(0, 3), 1.0), ("ext_att", slice(3, 6), 1.0 if fault == "no_factor_2" else 2.0), ("ext_lm", slice(6, 9), 1.0)):
        Bs = Bk[:, sl]
        getattr(o, key)[ok] = fac * np.sqrt(ncp / wk * _gen_mu_max(Bs.transpose(0, 2, 1) @ Bs, Rk))
    z = np.linalg.solve(Rk, rk[:, :, None])                             # [., 2, 1]
    o.del_pos[ok] = np.linalg.norm((Bk[:, 0:3] @ z)[:, :, 0], axis=1)
    o.del_lm[ok] = np.linalg.norm((Bk[:, 6:9] @ z)[:, :, 0], axis=1)
    # catalogue priors
    Pl = 0.5 * (Sll + Sll.transpose(0, 2, 1)) / sig ** 2
    eig = np.linalg.eigvalsh(Pl)
    pmax = eig[:, 0] if fault == "p_min" else eig[:, -1]
    o.q = 1.0 - pmax
    seen = np.bincount(lr, minlength=L) > 0
    o.seen = seen
    good = seen & (o.q > 0.0) & np.isfinite(o.q)
    o.lm_mdb, o.lm_ext, o.lm_del_pos = np.full(L, np.nan), np.full(L, np.nan), np.full(L, np.nan)
    o.lm_mdb[~seen], o.lm_ext[~seen], o.lm_del_pos[~seen] = np.inf, 0.0, 0.0
    o.lm_mdb[good] = sig * np.sqrt(ncp / o.q[good])
    o.lm_ext[good] = sig * np.sqrt(ncp) * pmax[good] / np.sqrt(o.q[good])
    # the pull of the prior on the position of every pose that sees the landmark; inverted only where I - P_l is clear of singular
    e = X - d["X0"]
    Ml = np.eye(3)[None] - Pl
    inv_ok = seen & (np.linalg.eigvalsh(Ml)[:, 0] >= LM_EIG_MIN) & (np.linalg.det(Ml) > 0.0)
    zl = np.zeros((L, 3))
    zl[inv_ok] = np.linalg.solve(Ml[inv_ok], e[inv_ok][:, :, None])[:, :, 0] / sig ** 2
    pull = np.linalg.norm((Sil[:, 0:3, :] @ zl[lr][:, :, None])[:, :, 0], axis=1)
    o.pull = np.where(on, pull, 0.0)
    acc = np.zeros(L)
    if fault == "pull_summed":
        acc = np.bincount(lr, weights=o.pull, minlength=L)
    else:
        np.maximum.at(acc, lr, o.pull)
    o.lm_del_pos[inv_ok] = acc[inv_ok]
    return o


def _routes_plain(d, st, X, lam):
    n6 = 6 * st.shape[0]
    B, Cm, E, _, _ = S.normal_equations(st, X, *C.args(d), lam)
    Hinv = np.linalg.inv(np.block([[B, E], [E.T, Cm]]))
    one = (Hinv[:n6, :n6], Hinv[:n6, n6:], R._blocks3(Hinv[n6:, n6:]))
    Cinv = np.linalg.inv(R._blocks3(Cm))
    G = np.einsum("alc,lcd->ald", E.reshape(n6, -1, 3), Cinv).reshape(n6, -1)
    W = np.linalg.inv(np.linalg.cholesky(B - G @ E.T))
    Sinv = W.T @ W
    SG = Sinv @ G
    two = (Sinv, -SG, Cinv + np.einsum("alc,ald->lcd", G.reshape(n6, -1, 3), SG.reshape(n6, -1, 3)))
    return one, two


def _routes_dyn(d, st, X, lam):
    n = st.shape[0]
    n6, n9 = 6 * n, 9 * n
    B9, Cm, E9, _, _ = D.normal_equations(st, X, *DC.args(d), lam, d["time_idx"], d["sigma_dyn"])
    Hinv = np.linalg.inv(np.block([[B9, E9], [E9.T, Cm]]))
    Hinv = 0.5 * (Hinv + Hinv.T)                            # (schur_dyn_rel_cases.evaluate says why)
    one = (Hinv[:n6, :n6], Hinv[:n6, n9:], R._blocks3(Hinv[n9:, n9:]))
    Cinv = np.linalg.inv(R._blocks3(Cm))
    G = np.einsum("alc,lcd->ald", E9.reshape(n9, -1, 3), Cinv).reshape(n9, -1)
    W = np.linalg.inv(np.linalg.cholesky(B9 - G @ E9.T))
    Sinv = W.T @ W
    SG = Sinv @ G
    two = (Sinv[:n6, :n6], -SG[:n6], Cinv + np.einsum("alc,ald->lcd", G.reshape(n9, -1, 3), SG.reshape(n9, -1, 3)))
    return one, two


def rel(a, b, mask):
    a, b = a[mask], b[mask]
    return float(np.abs(a - b).max() / np.abs(b).max())


def evaluate(d, st, X, lam, dyn=False, ncp=NCP, second_route=True, fault=None):
    """Reference at the state ``(st, X)`` of problem ``d`` and damping ``lam``: route 1, and with ``second_route`` the floors."""
    r, Jc, Jl = S.linearise(st, X, d["uv"], d["w"], d["pose_of_row"], d["landmark_of_row"], d["intrinsics"])
    one, two = (_routes_dyn if dyn else _routes_plain)(d, st, X, lam)
    o = figures_from_blocks(d, X, r, Jc, Jl, *one, ncp=ncp, fault=fault)
    o.lam, o.ncp, o.residual = lam, ncp, r
    o.kept = (d["w"] > 0.0) & ~(o.mineig < EIG_MIN)                    # rows compared on the six row families
    o.lm_kept = o.seen & ~(o.q < LM_EIG_MIN)                            # landmarks compared on the three landmark families
    o.left_out = int(((d["w"] > 0.0) & (o.mineig < EIG_MIN)).sum())
    o.lm_left_out = int((o.seen & (o.q < LM_EIG_MIN)).sum())
    if second_route:
        o2 = figures_from_blocks(d, X, r, Jc, Jl, *two, ncp=ncp)
        o.floor = {k: rel(getattr(o2, k), getattr(o, k), o.kept if k in ROW_FAMILIES else o.lm_kept) for k in FAMILIES}
    return o


@functools.lru_cache(maxsize=None)
def reference(name, lam, dyn=False):
    d = DC.case(name) if dyn else R.problem(name)
    return evaluate(d, d["states0"], d["Xs"], lam, dyn)


def bar(r, family):
    return max(100.0 * r.floor[family], 1e-11)


def figures(got, r):
    """Device (or any dict of the nine families, rows in the caller's order) against the reference: error per family relative to the
    largest entry, rows over ``r.kept``, landmarks over ``r.lm_kept``."""
    return {k: rel(np.asarray(got[k]), getattr(r, k), r.kept if k in ROW_FAMILIES else r.lm_kept) for k in FAMILIES}


# ------------------------------------------------------------------------------------------------ linearisation sanity
def without_row(d, row):
    """``d`` with the weight of one row set to 0."""
    p = dict(d)
    w = d["w"].copy()
    w[row] = 0.0
    p["w"] = w
    return p


def with_catalogue_entry(d, l, x):
    """``d`` with the catalogue position of landmark ``l`` set to ``x``."""
    p = dict(d)
    X0 = d["X0"].copy()
    X0[l] = x
    p["X0"] = X0
    return p


def release_prior(d, l, st, X, converge, rounds=14):
    """The fit of ``d`` WITHOUT the prior of landmark ``l``, from ``(st, X)``, with a solver that knows one sigma for every entry: the
    catalogue entry is moved onto the landmark's estimate and the fit re-converged, ``rounds`` times.  At the fixed point
    ``e_l = 0``: the prior pulls nowhere, so the point is stationary for the cost without it.  (The distance shrinks by the prior's
    share ``p_max`` of the landmark per round.)  ``converge(problem, st, X) -> (st, X)``."""
    for _ in range(rounds):
        d = with_catalogue_entry(d, l, X[l])
        st, X = converge(d, st, X)
    return st, X, float(np.linalg.norm(X[l] - d["X0"][l]))


# ``SchurBA.solve`` ends on the decrease of the cost, which along the weakly determined position of a pose comes long before the
# position has settled (12 / 150 with the planted row deleted: 0.14 km of 1.2 km moved when the default tolerance stops it, 0.40 km
# after 100 trials at a tolerance of 1e-16).  The linearisation tests therefore settle a fit by undamped Gauss-Newton steps applied
# whatever they do to the cost: ``step(st, X) -> (dc [n,6], dl [L,3])`` at ``lamda = 0``, the oracle's or the device's, retracted by
# the oracle.  The step falls below 1e-12 within 30 of them on the planted cases.
GN_STEPS = 30


def settle(step, st, X, steps=GN_STEPS):
    for _ in range(steps):
        dc, dl = step(st, X)
        st, X = S.apply_step(st, X, np.asarray(dc).reshape(-1), np.asarray(dl).reshape(-1))
    return st, X


def oracle_step(d):
    def step(st, X):
        B, Cm, E, v, wl = S.normal_equations(st, X, *C.args(d), 0.0)
        dc, dl, _, _ = S.step_schur(B, Cm, E, v, wl)
        return dc, dl
    return step


def oracle_linearisation():
    """The oracle's own linearisation errors on the planted cases of ``schur_rel_cases``, the origin of the margins of
    tests/test_gpu_schur_power.py: ``(del_pos, del_lm, lm_del_pos)`` as ``|moved / predicted - 1|``."""
    d = R.planted_outlier()
    row = d["planted_row"]
    i, l = d["pose_of_row"][row], d["landmark_of_row"][row]
    st, X = settle(oracle_step(d), *R.converge(d))
    ref = evaluate(d, st, X, 0.0, second_route=False)
    st2, X2 = settle(oracle_step(without_row(d, row)), st, X)
    e_pos = abs(np.linalg.norm(st2[i, :3] - st[i, :3]) / ref.del_pos[row] - 1.0)
    e_lm = abs(np.linalg.norm(X2[l] - X[l]) / ref.del_lm[row] - 1.0)
    d = R.displaced_landmark()
    l = d["displaced_lm"]
    st, X = settle(oracle_step(d), *R.converge(d))
    ref = evaluate(d, st, X, 0.0, second_route=False)
    st2, _, _ = release_prior(d, l, st, X, lambda p, s, x: settle(oracle_step(p), s, x, 6))
    poses = d["pose_of_row"][d["landmark_of_row"] == l]
    e_prior = abs(np.linalg.norm(st2[poses, :3] - st[poses, :3], axis=1).max() / ref.lm_del_pos[l] - 1.0)
    return float(e_pos), float(e_lm), float(e_prior)
