"""CPU reference of ``vba_schur_reliability_att`` / ``vba_schur_snoop_att`` / ``vba_schur_outlier_power_att``
(``SchurBA.attitude_reliability``, ``attitude_snoop``, ``attitude_outlier_power``) shared by tests/test_schur_att_rel_host.py and
tests/test_gpu_schur_att_rel.py (plain module, no tests).  Problems: ``schur_att_cases.NAMES`` (12 / 150, its sign variant ``12s``,
29 / 300, 43 / 450 with a pose without rows, 86 / 900) at ``lamda = 0`` and ``1e-3``, both factors at ``schur_att_cases``' weights;
the landmarks start at the case's ``Xs``.

Reference (:func:`evaluate`): ``schur_dyn_rel_cases.evaluate`` with ``schur_att_oracle.normal_equations`` in the place of the dynamics
oracle's -- route 1 takes every block from the symmetric part of the dense ``inv([[B9, E9], [E9^T, C]])``, route 2 is the Schur route
the device takes -- plus the attitude-edge family: edge ``i`` as a 3-row observation of weight ``sigma_att`` with the oracle's own
``J = [J_own | J_next]`` and ``a`` (``schur_att_oracle.edge_terms``), ``P_a = sigma_att J Sigma6 J^T`` over the attitude unknowns of
poses ``i`` and ``i + 1``, ``att_leverage = tr P_a``, ``att_wtest = sqrt(sigma_att a^T (I - P_a)^-1 a)`` by LAPACK.  The FLOOR of a
family (the five of ``schur_dyn_rel_cases`` plus ``att_leverage`` and ``att_wtest``) is the disagreement of the two routes relative to
the family's largest entry; the device is held to ``max(100 x floor, 1e-11)`` (:func:`bar`); the floor never comes from the device.
NO attitude edge is left out of either attitude family (tests/test_schur_att_rel_host.py asserts the conditions).  References are
built once per process and must be left unchanged.

:func:`edge_restated` is the NumPy restatement of the device's attitude edge pass (``Sigma6`` gathered from the attitude components
of the 9x9 state and edge blocks), with the mistakes it could make (``EDGE_FAULTS``).

Planted faults: the row and the catalogue entry of ``schur_dyn_rel_cases`` on 29 / 300 with both factors, and a GYRO fault -- the gap
rotation ``cumrot[GYRO_EDGE]`` composed with a rotation of ``GYRO_ANGLE`` rad about ``GYRO_AXIS`` (:func:`gyro_fault`).
"""
import functools
from types import SimpleNamespace

import numpy as np

import schur_att_cases as AC
import schur_att_oracle as A
import schur_dyn_oracle as D
import schur_dyn_rel_cases as Q
import schur_power_cases as PW
import schur_rel_cases as R
from oracle import ba_oracle as O
from oracle import schur_oracle as S

NAMES, LAMS = AC.NAMES, (0.0, 1e-3)
CASES = tuple((name, lam) for name in NAMES for lam in LAMS)
ATT_FAMILIES = ("att_leverage", "att_wtest")
FAMILIES = Q.FAMILIES + ATT_FAMILIES
FIT_NAMES = Q.FIT_NAMES + ("t_att", "omega_att", "max_att_wtest")
EIG_MIN, LM_EIG_MIN, MAX_LM_LEFT_OUT, MAX_LEFT_OUT = Q.EIG_MIN, Q.LM_EIG_MIN, Q.MAX_LM_LEFT_OUT, R.MAX_LEFT_OUT
ATT_EIG_MIN = 0.49              # the smallest eigenvalue of I - P_a any case may show (the two edges at a pose without rows: 0.4999)
EDGE_FAULTS = ("J_swapped", "edge_transposed", "position_components", "no_sigma", "att_not_in_rho")
ATT = np.array([3, 4, 5])       # dtheta in the 9-vector [dp, dtheta, dv]
POWER_CASES = tuple(c for c in CASES if c[0] in ("12", "29"))
PLANT_CASE, PLANT_MARGIN = Q.PLANT_CASE, Q.PLANT_MARGIN
# the gyro fault: edge 13 -> 14 of 29 / 300, 0.03 rad (1.7 degrees) about a fixed axis
GYRO_EDGE, GYRO_ANGLE, GYRO_AXIS = 13, 0.03, np.array([2.0, -1.0, 2.0]) / 3.0

case, rel, stats_of = AC.case, Q.rel, Q.stats_of


def _att_family(st, cumrot, sa, Sig9):
    """Attitude-edge leverages, tests and cost shares from ``Sig9``, the [9n, 9n] covariance of [pose | velocity]."""
    n = st.shape[0]
    a, J, _ = A.edge_terms(st[:, 3:7], cumrot)
    o = SimpleNamespace(att_leverage=np.empty(n - 1), att_wtest=np.empty(n - 1), att_mineig=np.empty(n - 1))
    o.att_omega = sa * (a * a).sum(1)
    o.att_a, o.att_J = a, J
    for e in range(n - 1):
        ii = np.concatenate([6 * e + ATT, 6 * (e + 1) + ATT])
        J6 = np.concatenate([J[e, 0], J[e, 1]], 1)
        P = sa * (J6 @ Sig9[np.ix_(ii, ii)] @ J6.T)
        o.att_leverage[e] = np.trace(P)
        M = np.eye(3) - 0.5 * (P + P.T)
        o.att_mineig[e] = np.linalg.eigvalsh(M)[0]
        t2 = sa * a[e] @ np.linalg.solve(M, a[e])
        o.att_wtest[e] = np.sqrt(t2) if (np.linalg.det(M) > 0.0 and t2 >= 0.0) else np.nan
    return o


def edge_restated(J, a, state, edges, sa, fault=None):
    """The device's attitude edge pass in NumPy: ``(att_leverage [n-1], att_wtest [n-1])`` from ``J [n-1,2,3,3]``, ``a [n-1,3]`` and
    the blocks ``state [n,9,9]``, ``edges [n-1,9,9]`` of ``vba_schur_covariance_dyn``.  ``fault`` plants one mistake."""
    comp = np.array([0, 1, 2]) if fault == "position_components" else ATT
    g = lambda M: M[np.ix_(comp, comp)]
    lev, wt = np.empty(J.shape[0]), np.empty(J.shape[0])
    for i in range(J.shape[0]):
        ed = edges[i].T if fault == "edge_transposed" else edges[i]
        Sig = np.block([[g(state[i]), g(ed)], [g(ed).T, g(state[i + 1])]])
        J6 = np.concatenate([J[i, 1], J[i, 0]] if fault == "J_swapped" else [J[i, 0], J[i, 1]], 1)
        s = 1.0 if fault == "no_sigma" else sa
        P = s * (J6 @ Sig @ J6.T)
        lev[i] = (P[0, 0] + P[1, 1]) + P[2, 2]
        M = np.eye(3) - 0.5 * (P + P.T)
        t2 = s * a[i] @ np.linalg.solve(M, a[i])
        wt[i] = np.sqrt(t2) if (np.linalg.det(M) > 0.0 and t2 >= 0.0) else np.nan
    return lev, wt


def fit_of(d, X, r, o, n, fault=None):
    f = Q.fit_of(d, X, r, o, n)
    t_att, om_att = float(o.att_leverage.sum()), float(o.att_omega.sum())
    omega = f["omega"] + om_att
    rho = f["rho"] if fault == "att_not_in_rho" else f["rho"] + 3.0 * (n - 1) - t_att
    fin = o.att_wtest[np.isfinite(o.att_wtest)]
    f.update(omega=omega, rho=rho, s0sq=omega / rho if rho > 0 else float("nan"), t_att=t_att, omega_att=om_att,
             max_att_wtest=float(fin.max(initial=0.0)))
    return {k: f[k] for k in FIT_NAMES}


def _routes(d, st, X, lam, sigma_att=None, second_route=True):
    """Blocks of ``Sigma`` by the two routes: ``(Sig9 [9n,9n], Sigma_pl [6n,3L], Sigma_ll [L,3,3], trace of H^-1)`` each."""
    n = st.shape[0]
    n6, n9 = 6 * n, 9 * n
    B9, Cm, E9, _, _ = A.normal_equations(st, X, *AC.args(d), lam, *AC.factors(d, sigma_att))
    Hinv = np.linalg.inv(np.block([[B9, E9], [E9.T, Cm]]))
    Hinv = 0.5 * (Hinv + Hinv.T)                            # (schur_dyn_rel_cases.evaluate says why)
    one = (Hinv[:n9, :n9], Hinv[:n6, n9:], R._blocks3(Hinv[n9:, n9:]), float(np.trace(Hinv)))
    if not second_route:
        return one, None
    Cinv = np.linalg.inv(R._blocks3(Cm))
    G = np.einsum("alc,lcd->ald", E9.reshape(n9, -1, 3), Cinv).reshape(n9, -1)                  # E9 C^-1
    W = np.linalg.inv(np.linalg.cholesky(B9 - G @ E9.T))
    Sinv = W.T @ W
    SG = Sinv @ G
    two = (Sinv, -SG[:n6], Cinv + np.einsum("alc,ald->lcd", G.reshape(n9, -1, 3), SG.reshape(n9, -1, 3)), None)
    return one, two


def evaluate(d, st, X, lam, sigma_att=None, second_route=True):
    """Reference at the state ``(st, X)`` of problem ``d`` (with ``cumrot``, ``sigma_att``) and damping ``lam``."""
    sd, sa = d["sigma_dyn"], d["sigma_att"] if sigma_att is None else sigma_att
    n, L = st.shape[0], X.shape[0]
    n6, n9 = 6 * n, 9 * n
    one, two = _routes(d, st, X, lam, sigma_att, second_route)
    r, Jc, Jl = S.linearise(st, X, d["uv"], d["w"], d["pose_of_row"], d["landmark_of_row"], d["intrinsics"])
    Sig9 = one[0]
    o = R._families(d, X, r, Jc, Jl, Sig9[:n6, :n6], one[1], one[2])
    o.__dict__.update(Q._edge_family(st, d["time_idx"], sd, Sig9).__dict__)
    o.__dict__.update(_att_family(st, d["cumrot"], sa, Sig9).__dict__)
    o.lam, o.sigma_dyn, o.sigma_att, o.residual, o.trace_Hinv, o.unknowns, o.n = lam, sd, sa, r, one[3], n9 + 3 * L, n
    idx = D.unknown_index(n)
    o.state = np.stack([Sig9[np.ix_(idx[i], idx[i])] for i in range(n)])
    o.edges = np.stack([Sig9[np.ix_(idx[i], idx[i + 1])] for i in range(n - 1)])
    o.kept = ~(o.mineig < EIG_MIN)
    o.lm_kept = ~(o.lm_mineig < LM_EIG_MIN)
    o.lm_stats = stats_of(o.leverage, o.wtest, d["w"], d["landmark_of_row"], L)
    o.pose_stats = stats_of(o.leverage, o.wtest, d["w"], d["pose_of_row"], n)
    o.fit = fit_of(d, X, r, o, n)
    o.identity = o.fit["t_rows"] + o.fit["t_prior"] + o.fit["t_edges"] + o.fit["t_att"] + lam * o.trace_Hinv
    o.cost = A.cost(st, X, *AC.args(d), *AC.factors(d, sigma_att))
    if second_route:
        S2 = two[0]
        o2 = R._families(d, X, r, Jc, Jl, S2[:n6, :n6], two[1], two[2])
        e2 = Q._edge_family(st, d["time_idx"], sd, S2)
        a2 = _att_family(st, d["cumrot"], sa, S2)
        o.att_wtest2, o.att_leverage2 = a2.att_wtest, a2.att_leverage
        o.floor = dict(leverage=rel(o2.leverage, o.leverage), wtest=rel(o2.wtest, o.wtest, o.kept), lm_leverage=rel(o2.lm_leverage, o.lm_leverage),
                       lm_wtest=rel(o2.lm_wtest, o.lm_wtest, o.lm_kept), edge_leverage=rel(e2.edge_leverage, o.edge_leverage),
                       att_leverage=rel(a2.att_leverage, o.att_leverage), att_wtest=rel(a2.att_wtest, o.att_wtest))
    return o


@functools.lru_cache(maxsize=None)
def reference(name, lam, sigma_att=None):
    d = case(name)
    return evaluate(d, d["states0"], d["Xs"], lam, sigma_att)


def bar(r, family):
    return max(100.0 * r.floor[family], 1e-11)


def figures(got, r):
    """Device (or any dict of the seven families, rows in the caller's order) against the reference: error per family relative to the
    largest entry, wtest over ``r.kept``, lm_wtest over ``r.lm_kept``, the attitude families over EVERY edge."""
    mask = dict(wtest=r.kept, lm_wtest=r.lm_kept)
    return {k: rel(np.asarray(got[k]), getattr(r, k), mask.get(k)) for k in FAMILIES}


# ------------------------------------------------------------------------------------------------ outlier power
@functools.lru_cache(maxsize=None)
def power_reference(name, lam):
    """``schur_power_cases.evaluate`` fed with the ``Sigma`` of a handle with both factors."""
    d = case(name)
    st, X = d["states0"], d["Xs"]
    n6 = 6 * st.shape[0]
    one, two = _routes(d, st, X, lam)
    r, Jc, Jl = S.linearise(st, X, d["uv"], d["w"], d["pose_of_row"], d["landmark_of_row"], d["intrinsics"])
    o = PW.figures_from_blocks(d, X, r, Jc, Jl, one[0][:n6, :n6], one[1], one[2])
    o.lam, o.ncp, o.residual = lam, PW.NCP, r
    o.kept = (d["w"] > 0.0) & ~(o.mineig < PW.EIG_MIN)
    o.lm_kept = o.seen & ~(o.q < PW.LM_EIG_MIN)
    o.left_out = int(((d["w"] > 0.0) & (o.mineig < PW.EIG_MIN)).sum())
    o.lm_left_out = int((o.seen & (o.q < PW.LM_EIG_MIN)).sum())
    o2 = PW.figures_from_blocks(d, X, r, Jc, Jl, two[0][:n6, :n6], two[1], two[2])
    o.floor = {k: PW.rel(getattr(o2, k), getattr(o, k), o.kept if k in PW.ROW_FAMILIES else o.lm_kept) for k in PW.FAMILIES}
    return o


# ------------------------------------------------------------------------------------------------ planted faults
def _with_factors(p):
    d = dict(p)
    c = case(PLANT_CASE)
    d["cumrot"], d["sigma_att"] = c["cumrot"], c["sigma_att"]
    return d


@functools.lru_cache(maxsize=None)
def planted_outlier():
    return _with_factors(Q.planted_outlier())


@functools.lru_cache(maxsize=None)
def displaced_landmark():
    return _with_factors(Q.displaced_landmark())


@functools.lru_cache(maxsize=None)
def gyro_fault():
    """29 / 300 with ``cumrot[GYRO_EDGE]`` composed with a rotation of ``GYRO_ANGLE`` about ``GYRO_AXIS`` (a unit quaternion still)."""
    d = dict(case(PLANT_CASE))
    c = d["cumrot"].copy()
    extra = np.concatenate([np.sin(0.5 * GYRO_ANGLE) * GYRO_AXIS, [np.cos(0.5 * GYRO_ANGLE)]])
    c[GYRO_EDGE] = O.qmul(c[GYRO_EDGE][None], extra[None])[0]
    c[GYRO_EDGE] /= np.linalg.norm(c[GYRO_EDGE])
    d["cumrot"], d["gyro_edge"] = c, GYRO_EDGE
    return d


def converge(d, lamda0=1e-4, max_iters=20, tol=1e-10):
    """``SchurBA.solve`` on a handle with both factors, by the oracle: the converged ``(states, X)``."""
    st, X, lam = d["states0"], d["Xs"], lamda0
    for _ in range(max_iters):
        c0, c1, ok, st, X, _, _, _ = A.lm_trial(st, X, *AC.args(d), lam, *AC.factors(d))
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
    d = dict(row=planted_outlier, landmark=displaced_landmark, gyro=gyro_fault)[kind]()
    st, X = converge(d)
    return evaluate(d, st, X, 0.0, second_route=False)
