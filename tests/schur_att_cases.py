"""Problems and CPU references of the free-landmark mode WITH the orbit-dynamics factor and the Gauss-Newton attitude factor, shared
by tests/test_schur_att_host.py and tests/test_gpu_schur_att.py (plain module, no tests).  Built once per process; users leave them
unchanged.

The four cases of tests/schur_dyn_cases.py, unchanged (12 / 150, 29 / 300, 43 / 450 with pose 20 without rows, 86 / 900), plus
``cumrot[i] = conj(q_gt[i]) (x) q_gt[i + 1]`` -- the residual at the truth is rounding -- and one variant, ``12s``: 12 / 150 with
``q_1`` of the start negated (the same rotation), which makes ``d < 0`` on edges 0 and 1 and exercises ``s``.

SIGMA_ATT = SIGMA_DYN * QUAT_COEFF / 2 = 5e5: the weight at which the factor weights the attitude as the reference's term does near
the solution.  Bars: those of ``schur_dyn_cases.BARS``.
"""
import functools
from types import SimpleNamespace

import numpy as np

import schur_att_oracle as A
import schur_dyn_cases as DC
from oracle import ba_oracle as O

SIGMA_DYN = DC.SIGMA_DYN
SIGMA_ATT = SIGMA_DYN * O.QUAT_COEFF / 2
LAMS = DC.LAMS
BARS = DC.BARS
NAMES = DC.NAMES + ("12s",)
SIGN_VARIANT = "12s"
EMPTY_POSE = DC.EMPTY_POSE
rel = DC.rel
args = DC.args


@functools.lru_cache(maxsize=None)
def case(name):
    d = dict(DC.case(name[:2]))
    q = d["states_gt"][:, 3:7]
    c = np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (q.shape[0], 1))
    c[:-1] = O.qmul(A.conj(q[:-1]), q[1:])
    d["cumrot"] = c
    d["sigma_att"] = SIGMA_ATT
    if name == SIGN_VARIANT:
        st = d["states0"].copy()
        st[1, 3:7] = -st[1, 3:7]
        d["states0"] = st
    return d


def factors(d, sigma_att=None):
    """The oracle's arguments after the damping."""
    return d["time_idx"], d["sigma_dyn"], d["cumrot"], d["sigma_att"] if sigma_att is None else sigma_att


@functools.lru_cache(maxsize=None)
def reference(name, lam, sigma_att=None, full=False, fault=None):
    """One LM trial of ``case(name)`` by the oracle's Schur route, with the reduced matrix and its factor.  ``full``: also the
    disagreement with the refined full solve, relative to the largest entry -- the floor of this reference."""
    d = case(name)
    st, Xs = d["states0"], d["Xs"]
    f = factors(d, sigma_att)
    n = st.shape[0]
    r = SimpleNamespace()
    r.c0 = A.cost(st, Xs, *args(d), *f)
    ne = A.normal_equations(st, Xs, *args(d), lam, *f, fault=fault)
    dc9, dl, r.Sm, r.Lc = A.step_schur(*ne)
    s1, X1 = A.apply_step(st, Xs, dc9, dl)
    r.c1 = A.cost(s1, X1, *args(d), *f)
    r.ok = r.c1 < r.c0
    r.st, r.X = (s1, X1) if r.ok else (st, Xs)
    r.dc, r.dv, r.dl = dc9[:6 * n].reshape(n, 6), dc9[6 * n:].reshape(n, 3), dl.reshape(-1, 3)
    if full:
        f9, fl = A.step_full(*ne)
        r.floor = dict(dc=rel(dc9[:6 * n], f9[:6 * n]), dv=rel(dc9[6 * n:], f9[6 * n:]), dl=rel(dl, fl))
    return r


@functools.lru_cache(maxsize=None)
def edge_reference(name):
    """a, J, edge costs of the start of ``case(name)`` in float64 and in longdouble, and the float64 oracle's own error against the
    longdouble restatement in units of 2^-53 of the largest entry: (a, J, ecost, units = dict(a=, J=, ecost=))."""
    d = case(name)
    q, c = d["states0"][:, 3:7], d["cumrot"]
    a, J, _ = A.edge_terms(q, c)
    al, Jl, _ = A.edge_terms(q.astype(np.longdouble), c.astype(np.longdouble))
    ec, ecl = d["sigma_att"] * (a * a).sum(1), np.longdouble(d["sigma_att"]) * (al * al).sum(1)
    u = lambda x, xl: float(np.abs(x - xl).max() / np.abs(xl).max() * 2.0 ** 53)
    return a, J, ec, dict(a=u(a, al), J=u(J, Jl), ecost=u(ec, ecl))


def edge_bars(name):
    """The device's bar per figure, as DESIGN 9.5 derives the orbit factor's: max(16, 4 x the float64 oracle's own error) units of
    2^-53 of the largest entry."""
    return {k: max(16.0, 4.0 * v) for k, v in edge_reference(name)[3].items()}


@functools.lru_cache(maxsize=None)
def covariance_reference(name, lam):
    """The reference of ``state_covariance`` on a handle with both factors, as ``schur_dyn_cov_cases.reference`` builds the one of a
    dynamics handle: the blocks of the dense inverse of the oracle's full system, the floor from the second route through the
    Cholesky factor of the reduced system; ``schur_dyn_cov_cases.scaled`` and ``bar`` judge against it."""
    import schur_dyn_cov_cases as V
    d = case(name)
    n = d["states0"].shape[0]
    s = V.structure(d)
    B9, Cm, E9, _, _ = A.normal_equations(d["states0"], d["Xs"], *args(d), lam, *factors(d))
    n9 = B9.shape[0]
    bi, bj = s["blk_i"].astype(np.int64), s["blk_j"].astype(np.int64)
    Hinv = np.linalg.inv(np.block([[B9, E9], [E9.T, Cm]]))
    r = SimpleNamespace(blk_i=bi, blk_j=bj, lam=lam, n=n)
    for k, v in V.families(Hinv[:n9, :n9], V._diag_blocks(Hinv[n9:, n9:], 3), n, bi, bj).items():
        setattr(r, k, v)
    Cinv = np.linalg.inv(V._diag_blocks(Cm, 3))
    G = np.einsum("alc,lcd->ald", E9.reshape(n9, -1, 3), Cinv).reshape(n9, -1)
    W = np.linalg.inv(np.linalg.cholesky(B9 - G @ E9.T))
    Sinv = W.T @ W
    lm2 = Cinv + np.einsum("alc,ald->lcd", G.reshape(n9, -1, 3), (Sinv @ G).reshape(n9, -1, 3))
    r.floor = V.scaled(V.families(Sinv, lm2, n, bi, bj), r)
    return r
