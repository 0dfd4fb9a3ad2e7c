"""Problems and CPU references of the free-landmark mode WITH the state prior factor, shared by tests/test_schur_prior_host.py and
tests/test_gpu_schur_prior.py (plain module, no tests).  Built once per process; users leave them unchanged.

Cases: 12 / 150, ``12s``, 29 / 300 and 43 / 450 of tests/schur_att_cases.py and ``L12`` of tests/schur_dyn_long_cases.py (gaps of 935 s
and 510 s), each with or without the attitude factor.  Prior sets:

  first     pose 0
  ends      poses 0 and n - 1 (idx is not 0, 1: a prior scattered to pose k shows)
  all       every pose, the ``BA_reg`` shape
  gap       pose 20 of 43 / 450 alone, without the attitude factor: the pose without rows, whose attitude nothing else holds
  flip      ``ends`` with the anchor quaternion of pose 0 negated (the same rotation): d < 0, s = -1
  posonly   pose 0, Lambda non-zero in its position block only: singular, accepted

``Lambda = D^-1 (M M^T) D^-1`` with ``M = I + 0.3 N(0, 1)`` seeded per prior and ``D = diag(0.1 km x3, 1e-3 rad x3, 1e-4 km/s x3)``: full
blocks, so a transposed velocity-pose block or a swapped group shows; symmetrised exactly.  Anchors are the ground truth moved by
about one sigma.  Bars: those of ``schur_dyn_cases.BARS``.
"""
import functools
from types import SimpleNamespace

import numpy as np

import schur_att_cases as AC
import schur_dyn_long_cases as LC
import schur_prior_oracle as P
from oracle import ba_oracle as O

LAMS = AC.LAMS
BARS = AC.BARS
rel, args = AC.rel, AC.args
SIGMAS = np.repeat(np.array([0.1, 1e-3, 1e-4]), 3)
NAMES = ("12", "12s", "29", "43", "L12")
SETS = ("first", "ends", "all", "flip", "posonly")
GAP_CASE, GAP_POSE = "43", AC.EMPTY_POSE["43"]
# (case, set, attitude factor) of every trial: the five sets on every case with and without the attitude factor, and ``gap``
COMBOS = tuple((n, s, a) for n in NAMES for s in SETS for a in (False, True)) + ((GAP_CASE, "gap", False),)


@functools.lru_cache(maxsize=None)
def case(name):
    return LC.att_case(name) if name.startswith("L") else AC.case(name)


def long_gaps(name):
    return name.startswith("L")


def _info(rng):
    M = np.eye(9) + 0.3 * rng.normal(0, 1, (9, 9))
    L = (M @ M.T) / (SIGMAS[:, None] * SIGMAS[None, :])
    return (L + L.T) / 2


@functools.lru_cache(maxsize=None)
def prior(name, pset):
    """(idx int32 [count], anchors [count, 10], infos [count, 9, 9]) of prior set ``pset`` on ``case(name)``."""
    d = case(name)
    gt = d["states_gt"]
    n = gt.shape[0]
    idx = {"first": [0], "ends": [0, n - 1], "all": list(range(n)), "gap": [GAP_POSE], "flip": [0, n - 1], "posonly": [0]}[pset]
    idx = np.array(idx, dtype=np.int32)
    rng = np.random.default_rng(700 + n)
    an = gt[idx].copy()
    k = idx.size
    an[:, :3] += rng.normal(0, SIGMAS[0], (k, 3))
    dq = np.concatenate([rng.normal(0, SIGMAS[3] / 2, (k, 3)), np.ones((k, 1))], 1)
    q = O.qmul(an[:, 3:7], dq / np.linalg.norm(dq, axis=1, keepdims=True))
    an[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    an[:, 7:10] += rng.normal(0, SIGMAS[6], (k, 3))
    infos = np.stack([_info(rng) for _ in range(k)])
    if pset == "flip":
        an[0, 3:7] = -an[0, 3:7]
    if pset == "posonly":
        Z = np.zeros_like(infos)
        Z[:, :3, :3] = infos[:, :3, :3]
        infos = Z
    for a in (idx, an, infos):
        a.setflags(write=False)
    return idx, an, infos


def factors(d, pr, att):
    """The oracle's arguments after the damping."""
    return (d["time_idx"], d["sigma_dyn"], pr) + ((d["cumrot"], d["sigma_att"]) if att else (None, None))


@functools.lru_cache(maxsize=None)
def reference(name, pset, lam, att, full=False, fault=None):
    """One LM trial of ``case(name)`` with prior set ``pset`` (``None``: no prior) by the oracle's Schur route, with the reduced matrix
    and its factor.  ``full``: also the disagreement with the refined full solve, relative to the largest entry -- the floor."""
    d = case(name)
    st, Xs = d["states0"], d["Xs"]
    f = factors(d, None if pset is None else prior(name, pset), att)
    n = st.shape[0]
    r = SimpleNamespace()
    r.c0 = P.cost(st, Xs, *args(d), *f, fault=fault)
    ne = P.normal_equations(st, Xs, *args(d), lam, *f, fault=fault)
    dc9, dl, r.Sm, r.Lc = P.step_schur(*ne)
    s1, X1 = P.apply_step(st, Xs, dc9, dl)
    r.c1 = P.cost(s1, X1, *args(d), *f, fault=fault)
    r.ok = r.c1 < r.c0
    r.st, r.X = (s1, X1) if r.ok else (st, Xs)
    r.dc, r.dv, r.dl = dc9[:6 * n].reshape(n, 6), dc9[6 * n:].reshape(n, 3), dl.reshape(-1, 3)
    if full:
        f9, fl = P.step_full(*ne)
        s2, X2 = P.apply_step(st, Xs, f9, fl)
        c2 = P.cost(s2, X2, *args(d), *f)
        Lc2 = np.linalg.cholesky((r.Sm + r.Sm.T) / 2)
        r.floor = dict(c0=0.0, c1=abs(r.c1 - c2) / c2, dc=rel(dc9[:6 * n], f9[:6 * n]), dv=rel(dc9[6 * n:], f9[6 * n:]), dl=rel(dl, fl),
                       LLt=rel(r.Lc @ r.Lc.T, r.Sm), L=rel(r.Lc, Lc2), states=max(rel(s1, s2), rel(X1, X2)))
    return r


def positive_definite(name, pset, lam, att):
    """Whether the oracle's reduced system of this combination has a Cholesky factor."""
    d = case(name)
    f = factors(d, None if pset is None else prior(name, pset), att)
    B9, C, E9, _, _ = P.normal_equations(d["states0"], d["Xs"], *args(d), lam, *f)
    Ci = np.linalg.inv(C)
    Sm = B9 - E9 @ Ci @ E9.T
    try:
        np.linalg.cholesky((Sm + Sm.T) / 2)
        return True
    except np.linalg.LinAlgError:
        return False


@functools.lru_cache(maxsize=None)
def terms_reference(name, pset):
    """e, J, shares at the start of ``case(name)`` in float64, and the float64 oracle's own error against the longdouble restatement in
    units of 2^-53 of the largest entry: (e, J, shares, units = dict(e=, J=, share=))."""
    d = case(name)
    idx, an, infos = prior(name, pset)
    st = d["states0"][idx]
    e, J = P.prior_terms(st, an)
    el, Jl = P.prior_terms_longdouble(st, an)
    sh, shl = P.prior_shares(e, infos), P.prior_shares(el, infos)
    u = lambda x, xl: float(np.abs(x - xl).max() / np.abs(xl).max() * 2.0 ** 53)
    return e, J, sh, dict(e=u(e, el), J=u(J, Jl), share=u(sh, shl))


def terms_bars(name, pset):
    """The device's bar per figure, the rule of DESIGN 9.5 / 9.9: max(16, 4 x the float64 oracle's own error) units of 2^-53 of the
    largest entry."""
    return {k: max(16.0, 4.0 * v) for k, v in terms_reference(name, pset)[3].items()}


@functools.lru_cache(maxsize=None)
def covariance_reference(name, pset, lam, att):
    """``schur_att_cases.covariance_reference`` with the prior in the system: the families of the state covariance by the dense inverse
    of the oracle's full system, the floor from the second route through the Cholesky factor of the reduced system."""
    import schur_dyn_cov_cases as V
    d = case(name)
    n = d["states0"].shape[0]
    s = V.structure(d)
    f = factors(d, None if pset is None else prior(name, pset), att)
    B9, Cm, E9, _, _ = P.normal_equations(d["states0"], d["Xs"], *args(d), lam, *f)
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


# ------------------------------------------------------------------------------------------------ hand-off
HANDOFF_STEPS = (1, 64, 65, 935)
HANDOFF_NOISE = (1e-8, 1e-12, 1e-14)       # per second: km^2, rad^2, (km/s)^2
HANDOFF_CUMROT = np.array([0.02, -0.05, 0.03, 0.0])
HANDOFF_CUMROT[3] = np.sqrt(1 - (HANDOFF_CUMROT[:3] ** 2).sum())


def handoff_floor(Sigma, state, steps, noise):
    """The oracle's fp64 ``handoff`` against its longdouble run on the same inputs, in sigmas of the information matrix."""
    _, i64 = P.handoff(Sigma, state, steps, HANDOFF_CUMROT, noise)
    _, ild = P.handoff(Sigma, state, steps, HANDOFF_CUMROT, noise, dtype=np.longdouble)
    return P.scaled_info_error(i64, ild)


def split_windows(name="29", cut=15):
    """Windows A (poses 0 .. cut - 1) and B (the rest) of ``case(name)``: the rows of each with pose and landmark indices of its own
    (landmarks a window does not see are dropped), everything else sliced.  B also carries ``gap`` (the steps from A's last pose to
    its pose 0) and ``cumrot_gap``."""
    d = case(name)
    out = []
    for lo, hi in ((0, cut), (cut, d["states0"].shape[0])):
        keep = (d["pose_of_row"] >= lo) & (d["pose_of_row"] < hi)
        lms, lm_new = np.unique(d["landmark_of_row"][keep], return_inverse=True)
        w = dict(states0=d["states0"][lo:hi].copy(), states_gt=d["states_gt"][lo:hi].copy(), X0=d["X0"][lms].copy(), Xs=d["Xs"][lms].copy(),
                 uv=d["uv"][keep].copy(), w=d["w"][keep].copy(), pose_of_row=d["pose_of_row"][keep] - lo, landmark_of_row=lm_new,
                 intrinsics=d["intrinsics"][lo:hi].copy(), sigma=d["sigma"], time_idx=d["time_idx"][lo:hi].copy(), sigma_dyn=d["sigma_dyn"],
                 cumrot=d["cumrot"][lo:hi].copy(), sigma_att=d["sigma_att"])
        out.append(w)
    out[1]["gap"] = int(d["time_idx"][cut] - d["time_idx"][cut - 1])
    out[1]["cumrot_gap"] = d["cumrot"][cut - 1].copy()
    return out
