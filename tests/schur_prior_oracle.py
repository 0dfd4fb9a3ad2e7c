"""CPU restatement of the free-landmark mode WITH the state prior factor (``vba_schur_enable_state_prior``) and of the window hand-off
(``vba_schur_handoff``) -- plain module, no tests.  On top of tests/schur_dyn_oracle.py and tests/schur_att_oracle.py: the same
unknown order ``[6 n pose | 3 n velocity | 3 L landmark]``; component ``c`` of ``x_i = [dp, dtheta, dv]`` is unknown
``schur_dyn_oracle.unknown_index(n)[i, c]``.

Model (quaternions scalar last, ``(x)`` = ``ba_oracle.qmul``), for prior ``k`` on pose ``i = idx[k]`` with anchor
``(pbar, qbar, vbar)`` and information matrix ``Lambda``::

    [eps, d] = conj(qbar) (x) q_i
    s        = d >= 0 ? +1 : -1
    e        = [p_i - pbar, 2 s eps, v_i - vbar]
    F        = blockdiag(I, J, I),   J = s (d I + [eps]x)

along ``ba_oracle.retract``; ``H += F^T Lambda F``, ``g -= F^T Lambda e``, ``cost += sum e^T Lambda e``.

``prior_terms`` works in the precision of its arguments (float64 or longdouble).  ``fault=`` plants one of the mistakes the device
code could make (tests/test_schur_prior_host.py shows that each of them is far outside the bars of the GPU tests):

  vp_transposed   the 3x6 velocity-pose block of F^T Lambda F written transposed (each 3x3 half on its own)
  no_J            J left out (identity)
  no_s            s dropped from the residual and the Jacobian (visible where d < 0: case ``flip``)
  lam_T           Lambda e taken with the transpose of an asymmetric copy of Lambda (its upper triangle doubled, its lower dropped: the
                  same symmetric part) -- a symmetric Lambda hides which of the two a kernel multiplies by, this copy does not
  wrong_pose      prior k scattered to pose k instead of pose idx[k] (visible where idx is not 0, 1, ..: case ``ends``)
  no_cost         the priors' share of the cost left out
  handoff_GtSG    hand-off with G^T Sigma G in the place of G Sigma G^T
  handoff_Rt      hand-off with R transposed
"""
import numpy as np

import exact_orbit as X
import schur_att_oracle as A
import schur_dyn_oracle as D
from oracle import ba_oracle as O
from oracle import schur_oracle as S

FAULTS = ("vp_transposed", "no_J", "no_s", "lam_T", "wrong_pose", "no_cost", "handoff_GtSG", "handoff_Rt")


def prior_terms(states, anchors, fault=None):
    """(e [count, 9], J [count, 3, 3]) of the states [count, 10] of the priors' poses against anchors [count, 10]."""
    w = O.qmul(A.conj(anchors[:, 3:7]), states[:, 3:7])
    eps, d = w[:, :3], w[:, 3]
    s = np.where(d >= 0, 1, -1).astype(states.dtype)
    if fault == "no_s":
        s = np.ones_like(s)
    two = np.array(2, dtype=states.dtype)
    e = np.concatenate([states[:, :3] - anchors[:, :3], two * s[:, None] * eps, states[:, 7:10] - anchors[:, 7:10]], 1)
    J = s[:, None, None] * (d[:, None, None] * np.eye(3, dtype=states.dtype) + A.skew(eps))
    if fault == "no_J":
        J = np.broadcast_to(np.eye(3, dtype=states.dtype), J.shape).copy()
    return e, J


def prior_terms_longdouble(states, anchors):
    """The longdouble restatement of the terms: the same formulas on widened arguments."""
    return prior_terms(np.asarray(states, dtype=np.longdouble), np.asarray(anchors, dtype=np.longdouble))


def prior_shares(e, infos):
    """e^T Lambda e per prior, in the precision of e."""
    return np.einsum("ka,kab,kb->k", e, infos.astype(e.dtype), e)


def prior_blocks(states, prior, fault=None):
    """(H [9n, 9n], g [9n], e, J) of the prior factor alone; prior = (idx, anchors, infos)."""
    idx, anchors, infos = prior
    n = states.shape[0]
    e, J = prior_terms(states[idx], anchors, fault)
    u = D.unknown_index(n)
    H, g = np.zeros((9 * n, 9 * n)), np.zeros(9 * n)
    for k, i in enumerate(idx):
        F = np.eye(9)
        F[3:6, 3:6] = J[k]
        L = infos[k]
        blk = F.T @ L @ F
        if fault == "vp_transposed":
            blk = blk.copy()
            for c0 in (0, 3):
                t = blk[6:9, c0:c0 + 3].T.copy()
                blk[6:9, c0:c0 + 3], blk[c0:c0 + 3, 6:9] = t, t.T
        Le = L @ e[k]
        if fault == "lam_T":
            Le = (2 * np.triu(L, 1) + np.diag(np.diag(L))).T @ e[k]
        rows = u[k if fault == "wrong_pose" else i]
        H[np.ix_(rows, rows)] += blk
        g[rows] -= F.T @ Le
    return H, g, e, J


def prior_cost(states, prior, fault=None):
    if fault == "no_cost":
        return 0.0
    idx, anchors, infos = prior
    e, _ = prior_terms(states[idx], anchors)
    return float(prior_shares(e, infos).sum())


def normal_equations(states, Xl, X0, uv, w, pose_of_row, landmark_of_row, K, sigma, lamda, time_idx, sigma_dyn, prior, cumrot=None, sigma_att=None,
                     fault=None):
    """Dense blocks of [[B9, E9], [E9^T, C]] [dc9; dl] = [v9; wl] with the dynamics factor, the attitude factor if ``cumrot`` is given,
    and the prior (``None``: without it)."""
    a = (states, Xl, X0, uv, w, pose_of_row, landmark_of_row, K, sigma, lamda, time_idx, sigma_dyn)
    B9, C, E9, v9, wl = D.normal_equations(*a) if cumrot is None else A.normal_equations(*a, cumrot, sigma_att)
    if prior is None:
        return B9, C, E9, v9, wl
    H, g, _, _ = prior_blocks(states, prior, fault)
    return B9 + H, C, E9, v9 + g, wl


step_full = D.step_full
step_schur = D.step_schur
apply_step = D.apply_step


def cost(states, Xl, X0, uv, w, pose_of_row, landmark_of_row, K, sigma, time_idx, sigma_dyn, prior, cumrot=None, sigma_att=None, fault=None):
    a = (states, Xl, X0, uv, w, pose_of_row, landmark_of_row, K, sigma, time_idx, sigma_dyn)
    c = D.cost(*a) if cumrot is None else A.cost(*a, cumrot, sigma_att)
    return c if prior is None else c + prior_cost(states, prior, fault)


def lm_trial(states, Xl, X0, uv, w, pose_of_row, landmark_of_row, K, sigma, lamda, time_idx, sigma_dyn, prior, cumrot=None, sigma_att=None):
    """One LM trial as ``vba_schur_iterate`` runs it on such a handle: (c0, c1, accepted, states', X', dc, dv, dl)."""
    n = states.shape[0]
    a = (X0, uv, w, pose_of_row, landmark_of_row, K, sigma)
    f = (time_idx, sigma_dyn, prior, cumrot, sigma_att)
    c0 = cost(states, Xl, *a, *f)
    dc9, dl, _, _ = step_schur(*normal_equations(states, Xl, *a, lamda, *f))
    s1, X1 = apply_step(states, Xl, dc9, dl)
    c1 = cost(s1, X1, *a, *f)
    ok = c1 < c0
    return c0, c1, ok, (s1 if ok else states), (X1 if ok else Xl), dc9[:6 * n].reshape(n, 6), dc9[6 * n:].reshape(n, 3), dl.reshape(-1, 3)


# ------------------------------------------------------------------------------------------------ hand-off
def gap_rotation_matrix(c):
    """R [3, 3] of dtheta' = conj(c) dtheta c, column by column through the quaternion products; the precision of c."""
    eye = np.eye(4, dtype=c.dtype)[:3]
    cols = O.qmul(O.qmul(np.broadcast_to(A.conj(c), (3, 4)), eye), np.broadcast_to(c, (3, 4)))
    return cols[:, :3].T


def handoff(Sigma, state, steps, c, noise=None, fault=None, dtype=np.float64):
    """(anchor [10], info [9, 9]) from the 9x9 marginal ``Sigma`` of ``state`` [10]: Phi and the propagated (p, v) by the exact chain
    (tests/exact_orbit.py), the algebra in ``dtype``, the inverse dense."""
    x0 = np.concatenate([state[:3], state[7:10]])[None]
    xh, Phi = X.propagate(x0, np.array([int(steps)]))
    c = np.asarray(c, dtype=dtype)
    R = gap_rotation_matrix(c)
    if fault == "handoff_Rt":
        R = R.T
    P = Phi[0].astype(dtype)
    G = np.zeros((9, 9), dtype=dtype)
    pv = np.array([0, 1, 2, 6, 7, 8])
    G[np.ix_(pv, pv)] = P
    G[3:6, 3:6] = R
    Sg = np.asarray(Sigma, dtype=dtype)
    Sp = G.T @ Sg @ G if fault == "handoff_GtSG" else G @ Sg @ G.T
    if noise is not None:
        Sp = Sp + np.diag(np.repeat(np.asarray(noise, dtype=dtype), 3)) * dtype(steps)
    Sp = (Sp + Sp.T) / dtype(2)
    info = _inverse(Sp)
    q = O.qmul(np.asarray(state[3:7], dtype=dtype)[None], c[None])[0]
    q = q / np.sqrt((q * q).sum())
    anchor = np.concatenate([xh[0, :3].astype(dtype), q, xh[0, 3:].astype(dtype)])
    return anchor, info


def _inverse(M):
    """Dense inverse in the precision of M (numpy's for float64; Gauss-Jordan with partial pivoting for longdouble)."""
    if M.dtype == np.float64:
        return np.linalg.inv(M)
    n = M.shape[0]
    a = np.concatenate([M.copy(), np.eye(n, dtype=M.dtype)], 1)
    for j in range(n):
        p = j + int(np.argmax(np.abs(a[j:, j])))
        a[[j, p]] = a[[p, j]]
        a[j] = a[j] / a[j, j]
        for r in range(n):
            if r != j:
                a[r] = a[r] - a[r, j] * a[j]
    return a[:, n:]


def scaled_info_error(got, ref):
    """max |got - ref| with every entry divided by sqrt(ref_aa ref_bb): an information matrix in units of its own sigmas."""
    ref = np.asarray(ref, dtype=np.longdouble)
    s = np.sqrt(np.diag(ref))
    return float((np.abs(np.asarray(got, dtype=np.longdouble) - ref) / (s[:, None] * s[None, :])).max())
