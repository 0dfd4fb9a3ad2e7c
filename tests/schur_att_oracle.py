"""CPU restatement of the free-landmark mode WITH the orbit-dynamics factor AND the Gauss-Newton attitude factor
(``vba_schur_enable_attitude``) -- plain module, no tests.  On top of tests/schur_dyn_oracle.py: the same unknown order
``[6 n pose | 3 n velocity | 3 L landmark]``, the attitude unknowns of pose ``i`` being ``6 i + 3 .. 6 i + 5``.

Model (quaternions scalar last, ``(x)`` = ``ba_oracle.qmul``), for every edge ``i -> i + 1`` with ``c_i = cumrot[i]``::

    qp_i   = q_i (x) c_i
    [e, d] = conj(qp_i) (x) q_{i+1}
    s      = d >= 0 ? +1 : -1
    a_i    = s e
    J_next = d a_i / d theta_{i+1} =  1/2 s (d I + [e]x)
    J_own  = d a_i / d theta_i     = -1/2 s (L(conj c_i) R(m_i))[0:3, 0:3],    m_i = conj(q_i) (x) q_{i+1}

along ``ba_oracle.retract``; ``H += sigma_att J^T J``, ``g -= sigma_att J^T a``, ``cost += sigma_att sum |a|^2``.

``edge_terms`` works in the precision of its arguments (float64 or longdouble).  ``fault=`` plants one of the mistakes the device
code could make (tests/test_schur_att_host.py shows that each of them is far outside the bars of the GPU tests):

  sign_Ji        J_own with the wrong sign
  no_s           s dropped from the residual (a = e) and kept in the Jacobians: s^2 = 1 hides a drop in both, and every drop in one
                 of them flips the right-hand side of the edges with d < 0 -- visible on the sign variant only
  swap_J         J_own and J_next taken for each other
  no_transpose   the sub-diagonal block (theta_{i+1}, theta_i) written untransposed
  edge_order     the two edges of a pose taken for each other: J_own of the edge that ends at the pose, J_next of the one that starts
"""
import numpy as np

import schur_dyn_oracle as D
from oracle import ba_oracle as O
from oracle import schur_oracle as S

FAULTS = ("sign_Ji", "no_s", "swap_J", "no_transpose", "edge_order")


def conj(q):
    return q * np.array([-1, -1, -1, 1], dtype=q.dtype)


def left_mult_matrix(p):
    """L(p) [..., 4, 4] with p (x) q = L(p) q."""
    eye = np.eye(4, dtype=p.dtype)
    return np.stack([O.qmul(p, np.broadcast_to(eye[k], p.shape)) for k in range(4)], -1)


def skew(e):
    z = np.zeros_like(e[..., 0])
    return np.stack([np.stack([z, -e[..., 2], e[..., 1]], -1), np.stack([e[..., 2], z, -e[..., 0]], -1),
                     np.stack([-e[..., 1], e[..., 0], z], -1)], -2)


def edge_terms(q, cumrot, fault=None):
    """(a [n-1, 3], J [n-1, 2, 3, 3] = (J_own, J_next), d [n-1]) of the quaternions q [n, 4]; cumrot[n - 1] is ignored."""
    q0, q1, c = q[:-1], q[1:], cumrot[: q.shape[0] - 1]
    w = O.qmul(conj(O.qmul(q0, c)), q1)
    e, d = w[:, :3], w[:, 3]
    s = np.where(d >= 0, 1, -1).astype(q.dtype)
    a = e.copy() if fault == "no_s" else s[:, None] * e
    half = np.array(0.5, dtype=q.dtype)
    Jn = half * s[:, None, None] * (d[:, None, None] * np.eye(3, dtype=q.dtype) + skew(e))
    m = O.qmul(conj(q0), q1)
    Ji = -half * s[:, None, None] * (left_mult_matrix(conj(c)) @ O.right_mult_matrix(m))[:, :3, :3]
    if fault == "sign_Ji":
        Ji = -Ji
    if fault == "swap_J":
        Ji, Jn = Jn, Ji
    return a, np.stack([Ji, Jn], 1), d


def edge_cost(states, cumrot, sigma_att):
    a, _, _ = edge_terms(states[:, 3:7], cumrot)
    return sigma_att * (a * a).sum(1)


def attitude_blocks(states, cumrot, sigma_att, fault=None):
    """(H [9n, 9n], g [9n], a, J) of the attitude factor alone: sigma J^T J and -sigma J^T a on the attitude unknowns."""
    n = states.shape[0]
    a, J, _ = edge_terms(states[:, 3:7], cumrot, fault)
    H, g = np.zeros((9 * n, 9 * n)), np.zeros(9 * n)
    for e in range(n - 1):
        i0, i1 = 6 * e + 3 + np.arange(3), 6 * (e + 1) + 3 + np.arange(3)
        Ji, Jn = J[e]
        if fault == "edge_order":
            Ji, Jn = Jn, Ji                          # ... in what lands on the poses' own blocks and entries
        H[np.ix_(i0, i0)] += sigma_att * Ji.T @ Ji
        H[np.ix_(i1, i1)] += sigma_att * Jn.T @ Jn
        g[i0] -= sigma_att * Ji.T @ a[e]
        g[i1] -= sigma_att * Jn.T @ a[e]
        X = sigma_att * J[e, 1].T @ J[e, 0]          # block (theta_{e+1}, theta_e)
        if fault == "no_transpose":
            X = X.T
        H[np.ix_(i1, i0)] += X
        H[np.ix_(i0, i1)] += X.T
    return H, g, a, J


def normal_equations(states, X, X0, uv, w, pose_of_row, landmark_of_row, K, sigma, lamda, time_idx, sigma_dyn, cumrot, sigma_att, fault=None):
    """Dense blocks of [[B9, E9], [E9^T, C]] [dc9; dl] = [v9; wl] with both factors, dc9 = [dc | dv]."""
    B9, C, E9, v9, wl = D.normal_equations(states, X, X0, uv, w, pose_of_row, landmark_of_row, K, sigma, lamda, time_idx, sigma_dyn)
    H, g, _, _ = attitude_blocks(states, cumrot, sigma_att, fault)
    return B9 + H, C, E9, v9 + g, wl


step_full = D.step_full
step_schur = D.step_schur
apply_step = D.apply_step


def cost(states, X, X0, uv, w, pose_of_row, landmark_of_row, K, sigma, time_idx, sigma_dyn, cumrot, sigma_att):
    return D.cost(states, X, X0, uv, w, pose_of_row, landmark_of_row, K, sigma, time_idx, sigma_dyn) + float(edge_cost(states, cumrot, sigma_att).sum())


def lm_trial(states, X, X0, uv, w, pose_of_row, landmark_of_row, K, sigma, lamda, time_idx, sigma_dyn, cumrot, sigma_att):
    """One LM trial as ``vba_schur_iterate`` runs it on a handle with both factors: (c0, c1, accepted, states', X', dc, dv, dl)."""
    n = states.shape[0]
    a = (X0, uv, w, pose_of_row, landmark_of_row, K, sigma)
    f = (time_idx, sigma_dyn, cumrot, sigma_att)
    c0 = cost(states, X, *a, *f)
    dc9, dl, _, _ = step_schur(*normal_equations(states, X, *a, lamda, *f))
    s1, X1 = apply_step(states, X, dc9, dl)
    c1 = cost(s1, X1, *a, *f)
    ok = c1 < c0
    return c0, c1, ok, (s1 if ok else states), (X1 if ok else X), dc9[:6 * n].reshape(n, 6), dc9[6 * n:].reshape(n, 3), dl.reshape(-1, 3)
