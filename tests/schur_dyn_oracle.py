"""CPU restatement of the free-landmark mode WITH the orbit-dynamics factor (``vba_schur_enable_dynamics``) -- plain module, no tests.

Built from the two oracles this repository already has: the reprojection part is ``oracle.schur_oracle.normal_equations``, the
dynamics part is ``oracle.ba_oracle.orbit_factor`` assembled as the orbit part of ``oracle.ba_oracle.assemble`` does
(``sigma J^T J``, ``-sigma J^T r``), without the fixed-landmark path's ``wmax_scale`` and without the attitude factor.  Unknowns are
ordered ``[6 n pose | 3 n velocity | 3 L landmark]`` as on the device; component ``c`` of ``orbit_factor``'s nine columns of pose
``i`` is unknown ``6 i + c`` for ``c < 6`` and ``6 n + 3 i + (c - 6)`` for the velocity.

Two routes to the same step: the FULL system of ``9 n + 3 L`` unknowns solved densely with iterative refinement in extended
precision, and the Schur route over ``[pose | velocity]`` that the GPU takes.  ``fault=`` plants one of the mistakes the device code
could make (tests/test_schur_dyn_host.py shows that each of them is far outside the bars of the GPU tests).
"""
import numpy as np

from oracle import ba_oracle as O
from oracle import schur_oracle as S

FAULTS = ("sign_F", "no_vel_coeff", "no_transpose", "edge_order")


def unknown_index(n):
    """[n, 9] -> unknown of column c of pose i."""
    idx = np.empty((n, 9), dtype=np.int64)
    idx[:, :6] = 6 * np.arange(n)[:, None] + np.arange(6)
    idx[:, 6:] = 6 * n + 3 * np.arange(n)[:, None] + np.arange(3)
    return idx


def dynamics_blocks(states, time_idx, sigma_dyn, fault=None):
    """(H [9n, 9n], g [9n], r [n-1, 6], E [n-1, 6, 9]) of the dynamics factor alone: sigma J^T J and -sigma J^T r."""
    n = states.shape[0]
    r, E, F = O.orbit_factor(states, np.asarray(time_idx), jacobian=True)
    if fault == "sign_F":
        F = -F
    if fault == "no_vel_coeff":
        F = F.copy()
        F[3:6, 6:9] = -np.eye(3)
    idx = unknown_index(n)
    H, g = np.zeros((9 * n, 9 * n)), np.zeros(9 * n)
    for e in range(n - 1):
        a, b = idx[e], idx[e + 1]
        Ee = E[e]
        if fault == "edge_order":
            # the two edges of a pose taken for each other: the start-of-edge block where the end-of-edge block belongs
            H[np.ix_(b, b)] += sigma_dyn * Ee.T @ Ee
            H[np.ix_(a, a)] += sigma_dyn * F.T @ F
        else:
            H[np.ix_(a, a)] += sigma_dyn * Ee.T @ Ee
            H[np.ix_(b, b)] += sigma_dyn * F.T @ F
        X = sigma_dyn * F.T @ Ee                     # block (pose e + 1, pose e)
        if fault == "no_transpose":
            # (p_{e+1}, v_e) written into its lower-triangle place (v_e, p_{e+1}) without the transpose
            X = X.copy()
            X[0:3, 6:9] = X[0:3, 6:9].T
        H[np.ix_(b, a)] += X
        H[np.ix_(a, b)] += X.T
        g[a] -= sigma_dyn * Ee.T @ r[e]
        g[b] -= sigma_dyn * F.T @ r[e]
    return H, g, r, E


def normal_equations(states, X, X0, uv, w, pose_of_row, landmark_of_row, K, sigma, lamda, time_idx, sigma_dyn, fault=None):
    """Dense blocks of [[B9, E9], [E9^T, C]] [dc9; dl] = [v9; wl], dc9 = [dc | dv]."""
    n = states.shape[0]
    B, C, E, v, wl = S.normal_equations(states, X, X0, uv, w, pose_of_row, landmark_of_row, K, sigma, lamda)
    H, g, _, _ = dynamics_blocks(states, time_idx, sigma_dyn, fault)
    B9 = H
    B9[:6 * n, :6 * n] += B
    B9[6 * n:, 6 * n:] += lamda * np.eye(3 * n)
    E9 = np.concatenate([E, np.zeros((3 * n, E.shape[1]))], 0)
    v9 = g
    v9[:6 * n] += v
    return B9, C, E9, v9, wl


def step_full(B9, C, E9, v9, wl, refine=3):
    """Step from the full system: LU in fp64, the residual of the refinement in extended precision."""
    n9 = B9.shape[0]
    H = np.block([[B9, E9], [E9.T, C]])
    rhs = np.concatenate([v9, wl])
    Hl, rl = H.astype(np.longdouble), rhs.astype(np.longdouble)
    d = np.linalg.solve(H, rhs).astype(np.longdouble)
    for _ in range(refine):
        d = d + np.linalg.solve(H, (rl - Hl @ d).astype(np.float64))
    d = d.astype(np.float64)
    return d[:n9], d[n9:]


step_schur = S.step_schur               # (dc9, dl, S9, chol(S9)): the landmark blocks are the same 3x3 blocks


def cost(states, X, X0, uv, w, pose_of_row, landmark_of_row, K, sigma, time_idx, sigma_dyn):
    r = O.orbit_factor(states, np.asarray(time_idx), jacobian=False)
    return S.cost(states, X, X0, uv, w, pose_of_row, landmark_of_row, K, sigma) + float(sigma_dyn * (r * r).sum())


def apply_step(states, X, dc9, dl):
    n = states.shape[0]
    d9 = np.zeros((n, 9))
    d9[:, :6] = dc9[:6 * n].reshape(n, 6)
    d9[:, 6:] = dc9[6 * n:].reshape(n, 3)
    return O.retract(states, d9), X + dl.reshape(-1, 3)


def lm_trial(states, X, X0, uv, w, pose_of_row, landmark_of_row, K, sigma, lamda, time_idx, sigma_dyn):
    """One LM trial as ``vba_schur_iterate`` runs it on a dynamics handle: (c0, c1, accepted, states', X', dc, dv, dl)."""
    n = states.shape[0]
    a = (X0, uv, w, pose_of_row, landmark_of_row, K, sigma)
    c0 = cost(states, X, *a, time_idx, sigma_dyn)
    dc9, dl, _, _ = step_schur(*normal_equations(states, X, *a, lamda, time_idx, sigma_dyn))
    s1, X1 = apply_step(states, X, dc9, dl)
    c1 = cost(s1, X1, *a, time_idx, sigma_dyn)
    ok = c1 < c0
    return c0, c1, ok, (s1 if ok else states), (X1 if ok else X), dc9[:6 * n].reshape(n, 6), dc9[6 * n:].reshape(n, 3), dl.reshape(-1, 3)
