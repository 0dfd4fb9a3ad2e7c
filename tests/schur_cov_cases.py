"""CPU reference of ``vba_schur_covariance`` shared by tests/test_schur_cov_host.py and tests/test_gpu_schur_cov.py (plain module,
no tests).  Problems are those of tests/schur_cases.py plus ``"12"`` (12 poses / 150 landmarks: one panel).

Reference: the blocks of ``inv([[B, E], [E^T, C]])`` from ``oracle.schur_oracle.normal_equations``.  Its FLOOR is its disagreement
with a second NumPy route (``W = inv(cholesky(S))``, ``S^-1 = W^T W``, ``C^-1 + C^-1 E^T S^-1 E C^-1``), relative to the largest
entry of the block family (``pose``: diagonal 6x6 blocks, ``pairs``: the blocks of the uploaded list, ``landmark``: 3x3 blocks).
The device is held to ``max(100 x floor, 1e-11)`` per family (:func:`bar`); the floor never comes from the device.
References are built once per process and must be left unchanged by their users.
"""
import functools
from types import SimpleNamespace

import numpy as np

import schur_cases as C
from oracle import schur_oracle as S

# (case, lamda) pairs the GPU tests hold against the reference; behind_the_camera at 1e4 as the trial tests run it
CASES = (("12", 0.0), ("12", 1e-3), ("43", 0.0), ("43", 1e-3), ("128", 1e-3), ("129", 1e-3), ("wide", 1e-3), ("pose_without_rows", 1e-3),
         ("more_landmarks_than_rows", 0.0), ("more_landmarks_than_rows", 1e-3), ("more_poses_than_landmarks", 1e-3),
         ("behind_the_camera", 1e4))
CLAMP = "behind_the_camera"
FAMILIES = ("pose", "pairs", "landmark")


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "12":
        d = C.problem(12, 150, 1)
        d.setdefault("Xs", d["X0"])
        return d
    return C.case(name)


def _diag_blocks(M, k):
    n = M.shape[0] // k
    return np.stack([M[k * i:k * i + k, k * i:k * i + k] for i in range(n)])


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@functools.lru_cache(maxsize=None)
def reference(name, lam):
    d = case(name)
    s = C.structure(d)
    B, Cm, E, _, _ = S.normal_equations(d["states0"], d["Xs"], *C.args(d), lam)
    n6 = B.shape[0]
    bi, bj = s["blk_i"].astype(np.int64), s["blk_j"].astype(np.int64)
    listed = lambda M: np.stack([M[6 * i:6 * i + 6, 6 * j:6 * j + 6] for i, j in zip(bi, bj)])
    Hinv = np.linalg.inv(np.block([[B, E], [E.T, Cm]]))
    r = SimpleNamespace(blk_i=bi, blk_j=bj, lam=lam, sigma=d["sigma"])
    r.pose, r.pairs, r.landmark = _diag_blocks(Hinv[:n6, :n6], 6), listed(Hinv[:n6, :n6]), _diag_blocks(Hinv[n6:, n6:], 3)
    # second route
    r.Cinv = np.linalg.inv(_diag_blocks(Cm, 3))
    G = np.einsum("alc,lcd->ald", E.reshape(n6, -1, 3), r.Cinv).reshape(n6, -1)             # E C^-1
    Sm = B - G @ E.T
    W = np.linalg.inv(np.linalg.cholesky(Sm))
    Sinv = W.T @ W
    lm2 = r.Cinv + np.einsum("alc,ald->lcd", G.reshape(n6, -1, 3), (Sinv @ G).reshape(n6, -1, 3))
    r.floor = dict(pose=rel(_diag_blocks(Sinv, 6), r.pose), pairs=rel(listed(Sinv), r.pairs), landmark=rel(lm2, r.landmark))
    r.Bdiag = _diag_blocks(B, 6)
    r.condS = float(np.linalg.cond(Sm))
    return r


def bar(r, family):
    return max(100.0 * r.floor[family], 1e-11)


def definiteness(pose, landmark, r):
    """Margins of the three orderings, each in units of the prior variance (>= -1e-9 passes): ``sigma^2 I - lm_cov`` (meaningful at
    ``lamda = 0``), ``lm_cov - C_l^-1`` and ``pose_cov_i - B_i^-1`` (the frozen-landmark conditional): the smallest eigenvalue."""
    s2 = r.sigma ** 2
    sym = lambda M: 0.5 * (M + np.swapaxes(M, -1, -2))
    mineig = lambda M: float(np.linalg.eigvalsh(sym(M)).min())
    return dict(below_prior=mineig(s2 * np.eye(3) - landmark) / s2, above_conditional=mineig(landmark - r.Cinv) / s2,
                pose_above_frozen=mineig(pose - np.linalg.inv(r.Bdiag)) / s2)
