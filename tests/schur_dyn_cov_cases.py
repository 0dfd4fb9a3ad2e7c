"""CPU reference of ``vba_schur_covariance_dyn`` / ``SchurBA.state_covariance`` shared by tests/test_schur_dyn_cov_host.py and
tests/test_gpu_schur_dyn_cov.py (plain module, no tests).  Problems are those of tests/schur_dyn_cases.py, at its ``SIGMA_DYN``.

Cases, each the smallest shape that reaches its edge (tiles of 64; ``N = 9 n`` unknowns ordered ``[6 n pose | 3 n velocity]``):

  12 / 150    N = 108: 2 tiles, the pose / velocity boundary 6 n = 72 inside tile 1, every gap 1 s
  29 / 300    N = 261: 5 tiles and two panels, 6 n = 174 inside tile 2, gaps 1 / 5 / 64 s
  43 / 450    pose 20 has no rows: at lamda = 0 its attitude rows of S9 are exactly zero (the failure case)
  86 / 900    N = 774: 13 tiles and four panels, 6 n = 516 four rows into tile 8, velocity tiles far from the pose band

Reference: the blocks of the dense ``inv([[B9, E9], [E9^T, C]])`` from ``schur_dyn_oracle.normal_equations``.  Its FLOOR is its
disagreement with a second NumPy route (``W = inv(cholesky(S9))``, ``S9^-1 = W^T W``, ``C^-1 + C^-1 E9^T S9^-1 E9 C^-1``).

Position, attitude and velocity variances differ by six orders of magnitude, so an error relative to the largest entry of a family
would hide the attitude and velocity blocks.  Every entry is judged scaled by the reference sigmas of its own row and column,
``|d_ab| / sqrt(ref_aa ref_bb)``, the maximum per family (``state``, ``edges``, ``pairs``, ``landmark``).  The device is held to
``max(100 x floor, 1e-11)`` per family (:func:`bar`, the rule of DESIGN 9.1); the floor never comes from the device.
References are built once per process and must be left unchanged by their users.
"""
import functools
from types import SimpleNamespace

import numpy as np

import schur_dyn_cases as DC
import schur_dyn_oracle as D
from vinsat_amd.schur import build_structure

# (case, lamda) pairs the GPU tests hold against the reference; FAILURE is not positive definite (reference and device alike)
CASES = (("12", 0.0), ("12", 1e-3), ("29", 0.0), ("29", 1e-3), ("43", 1e-3), ("86", 0.0), ("86", 1e-3))
FAILURE = ("43", 0.0)
FAMILIES = ("state", "edges", "pairs", "landmark")
FAULTS = ("next_velocity", "edge_transposed", "offset", "upper_unmirrored", "no_cross")
TILE = 64

case = DC.case


def structure(d):
    return build_structure(d["pose_of_row"], d["landmark_of_row"], d["states0"].shape[0], d["X0"].shape[0])[1]


def unknown(n, i, c, off=None):
    """u(i, c): the unknown of component c of [dp, dtheta, dv] of pose i in S9 (``off``: a planted velocity offset)."""
    off = 6 * n if off is None else off
    return np.where(c < 6, 6 * i + c, off + 3 * i + (c - 6))


def gather(stored, n, fault=None):
    """The NumPy restatement of k_state_gather: ``(state [n,9,9], edges [n-1,9,9])`` from ``stored``, an array that holds S9^-1 in
    its LOWER triangle only (the upper one may hold anything: on the device it holds what the factorisation left).  Entry (a, c)
    of the block of poses (i, j) is read at ``(max, min)`` of ``u(i, a), u(j, c)``.  ``fault`` plants one mistake."""
    a, c = np.meshgrid(np.arange(9), np.arange(9), indexing="ij")
    off = 6 * (n - 1) if fault == "offset" else None

    def block(i, j):
        ia = np.where((a >= 6) & (fault == "next_velocity"), min(i + 1, n - 1), i)
        p, q = unknown(n, ia, a, off), unknown(n, j, c, off)
        if fault == "upper_unmirrored":
            out = stored[p, q]
        else:
            out = stored[np.maximum(p, q), np.minimum(p, q)]
        if fault == "no_cross":
            out = np.where((a >= 6) != (c >= 6), 0.0, out)
        return out

    state = np.stack([block(i, i) for i in range(n)])
    edges = np.stack([block(i, i + 1) for i in range(n - 1)])
    if fault == "edge_transposed":
        edges = np.swapaxes(edges, 1, 2)
    return state, edges


def read_entries(n, blk_i, blk_j):
    """Every (row, column) of the stored triangle that some output reads: the gathers' entries, for the tile list."""
    a, c = np.meshgrid(np.arange(9), np.arange(9), indexing="ij")
    rows, cols = [], []
    for i, j in [(i, i) for i in range(n)] + [(i, i + 1) for i in range(n - 1)]:
        p, q = unknown(n, i, a), unknown(n, j, c)
        rows.append(np.maximum(p, q).ravel()), cols.append(np.minimum(p, q).ravel())
    a6, c6 = np.meshgrid(np.arange(6), np.arange(6), indexing="ij")
    for i, j in zip(blk_i, blk_j):
        p, q = (6 * i + np.maximum(a6, c6), 6 * i + np.minimum(a6, c6)) if i == j else (6 * i + a6, 6 * j + c6)
        rows.append(p.ravel()), cols.append(q.ravel())
    return np.concatenate(rows), np.concatenate(cols)


def listed_tiles(n, blk_i, blk_j):
    """The tile list of the selected product as the host builds it: sorted unique (I, J) of the entries read."""
    r, c = read_entries(n, blk_i, blk_j)
    return sorted(set(zip((r // TILE).tolist(), (c // TILE).tolist())))


def _diag_blocks(M, k):
    n = M.shape[0] // k
    return np.stack([M[k * i:k * i + k, k * i:k * i + k] for i in range(n)])


def families(Sinv, lm, n, bi, bj):
    """The four families out of a full symmetric S9^-1 and the landmark blocks, by the oracle's own unknown order (not by
    :func:`gather`, which restates the device and is tested against this)."""
    idx = D.unknown_index(n)
    state = np.stack([Sinv[np.ix_(idx[i], idx[i])] for i in range(n)])
    edges = np.stack([Sinv[np.ix_(idx[i], idx[i + 1])] for i in range(n - 1)])
    pairs = np.stack([Sinv[6 * i:6 * i + 6, 6 * j:6 * j + 6] for i, j in zip(bi, bj)])
    return dict(state=state, edges=edges, pairs=pairs, landmark=lm)


def scaled(got, r):
    """Per family: the largest ``|got - ref| / sqrt(ref_aa ref_bb)``, a and b the unknowns of the entry's row and column."""
    sd_state = np.sqrt(np.diagonal(r.state, axis1=1, axis2=2))          # [n, 9]
    sd_lm = np.sqrt(np.diagonal(r.landmark, axis1=1, axis2=2))          # [L, 3]
    scale = dict(state=sd_state[:, :, None] * sd_state[:, None, :], edges=sd_state[:-1, :, None] * sd_state[1:, None, :],
                 pairs=sd_state[r.blk_i][:, :6, None] * sd_state[r.blk_j][:, None, :6], landmark=sd_lm[:, :, None] * sd_lm[:, None, :])
    return {k: float((np.abs(np.asarray(got[k]) - getattr(r, k)) / scale[k]).max()) for k in FAMILIES}


@functools.lru_cache(maxsize=None)
def reference(name, lam, sigma_dyn=None):
    d = case(name)
    sd = d["sigma_dyn"] if sigma_dyn is None else sigma_dyn
    n = d["states0"].shape[0]
    s = structure(d)
    B9, Cm, E9, _, _ = D.normal_equations(d["states0"], d["Xs"], *DC.args(d), lam, d["time_idx"], sd)
    n9 = B9.shape[0]
    bi, bj = s["blk_i"].astype(np.int64), s["blk_j"].astype(np.int64)
    Hinv = np.linalg.inv(np.block([[B9, E9], [E9.T, Cm]]))
    r = SimpleNamespace(blk_i=bi, blk_j=bj, lam=lam, n=n)
    for k, v in families(Hinv[:n9, :n9], _diag_blocks(Hinv[n9:, n9:], 3), n, bi, bj).items():
        setattr(r, k, v)
    # second route
    Cinv = np.linalg.inv(_diag_blocks(Cm, 3))
    G = np.einsum("alc,lcd->ald", E9.reshape(n9, -1, 3), Cinv).reshape(n9, -1)              # E9 C^-1
    r.S9 = B9 - G @ E9.T
    r.Lc = np.linalg.cholesky(r.S9)
    W = np.linalg.inv(r.Lc)
    r.Sinv = W.T @ W
    lm2 = Cinv + np.einsum("alc,ald->lcd", G.reshape(n9, -1, 3), (r.Sinv @ G).reshape(n9, -1, 3))
    r.floor = scaled(families(r.Sinv, lm2, n, bi, bj), r)
    r.condS = float(np.linalg.cond(r.S9))
    return r


def bar(r, family):
    return max(100.0 * r.floor[family], 1e-11)


@functools.lru_cache(maxsize=None)
def failure_system():
    """S9 of the failure case (43 / 450 at lamda = 0) by the oracle: the attitude rows of the pose without rows are exactly zero."""
    name, lam = FAILURE
    d = case(name)
    B9, Cm, E9, _, _ = D.normal_equations(d["states0"], d["Xs"], *DC.args(d), lam, d["time_idx"], d["sigma_dyn"])
    n9 = B9.shape[0]
    Cinv = np.linalg.inv(_diag_blocks(Cm, 3))
    G = np.einsum("alc,lcd->ald", E9.reshape(n9, -1, 3), Cinv).reshape(n9, -1)
    return B9, Cm, E9, B9 - G @ E9.T
