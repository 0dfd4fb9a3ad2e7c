"""Problems and CPU references shared by tests/test_schur_gpu.py and tests/test_schur_oracle.py (plain module, no tests).

Every problem is a dict as ``synth.make_tracked_landmarks`` returns it plus ``states0`` (the perturbed start), ``w`` and ``Xs``
(the landmark part of the state the trial starts from; the catalogue ``X0`` unless a case says otherwise).  Problems and
references are built once per process and must be left unchanged by their users.
"""
import functools
import os
import re
from types import SimpleNamespace

import numpy as np

from oracle import ba_oracle as O
from oracle import schur_oracle as S
from vinsat_amd import synth
from vinsat_amd.schur import build_structure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATE_FAILURE_SEED = 1           # seed of the "late_failure" problem: chosen so that its first bad pivot is unambiguous


def kernel_constants():
    """``(kT, kPanel)`` as csrc/vba_schur.hip defines them: the shapes below reach their branches for 64 x 4 only."""
    with open(os.path.join(ROOT, "vinsat_amd", "csrc", "vba_schur.hip")) as f:
        src = f.read()
    return tuple(int(re.search(r"constexpr int %s = (\d+);" % k, src).group(1)) for k in ("kT", "kPanel"))


def padded_shape(n_poses):
    """``(N, Npad, panels)`` of the reduced system as ``vba_schur_create`` sizes it."""
    kT, kPanel = kernel_constants()
    N = 6 * n_poses
    panels = (N + kT * kPanel - 1) // (kT * kPanel)
    return N, panels * kT * kPanel, panels


def problem(n_poses, n_landmarks, seed):
    d = synth.make_tracked_landmarks(n_poses=n_poses, n_landmarks=n_landmarks, seed=seed)
    rng = np.random.default_rng(seed + 100)
    st = d["states_gt"].copy()
    st[:, :3] += rng.normal(0, 2.0, (st.shape[0], 3))
    dq = np.concatenate([rng.normal(0, 2e-3, (st.shape[0], 3)), np.ones((st.shape[0], 1))], 1)
    st[:, 3:7] = O.qmul(st[:, 3:7], dq / np.linalg.norm(dq, axis=1, keepdims=True))
    d["states0"] = st
    d["w"] = np.full(d["uv"].shape[0], 0.95)
    return d


def _keep_rows(d, keep):
    for k in ("uv", "w", "pose_of_row", "landmark_of_row"):
        d[k] = d[k][keep]


def _append_rows(d, poses, landmarks, uv):
    d["pose_of_row"] = np.concatenate([d["pose_of_row"], poses])
    d["landmark_of_row"] = np.concatenate([d["landmark_of_row"], landmarks])
    d["uv"] = np.concatenate([d["uv"], uv])
    d["w"] = np.concatenate([d["w"], np.full(len(poses), 0.95)])


def _wide_band():
    """129 / 1300 plus 20 rows that observe landmarks of the first ten poses from the last ten: the reduced system is full."""
    d = problem(129, 1300, 1)
    n = d["states0"].shape[0]
    rng = np.random.default_rng(7)
    early = np.unique(d["landmark_of_row"][d["pose_of_row"] < 10])
    lms = rng.choice(early, 20, replace=False)                     # distinct landmarks: every added pair is unique
    poses = n - 1 - np.arange(20) % 10
    assert not np.any(np.isin(d["landmark_of_row"][d["pose_of_row"] >= n - 10], lms))       # ... and new
    est = O.landmark_project(d["states_gt"], d["X_true"][lms], d["intrinsics"], poses, jacobian=False)
    _append_rows(d, poses, lms, est + rng.normal(0.0, 1.0, est.shape))
    return d


def _late_failure():
    """129 / 1300 with negative weights on the rows of the last 30 poses: not positive definite from somewhere in the third panel."""
    d = problem(129, 1300, LATE_FAILURE_SEED)
    d["w"] = np.where(d["pose_of_row"] >= d["states0"].shape[0] - 30, -d["w"], d["w"])
    return d


def _pose_without_rows():
    d = problem(12, 150, 1)
    _keep_rows(d, d["pose_of_row"] != 6)
    d["empty_pose"] = 6
    return d


def _more_landmarks_than_rows():
    """Every fifth row, and unobserved landmarks appended until L = 400 > m; the unobserved ones start off their catalogue place."""
    d = problem(12, 150, 1)
    _keep_rows(d, np.arange(d["uv"].shape[0]) % 5 == 0)
    rng = np.random.default_rng(11)
    extra = 400 - d["X0"].shape[0]
    d["X0"] = np.concatenate([d["X0"], d["X0"][rng.integers(0, d["X0"].shape[0], extra)] + rng.normal(0, 5.0, (extra, 3))])
    d["X_true"] = np.concatenate([d["X_true"], d["X0"][-extra:]])
    seen = np.zeros(400, dtype=bool)
    seen[d["landmark_of_row"]] = True
    d["unobserved"] = np.nonzero(~seen)[0]
    Xs = d["X0"].copy()
    Xs[~seen] += rng.normal(0, 0.03, (int((~seen).sum()), 3))
    d["Xs"] = Xs
    return d


def _more_poses_than_landmarks():
    """Only the 8 most-observed landmarks and their rows: L = 8 < n = 12."""
    d = problem(12, 150, 1)
    cnt = np.bincount(d["landmark_of_row"], minlength=d["X0"].shape[0])
    top = np.sort(np.argsort(-cnt, kind="stable")[:8])
    _keep_rows(d, np.isin(d["landmark_of_row"], top))
    d["landmark_of_row"] = np.searchsorted(top, d["landmark_of_row"])
    d["X0"], d["X_true"] = d["X0"][top], d["X_true"][top]
    return d


def _behind_the_camera():
    """Five more landmarks, each seen once, 1 km BEHIND the camera plane of its pose at the start and within 5 m of the optical
    axis: the depth is clamped (Z_MIN) and the derivative along the axis is switched off, in the oracle as on the device."""
    d = problem(12, 150, 1)
    rng = np.random.default_rng(13)
    poses = np.array([1, 3, 5, 8, 10])
    st = d["states0"][poses]
    R = O.rotation_matrix(st[:, 3:7] / np.linalg.norm(st[:, 3:7], axis=1, keepdims=True))        # camera -> ECI
    pc = np.concatenate([rng.uniform(-0.005, 0.005, (5, 2)) / np.sqrt(2.0), -np.ones((5, 1))], 1)
    X = st[:, :3] + np.einsum("kij,kj->ki", R, pc)
    L = d["X0"].shape[0]
    d["X0"], d["X_true"] = np.concatenate([d["X0"], X]), np.concatenate([d["X_true"], X])
    lms = L + np.arange(5)
    est = O.landmark_project(d["states0"], X, d["intrinsics"], poses, jacobian=False)
    _append_rows(d, poses, lms, est + rng.normal(0.0, 1.0, est.shape))
    d["clamped_rows"] = np.arange(d["uv"].shape[0] - 5, d["uv"].shape[0])
    return d


_MAKERS = {"43": lambda: problem(43, 450, 1), "128": lambda: problem(128, 1300, 1), "129": lambda: problem(129, 1300, 1),
           "wide": _wide_band, "late_failure": _late_failure, "pose_without_rows": _pose_without_rows,
           "more_landmarks_than_rows": _more_landmarks_than_rows, "more_poses_than_landmarks": _more_poses_than_landmarks,
           "behind_the_camera": _behind_the_camera}
NARROW = ("43", "128", "129")
EDGES = ("pose_without_rows", "more_landmarks_than_rows", "more_poses_than_landmarks", "behind_the_camera")


@functools.lru_cache(maxsize=None)
def case(name):
    d = _MAKERS[name]()
    d.setdefault("Xs", d["X0"])
    return d


def args(d):
    """Arguments of the oracle's functions after (states, X)."""
    return d["X0"], d["uv"], d["w"], d["pose_of_row"], d["landmark_of_row"], d["intrinsics"], d["sigma"]


@functools.lru_cache(maxsize=None)
def reference(name, lam, full=False):
    """One LM trial of ``case(name)`` by the oracle, as ``S.lm_trial`` runs it (the same calls in the same order, the normal
    equations formed once), with the reduced matrix and its factor.  ``full``: also the step of the full system and the
    disagreement of the two routes, relative to the largest entry -- the noise floor of this reference."""
    d = case(name)
    st, X = d["states0"], d["Xs"]
    r = SimpleNamespace()
    r.c0 = S.cost(st, X, *args(d))
    B, C, E, v, wl = S.normal_equations(st, X, *args(d), lam)
    dc, dl, r.Sm, r.Lc = S.step_schur(B, C, E, v, wl)
    s1, X1 = S.apply_step(st, X, dc, dl)
    r.c1 = S.cost(s1, X1, *args(d))
    r.ok = r.c1 < r.c0
    r.st, r.X = (s1, X1) if r.ok else (st, X)
    r.dc, r.dl = dc.reshape(-1, 6), dl.reshape(-1, 3)
    if full:
        dcf, dlf = S.step_full(B, C, E, v, wl)
        r.floor_dc = np.abs(dc - dcf).max() / np.abs(dcf).max()
        r.floor_dl = np.abs(dl - dlf).max() / np.abs(dlf).max()
    return r


@functools.lru_cache(maxsize=None)
def late_failure_reference():
    """The oracle's reduced matrix of the late_failure case at lam = 0, its first bad pivot (row, pivots up to it)."""
    d = case("late_failure")
    B, Cm, E, v, wl = S.normal_equations(d["states0"], d["Xs"], *args(d), 0.0)
    Cinv = np.zeros_like(Cm)
    for l in range(Cm.shape[0] // 3):
        q = slice(3 * l, 3 * l + 3)
        Cinv[q, q] = np.linalg.inv(Cm[q, q])
    Sm = B - E @ Cinv @ E.T
    row, piv = first_bad_pivot(Sm)
    return Sm, row, piv


def structure(d):
    return build_structure(d["pose_of_row"], d["landmark_of_row"], d["states0"].shape[0], d["X0"].shape[0])[1]


def tile_bandwidth(s, tile=64):
    """Largest distance from the diagonal of a non-zero tile of the reduced system, as ``vba_schur_upload`` derives it."""
    return int(((6 * s["blk_i"].astype(np.int64) + 5) // tile - (6 * s["blk_j"].astype(np.int64)) // tile).max())


def tiles_beyond_band_are_zero(Lc, bw, tile=64):
    """The factor is EXACTLY zero in every tile further than ``bw`` from the diagonal (what ``k_trsv_step`` skips)."""
    nb = (Lc.shape[0] + tile - 1) // tile
    beyond = [(I, J) for I in range(nb) for J in range(nb) if I - J > bw]
    return len(beyond), all(not Lc[I * tile:(I + 1) * tile, J * tile:(J + 1) * tile].any() for I, J in beyond)


def first_bad_pivot(Sm):
    """Plain right-looking Cholesky that stops at the first pivot <= 0: (its row or -1, the pivots met up to and including it)."""
    A = np.array(Sm, dtype=np.float64)
    piv = []
    for j in range(A.shape[0]):
        d = A[j, j]
        piv.append(d)
        if not d > 0.0:
            return j, np.array(piv)
        l = A[j + 1:, j] / np.sqrt(d)
        A[j + 1:, j + 1:] -= np.outer(l, l)
    return -1, np.array(piv)


def pairs_by_brute_force(rp, rl, L):
    """{(i, j): set of (k, k2)}: for every landmark, every pair of its (sorted) rows with pose(k) >= pose(k2), k2 = k included."""
    out = {}
    for l in range(L):
        rows = np.nonzero(rl == l)[0]
        for k in rows:
            for k2 in rows:
                if rp[k] > rp[k2] or k == k2:
                    out.setdefault((int(rp[k]), int(rp[k2])), set()).add((int(k), int(k2)))
    return out
