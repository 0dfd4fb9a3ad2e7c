"""Problems and CPU references of the free-landmark mode WITH the dynamics factor, shared by tests/test_schur_dyn_host.py and
tests/test_gpu_schur_dyn.py (plain module, no tests).  Built once per process; users leave them unchanged.

A problem is ``synth.make_tracked_landmarks`` at the case's own pose times (the generator of tests/schur_cases.py; its trajectory is
the oracle's one-second J2 RK4 chain) with the position and velocity columns of ``states_gt`` replaced by the EXACT chain of
tests/exact_orbit.py from pose 0 over ``time_idx`` (extended precision, rounded once: the dynamics residual at the truth is
rounding), then perturbed as ``schur_cases.problem`` perturbs (2 km, 2e-3 in attitude) plus 2 m/s in velocity and 20 m on the
landmarks the trial starts from.

Poses / landmarks (before unseen landmarks are dropped), and why:

  12 / 150    one panel of 256 (9 n = 108), every gap 1 s
  29 / 300    9 n = 261 is two panels where 6 n = 174 is one: enabling the factor changes the panel count.  Gaps mixed 1, 5, 64 s,
              a 64 beside a 1
  43 / 450    two panels either way (258 / 387); pose 20 has no row: the dynamics alone hold it
  86 / 900    9 n = 774 is four panels: two successive bulk updates on the second stream, a 250-row identity tail, and tiles of
              the factor (velocity rows against pose columns) far beyond the band of the reprojection blocks

SIGMA_DYN: the weight of the dynamics factor in every case, the fixed-landmark path's first value (``oracle.ba_oracle.lm_schedule(0)``:
sigma = 1e4, rising to 1e6).  At 1e4 and at 1e6 the oracle's own two routes agree to better than a tenth of every step bar on
every case (at most 8.3e-10 against 1e-8; tests/test_schur_dyn_host.py asserts it at SIGMA_DYN, DESIGN 9.5 has the table).
"""
import functools
from types import SimpleNamespace

import numpy as np

import exact_orbit as X
import schur_dyn_oracle as D
from oracle import ba_oracle as O
from oracle import schur_oracle as S
from vinsat_amd import synth

SIGMA_DYN = float(O.lm_schedule(0)[1])
LAMS = (1e-3, 1e-6)
# bars of DESIGN 9 (relative to the largest entry); dv answers to the bar of dc
BARS = dict(c0=1e-10, c1=1e-7, dc=1e-7, dv=1e-7, dl=1e-7, LLt=1e-11, L=1e-8, states=1e-9)

_GAPS = {
    "12": lambda n: np.ones(n - 1, dtype=np.int64),
    "29": lambda n: np.resize(np.array([5, 1, 64, 1, 5, 5, 64, 5, 1, 1]), n - 1),
    "43": lambda n: np.resize(np.array([5, 3, 5, 7, 2]), n - 1),
    "86": lambda n: np.resize(np.array([3, 5, 2, 4]), n - 1),
}
_SHAPES = {"12": (12, 150), "29": (29, 300), "43": (43, 450), "86": (86, 900)}
NAMES = tuple(_SHAPES)
EMPTY_POSE = {"43": 20}


@functools.lru_cache(maxsize=None)
def case(name, seed=1):
    n, L = _SHAPES[name]
    gaps = _GAPS[name](n)
    times = 10 + np.concatenate([[0], np.cumsum(gaps)])
    d = synth.make_tracked_landmarks(n_landmarks=L, seed=seed, times=times)
    gt = d["states_gt"]
    x0 = np.concatenate([gt[0, :3], gt[0, 7:10]])
    # pose k = pose 0 over time_idx[k] - time_idx[0] exact steps
    xs = X.propagate(np.repeat(x0[None], n, 0), times - times[0], stm=False).astype(np.float64)
    gt = gt.copy()
    gt[:, :3], gt[:, 7:10] = xs[:, :3], xs[:, 3:]
    d["states_gt"] = gt
    rng = np.random.default_rng(seed + 100)
    st = gt.copy()
    st[:, :3] += rng.normal(0, 2.0, (n, 3))
    dq = np.concatenate([rng.normal(0, 2e-3, (n, 3)), np.ones((n, 1))], 1)
    st[:, 3:7] = O.qmul(st[:, 3:7], dq / np.linalg.norm(dq, axis=1, keepdims=True))
    st[:, 7:10] += rng.normal(0, 2e-3, (n, 3))
    d["states0"] = st
    d["w"] = np.full(d["uv"].shape[0], 0.95)
    if name in EMPTY_POSE:
        keep = d["pose_of_row"] != EMPTY_POSE[name]
        for k in ("uv", "w", "pose_of_row", "landmark_of_row"):
            d[k] = d[k][keep]
    d["Xs"] = d["X0"] + rng.normal(0, 0.02, d["X0"].shape)
    d["time_idx"] = times.astype(np.int32)
    d["sigma_dyn"] = SIGMA_DYN
    return d


def args(d):
    """Arguments of the oracle's functions after (states, X), up to the damping."""
    return d["X0"], d["uv"], d["w"], d["pose_of_row"], d["landmark_of_row"], d["intrinsics"], d["sigma"]


def rel(a, b):
    """Largest difference relative to the largest entry of the reference ``b``."""
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


@functools.lru_cache(maxsize=None)
def reference(name, lam, sigma_dyn=None, full=False, fault=None):
    """One LM trial of ``case(name)`` by the oracle's Schur route, with the reduced matrix and its factor.  ``full``: also the
    disagreement with the refined full solve, relative to the largest entry -- the floor of this reference."""
    d = case(name)
    sd = d["sigma_dyn"] if sigma_dyn is None else sigma_dyn
    st, Xs, t = d["states0"], d["Xs"], d["time_idx"]
    n = st.shape[0]
    r = SimpleNamespace()
    r.c0 = D.cost(st, Xs, *args(d), t, sd)
    ne = D.normal_equations(st, Xs, *args(d), lam, t, sd, fault=fault)
    dc9, dl, r.Sm, r.Lc = D.step_schur(*ne)
    s1, X1 = D.apply_step(st, Xs, dc9, dl)
    r.c1 = D.cost(s1, X1, *args(d), t, sd)
    r.ok = r.c1 < r.c0
    r.st, r.X = (s1, X1) if r.ok else (st, Xs)
    r.s1, r.X1 = s1, X1
    r.dc, r.dv, r.dl = dc9[:6 * n].reshape(n, 6), dc9[6 * n:].reshape(n, 3), dl.reshape(-1, 3)
    if full:
        f9, fl = D.step_full(*ne)
        r.floor = dict(dc=rel(dc9[:6 * n], f9[:6 * n]), dv=rel(dc9[6 * n:], f9[6 * n:]), dl=rel(dl, fl))
    return r
