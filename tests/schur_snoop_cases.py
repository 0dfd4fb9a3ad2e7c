"""The planted window of the free-landmark snooping tests (plain module, no tests; tests/test_schur_snoop_host.py vets it with the
oracle alone, tests/test_gpu_schur_snoop.py runs it on the device).

Problem "43" of tests/schur_rel_cases.py (43 poses / 450 landmarks, two panels) with ``N_ROWS`` detections moved by ``PLANT_PX``
pixels in both coordinates (one per landmark, seeded choice among the rows of tracks of at least 4) and the catalogue entries of
``N_LANDMARKS`` other landmarks (tracks of at least 4) displaced by ``DISPLACE_SIGMAS`` sigma; the state starts at the displaced
catalogue.  :func:`oracle_loop` is ``SchurBA.solve(snoop=SNOOP)`` by the oracle: converge, one call of the rule, converge again
from where it stands, until a round rejects nothing.
"""
import functools

import numpy as np

import schur_cases as C
import schur_rel_cases as R
import schur_snoop_oracle as SO
from oracle import schur_oracle as S

SEED, N_ROWS, N_LANDMARKS = 7, 100, 5
# (lamda: a landmark whose rows are all rejected has P_l = I exactly at lamda = 0 -- the reference's LAPACK inverse of I - P_l then
# raises where the device writes NaN; a damping far below 1 / sigma^2 = 400 keeps the reference defined and changes no decision)
# (rows, landmarks, rows through landmarks) per round as the oracle loop gives them (tests/test_schur_snoop_host.py asserts it)
EXPECTED_ROUNDS = ((39, 0, 0), (31, 0, 0), (13, 0, 0), (11, 0, 0), (6, 0, 0), (0, 5, 63), (0, 0, 0))
SNOOP = dict(lamda=1e-3, crit=5.5, scaled=True, min_rows=6, min_track=3, rounds=8)


@functools.lru_cache(maxsize=None)
def planted():
    d = dict(R.problem("43"))
    rng = np.random.default_rng(SEED)
    L = d["X0"].shape[0]
    track = np.bincount(d["landmark_of_row"], minlength=L)
    long_lms = np.nonzero(track >= 4)[0]
    lms = np.sort(rng.choice(long_lms, N_LANDMARKS, replace=False))
    hosts = rng.choice(np.setdiff1d(long_lms, lms), N_ROWS, replace=False)              # one planted row per landmark
    rows = np.sort(np.array([int(rng.choice(np.nonzero(d["landmark_of_row"] == l)[0])) for l in hosts]))
    uv = d["uv"].copy()
    uv[rows] += R.PLANT_PX
    X0 = d["X0"].copy()
    X0[lms] += R.DISPLACE_SIGMAS * d["sigma"] / np.sqrt(3.0) * np.array([1.0, -1.0, 1.0])
    d["uv"], d["X0"], d["Xs"], d["planted_rows"], d["displaced_lms"] = uv, X0, X0, rows, lms
    return d


def lm_loop(d, w, st, X, lamda0=1e-4, max_iters=20, tol=1e-10):
    """The LM loop of ``SchurBA.solve`` by the oracle from the state ``(st, X)`` with the weights ``w``."""
    args = (d["X0"], d["uv"], w, d["pose_of_row"], d["landmark_of_row"], d["intrinsics"], d["sigma"])
    lam = lamda0
    for _ in range(max_iters):
        c0, c1, ok, st, X, _, _ = S.lm_trial(st, X, *args, lam)
        if ok:
            lam = max(lam * 0.1, 1e-9)
            if c0 - c1 <= tol * max(c0, 1e-300):
                break
        else:
            lam *= 10.0
            if lam > 1e8:
                break
    return st, X


def position_error(d, st):
    """Mean pose position error against the generating states, km."""
    return float(np.linalg.norm(st[:, :3] - d["states_gt"][:, :3], axis=1).mean())


@functools.lru_cache(maxsize=None)
def oracle_loop():
    """``rounds``: per round the dict of ``schur_snoop_oracle.select`` plus ``bar`` (100 x the larger of the wtest / lm_wtest bars of
    ``schur_rel_cases.bar`` x the largest test of the window) and the state it ran at; ``rows`` / ``landmarks``: everything rejected;
    ``err_before`` / ``err_after``: mean position error after the first solve and at the end."""
    d = planted()
    opts = dict(SNOOP)
    rounds_max, lamda = opts.pop("rounds"), opts.pop("lamda")
    w = d["w"].copy()
    st, X = lm_loop(d, w, d["states0"], d["Xs"])
    out = dict(rounds=[], rows=np.zeros(w.size, dtype=bool), landmarks=np.zeros(d["X0"].shape[0], dtype=bool), err_before=position_error(d, st))
    for _ in range(rounds_max):
        dd = dict(d)
        dd["w"] = w
        r = R.evaluate(dd, st, X, lamda)
        sel = SO.select(r.wtest, r.lm_wtest, r.fit["s0sq"], 0, w, d["pose_of_row"], d["landmark_of_row"], st.shape[0], X.shape[0], **opts)
        fin = lambda a: float(np.max(a[np.isfinite(a)], initial=0.0))
        sel["bar"] = SO.MARGIN_FACTOR * max(R.bar(r, "wtest"), R.bar(r, "lm_wtest")) * max(fin(r.wtest), fin(r.lm_wtest))
        sel["state"], sel["s0sq"] = (st, X), r.fit["s0sq"]
        out["rounds"].append(sel)
        if sel["counts"][0] + sel["counts"][1] == 0:
            break
        out["rows"] |= sel["rows"]
        out["landmarks"] |= sel["landmarks"]
        w = np.where(sel["rows"] | sel["via"], 0.0, w)
        st, X = lm_loop(d, w, st, X)
    out["err_after"], out["w"], out["state"] = position_error(d, st), w, (st, X)
    return out
