"""NumPy restatement of the rule of ``vba_schur_snoop`` (include/vinsat_ba.h; vinsat_amd/csrc/vba_schur_snoop_pick.h holds the
combine rule the device compiles).  Plain module, no tests; shared by tests/test_schur_snoop_host.py and
tests/test_gpu_schur_snoop.py.

Rows are in the CALLER's order.  "The smaller sorted row" of the rule is the row that comes first when rows are sorted by
(landmark, pose) as ``vinsat_amd.schur.build_structure`` sorts them: inside a landmark the smaller pose, inside a pose the smaller
landmark.  :func:`select` is written group by group, without any vectorised shortcut, so that it can be read against the rule.
"""
import numpy as np

MARGIN_FACTOR = 100.0           # a decided comparison is safe if its margin is 100 x the bar of the tests x the largest test


def crit_used(crit, scaled, s0sq, info=0):
    """``crit``, or ``crit * sqrt(s0sq)`` with ``scaled`` (NaN for a fit that does not exist: ``info != 0`` or ``s0sq`` NaN)."""
    if not scaled:
        return float(crit)
    if info != 0:
        return float("nan")
    with np.errstate(invalid="ignore"):
        return float(np.float64(crit) * np.sqrt(np.float64(s0sq)))


def _better(a_val, a_pos, b_val, b_pos):
    """Candidate a is rejected before candidate b: a NaN never wins, the larger value wins, ties go to the smaller position."""
    if np.isnan(a_val):
        return False
    if np.isnan(b_val):
        return True
    return a_val > b_val or (a_val == b_val and a_pos < b_pos)


def _best(cands):
    """The winner of a list of ``(value, position, tag)`` and the runner-up's value (None if there is none)."""
    win = None
    for c in cands:
        if win is None or _better(c[0], c[1], win[0], win[1]):
            win = c
    rest = [c[0] for c in cands if c is not win and not np.isnan(c[0])]
    return win, (max(rest) if rest else None)


def select(wtest, lm_wtest, s0sq, info, w, pose_of_row, landmark_of_row, n, L, crit, scaled=True, min_rows=6, min_track=3):
    """One call of the rule.  Returns a dict: ``rows`` [m] bool (rejected by their own test), ``landmarks`` [L] bool, ``via`` [m] bool
    (rows zeroed through a rejected landmark), ``counts`` (3 ints), ``crit_used``, ``marked`` [L] bool, ``short`` [n] bool, and
    ``margin``: the smallest margin of a decided comparison (winner against runner-up in a landmark's or a pose's group, every
    eligible test against ``c``), inf if nothing was compared."""
    wtest, lm_wtest, w = (np.asarray(a, dtype=np.float64) for a in (wtest, lm_wtest, w))
    pr, lr = np.asarray(pose_of_row, dtype=np.int64), np.asarray(landmark_of_row, dtype=np.int64)
    m = w.size
    rank = np.empty(m, dtype=np.int64)
    rank[np.lexsort((pr, lr))] = np.arange(m)
    c = crit_used(crit, scaled, s0sq, info)
    out = dict(rows=np.zeros(m, dtype=bool), landmarks=np.zeros(L, dtype=bool), via=np.zeros(m, dtype=bool), counts=(0, 0, 0), crit_used=c,
               marked=np.zeros(L, dtype=bool), short=np.zeros(n, dtype=bool), margin=float("inf"))
    if info != 0 or not np.isfinite(c):
        return out
    margin = float("inf")
    on = w > 0.0
    prior_pos = m                                                       # after every row: a row beats the prior on a tie
    rows_of_lm = [np.nonzero(lr == l)[0] for l in range(L)]
    rows_of_pose = [np.nonzero(pr == i)[0] for i in range(n)]
    proposed = np.full(L, -1, dtype=np.int64)
    # 1. per landmark
    for l in range(L):
        ks = rows_of_lm[l]
        cntl = int(on[ks].sum())
        cands = []
        for k in ks:
            if on[k] and np.isfinite(wtest[k]):
                margin = min(margin, abs(wtest[k] - c))
                if wtest[k] > c:
                    cands.append((wtest[k], int(rank[k]), int(k)))
        if cntl >= min_track and np.isfinite(lm_wtest[l]):
            margin = min(margin, abs(lm_wtest[l] - c))
            if lm_wtest[l] > c:
                cands.append((lm_wtest[l], prior_pos, -1))
        if not cands:
            continue
        win, second = _best(cands)
        if second is not None:
            margin = min(margin, win[0] - second)
        if win[2] < 0:
            out["marked"][l] = True
        else:
            proposed[l] = win[2]
    # 2. per pose
    for i in range(n):
        ks = rows_of_pose[i]
        cnt = int(on[ks].sum())
        c_lm = int((on[ks] & out["marked"][lr[ks]]).sum())
        left = cnt - c_lm
        out["short"][i] = left < min_rows
        cands = [(wtest[k], int(rank[k]), int(k)) for k in ks if proposed[lr[k]] == k]
        if not cands:
            continue
        win, second = _best(cands)
        if second is not None:
            margin = min(margin, win[0] - second)
        if not out["short"][i] and left - 1 >= min_rows:
            out["rows"][win[2]] = True
    # 3. per landmark
    for l in np.nonzero(out["marked"])[0]:
        ks = rows_of_lm[l][on[rows_of_lm[l]]]
        if not out["short"][pr[ks]].any():
            out["landmarks"][l] = True
            out["via"][ks] = True
    assert not (out["rows"] & out["via"]).any()                         # a landmark either marks or proposes
    out["counts"] = (int(out["rows"].sum()), int(out["landmarks"].sum()), int(out["via"].sum()))
    out["margin"] = margin
    return out


def select_from(rel, d, crit, scaled=True, min_rows=6, min_track=3, w=None):
    """:func:`select` on a dict of ``SchurBA.reliability`` (or any object with those keys) and a problem dict of tests/schur_cases.py;
    ``w`` overrides the problem's weights (rows already rejected)."""
    return select(rel["wtest"], rel["lm_wtest"], rel["fit"]["s0sq"], rel.get("info", 0), d["w"] if w is None else w, d["pose_of_row"],
                  d["landmark_of_row"], d["states0"].shape[0], d["X0"].shape[0], crit, scaled, min_rows, min_track)
