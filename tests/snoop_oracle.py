"""NumPy restatement of the selection rule of data snooping (vba_snoop, include/vinsat_ba.h) on top of tests/rel_oracle.py: from
the w-tests, the final weights and the pose index of the rows, the rows one call rejects.  ``ambiguous`` reports the poses whose
decision hangs on a comparison closer than a margin -- there the device (whose w-tests agree with the oracle's to a bar, not to
the bit) may rightly decide otherwise, and a test that compares masks must not use such a window."""
import copy

import numpy as np

import rel_oracle as R

# tests/test_gpu_reliability.py holds the device's wtest to this oracle within BAR = 1e-8 of the window's largest value; a
# comparison is called ambiguous at 100 times that
REL_BAR = 1e-8
MARGIN_FACTOR = 100.0


def margin_of(wtest):
    fin = wtest[np.isfinite(wtest)]
    return MARGIN_FACTOR * REL_BAR * (float(np.abs(fin).max()) if fin.size else 0.0)


def _poses(ii, n):
    order = np.argsort(ii, kind="stable")
    cuts = np.searchsorted(ii[order], np.arange(n + 1))
    return [order[cuts[i]:cuts[i + 1]] for i in range(n)]        # rows of pose i, ascending input index


def _candidates(wtest, w, rows, crit):
    with np.errstate(invalid="ignore"):
        return rows[(w[rows] > 0) & np.isfinite(wtest[rows]) & (wtest[rows] > crit)]


def select(wtest, w, ii, n, crit, mode=0, min_rows=6, barred=False):
    """The rows one vba_snoop call rejects: ``(mask [m] bool, per_pose [n] int)``.  ``barred``: the window's covariance step was
    flagged (zero pivot, non-finite, indefinite)."""
    ii = np.asarray(ii, dtype=np.int64)
    mask = np.zeros(ii.size, dtype=bool)
    per = np.zeros(n, dtype=np.int64)
    if barred:
        return mask, per
    for i, rows in enumerate(_poses(ii, n)):
        cand = _candidates(wtest, w, rows, crit)
        if cand.size == 0:
            continue
        cnt = int(np.count_nonzero(w[rows] != 0))
        if mode == 1 and cnt - cand.size >= min_rows:
            mask[cand] = True
            per[i] = cand.size
        elif cnt - 1 >= min_rows:
            mask[cand[np.argmax(wtest[cand])]] = True           # (the first maximum: the smallest input index)
            per[i] = 1
    return mask, per


def ambiguous(wtest, w, ii, n, crit, mode=0, min_rows=6, margin=None):
    """Poses whose decision hangs on a comparison closer than ``margin`` (default :func:`margin_of`): a weighted row's wtest
    against ``crit``; the best against the runner-up candidate where one row is chosen; in mode 1 the guard's count, which moves
    with a candidate within the margin of ``crit`` (the first comparison again).  Returns the list of pose indices."""
    ii = np.asarray(ii, dtype=np.int64)
    margin = margin_of(wtest) if margin is None else margin
    out = []
    for i, rows in enumerate(_poses(ii, n)):
        live = rows[(w[rows] > 0) & np.isfinite(wtest[rows])]
        if np.isfinite(crit) and (np.abs(wtest[live] - crit) <= margin).any():
            out.append(i)
            continue
        cand = _candidates(wtest, w, rows, crit)
        cnt = int(np.count_nonzero(w[rows] != 0))
        picks_one = cand.size >= 2 and not (mode == 1 and cnt - cand.size >= min_rows) and cnt - 1 >= min_rows
        if picks_one:
            top = np.sort(wtest[cand])[-2:]
            if top[1] - top[0] <= margin:
                out.append(i)
    return out


def with_conf(win, conf):
    """``win`` with other confidences (a shallow copy: the window itself is shared among tests and stays as it is)."""
    w2 = copy.copy(win)
    w2.confidences = np.ascontiguousarray(conf, dtype=np.float64)
    return w2


def at_states(win, st, lam, it=19, damped=False, conf=None, **kw):
    """``rel_oracle.at_states`` with the confidences ``conf`` (default: the window's): ``(wtest, w)`` in input order."""
    ref, dbg = R.at_states(win if conf is None else with_conf(win, conf), st, lam, it=it, damped=damped, **kw)
    return ref["wtest"], dbg["w"]
