"""NumPy restatement of the reliability query (vba_reliability): from the oracle's debug dict of a full-phase call (``Jg``, ``w``,
``r_obs``, ``bands``) and the dense marginals of tests/cov_oracle.py, the leverage and the standardised residual (w-test) of every
observation row and the per-pose summary, by the formulas of include/vinsat_ba.h."""
import numpy as np

import cov_oracle as C
from oracle import ba_oracle as O


def row_projectors(Jg, w, S):
    """P_k = w_k J_k S_k J_k^T [m,2,2], symmetric part; S [m,6,6] the row's pose block."""
    P = np.einsum("k,kra,kab,ksb->krs", w, Jg, S, Jg)
    return 0.5 * (P + P.transpose(0, 2, 1))


def reliability(dbg, ii, lam32=0.0, method="inv"):
    """``dbg``: the debug dict of ``ba_iteration(..., initialize=False, debug=dbg)`` at the states in question; ``ii [m]``.
    Returns dict(leverage [m], wtest [m], pose_stats [n,3], P [m,2,2], S [n,6,6])."""
    ii = np.asarray(ii, dtype=np.int64)
    Jg, w, r = dbg["Jg"], dbg["w"], dbg["r_obs"]
    n = dbg["bands"].shape[0]
    S = C.marginal_dense(dbg["bands"], lam32, method=method)[0][:, :6, :6]
    P = row_projectors(Jg, w, S[ii])
    lev = P[:, 0, 0] + P[:, 1, 1]
    M = np.eye(2)[None] - P
    det = M[:, 0, 0] * M[:, 1, 1] - M[:, 0, 1] * M[:, 1, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (r[:, 0] ** 2 * M[:, 1, 1] - 2.0 * r[:, 0] * r[:, 1] * M[:, 0, 1] + r[:, 1] ** 2 * M[:, 0, 0]) / det
        t = np.sqrt(w * q)
    t = np.where((det > 0) & (w * q >= 0), t, np.nan)
    lev = np.where(w == 0, 0.0, lev)
    t = np.where(w == 0, 0.0, t)
    ps = np.zeros((n, 3))
    for i in range(n):
        sel = ii == i
        if sel.any():
            fin = t[sel][np.isfinite(t[sel])]
            ps[i] = lev[sel].sum(), fin.max() if fin.size else 0.0, np.count_nonzero(w[sel] > 0)
    return dict(leverage=lev, wtest=t, pose_stats=ps, P=P, S=S)


def at_states(win, st, lam, it=19, damped=False, method="inv", **kw):
    """The reference values at states ``st`` of window ``win`` (od_pipe.prepare_window) for a full-phase call ``it``; ``kw`` goes to
    the oracle (``prior=``, ``hop=``).  Also returns the debug dict."""
    d = {}
    O.ba_iteration(it, st, win.cumrot_last, win.landmarks_uv, win.landmarks_xyz, win.ii, win.time_idx, win.intrinsics,
                   win.confidences, lam, initialize=False, debug=d, **kw)
    return reliability(d, win.ii, float(np.float32(lam)) if damped else 0.0, method=method), d


def row_rel_err(got, ref):
    """max |got - ref| over the rows, normalised by the window's largest |ref| (a near-zero row cannot dominate)."""
    return float(np.abs(got - ref).max() / np.abs(ref).max())
