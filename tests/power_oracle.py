"""NumPy / SciPy restatement of the outlier power query (vba_outlier_power): from the oracle's debug dict of a full-phase call
(``Jg``, ``w``, ``r_obs``, ``bands``) and the dense marginals of tests/cov_oracle.py, the minimal detectable bias, the external
reliabilities and the deletion influence of every observation row, the per-pose summary and the window's fit record, by the
definitions of include/vinsat_ba.h.  Eigenvalues come from LAPACK (``numpy.linalg.eigvalsh``, ``scipy.linalg.eigh(M, R)``), not
from the closed forms of vinsat_amd/csrc/vba_power_math.h, which tests/test_outlier_power_host.py checks against them."""
import numpy as np
import scipy.linalg

import rel_oracle as R
from oracle import ba_oracle as O

NCP = 17.075


def mu_min_sym2(a, b, d):
    """Smaller eigenvalue of [a, b; b, d] by LAPACK (arrays broadcast)."""
    a, b, d = np.broadcast_arrays(np.asarray(a, float), np.asarray(b, float), np.asarray(d, float))
    A = np.stack([np.stack([a, b], -1), np.stack([b, d], -1)], -2)
    return np.linalg.eigvalsh(A)[..., 0]


def mu_max_pair(M, Rm):
    """Larger root of det(M - mu R) = 0 by ``scipy.linalg.eigh(M, R)``; NaN where LAPACK does not find R positive definite."""
    try:
        return float(scipy.linalg.eigh(M, Rm, eigvals_only=True)[-1])
    except (np.linalg.LinAlgError, ValueError):
        return float("nan")


def power(dbg, ii, lam32=0.0, ncp=NCP, crit=np.inf, method="inv"):
    """``dbg``: the debug dict of ``ba_iteration(..., initialize=False, debug=dbg)`` at the states in question; ``ii [m]``.
    Returns dict(mdb, ext_pos, ext_att, del_pos [m]; pose_fit [n,4]; fit [8]; leverage, wtest [m]; detR, mu_min [m])."""
    ii = np.asarray(ii, dtype=np.int64)
    rel = R.reliability(dbg, ii, lam32, method=method)
    Jg, w, r = dbg["Jg"], dbg["w"], dbg["r_obs"]
    m, n = w.size, dbg["bands"].shape[0]
    Rk = np.eye(2)[None] - rel["P"]
    B = w[:, None, None] * np.einsum("kab,krb->kar", rel["S"][ii], Jg)           # [m,6,2]
    detR = Rk[:, 0, 0] * Rk[:, 1, 1] - Rk[:, 0, 1] * Rk[:, 1, 0]
    mu = np.linalg.eigvalsh(Rk)[:, 0]
    mdb, ep, ea, dp = (np.full(m, np.nan) for _ in range(4))
    for k in range(m):
        if w[k] == 0.0:
            mdb[k], ep[k], ea[k], dp[k] = np.inf, 0.0, 0.0, 0.0
            continue
        if not (detR[k] > 0.0 and mu[k] > 0.0):
            continue
        Bp, Bt = B[k, :3], B[k, 3:]
        mdb[k] = np.sqrt(ncp / (w[k] * mu[k]))
        ep[k] = np.sqrt(ncp / w[k] * mu_max_pair(Bp.T @ Bp, Rk[k]))
        ea[k] = 2.0 * np.sqrt(ncp / w[k] * mu_max_pair(Bt.T @ Bt, Rk[k]))
        dp[k] = np.linalg.norm(Bp @ np.linalg.solve(Rk[k], r[k]))
    wt, lev = rel["wtest"], rel["leverage"]
    wr2 = w * (r ** 2).sum(1)
    pf = np.zeros((n, 4))
    for i in range(n):
        sel = ii == i
        if sel.any():
            e = ep[sel][np.isfinite(ep[sel])]
            pf[i] = wr2[sel].sum(), lev[sel].sum(), e.max() if e.size else 0.0, np.count_nonzero(wt[sel] > crit)
    m_eff = float(np.count_nonzero(w > 0))
    omega, t = wr2.sum(), lev.sum()
    rho = 2.0 * m_eff - t
    fin_t, fin_e = wt[np.isfinite(wt)], ep[np.isfinite(ep)]
    fit = np.array([omega, m_eff, t, rho, omega / rho if rho > 0 else np.nan, fin_t.max() if fin_t.size else 0.0,
                    float(np.count_nonzero(wt > crit)), fin_e.max() if fin_e.size else 0.0])
    return dict(mdb=mdb, ext_pos=ep, ext_att=ea, del_pos=dp, pose_fit=pf, fit=fit, leverage=lev, wtest=wt, detR=detR, mu_min=mu,
                S=rel["S"], P=rel["P"])


def at_states(win, st, lam, it=19, damped=False, ncp=NCP, crit=np.inf, method="inv", conf=None, **kw):
    """The reference values at states ``st`` of window ``win`` (od_pipe.prepare_window) for a full-phase call ``it``; ``conf``
    replaces the window's confidences; ``kw`` goes to the oracle (``prior=``, ``hop=``).  Also returns the debug dict."""
    d = {}
    O.ba_iteration(it, st, win.cumrot_last, win.landmarks_uv, win.landmarks_xyz, win.ii, win.time_idx, win.intrinsics,
                   win.confidences if conf is None else conf, lam, initialize=False, debug=d, **kw)
    return power(d, win.ii, float(np.float32(lam)) if damped else 0.0, ncp=ncp, crit=crit, method=method), d


def rel_err_finite(got, ref):
    """max |got - ref| over the entries where ``ref`` is finite, over the largest finite |ref| (tests/rel_oracle.py:
    ``row_rel_err``); the non-finite patterns (+inf of a row of weight zero, NaN of a degenerate row) must agree exactly."""
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    f = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isposinf(got), np.isposinf(ref))
    if not f.any():
        return 0.0
    den = np.abs(ref[f]).max()
    return float(np.abs(got[f] - ref[f]).max() / (den if den > 0 else 1.0))
