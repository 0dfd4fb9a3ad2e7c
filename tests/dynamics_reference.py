"""Judging the part of a BA call between the accumulation and the solve in extended precision (no GPU needed): the orbit-dynamics
factor with its transition matrix (A4), the attitude Newton term (A5), the block-tridiagonal assembly (A6), the landmark-only step
that replaces assembly and solve, and the residual sums of the accept test.

Everything is a restatement in ``np.longdouble`` of the formulas of oracle/ba_oracle.py (``propagate_orbit``, ``orbit_factor``,
``attitude_factor``, ``assemble``, ``prior_factor``, ``retract``, the two means of ``ba_iteration``) from arrays the caller passes in;
the one-second RK4 chain is tests/exact_orbit.py's, the hop integrator (``propagate_orbit(hop=True)``: hops of at most 100 s) is
restated here on top of its step.

Two layers, as tests/accumulate_reference.py:

  factor layer     Phi, x_hat, r_orbit, f, qgrad, Hd, Hu, Hl against the STATES they were formed at;
  assembly layer   bands, rhs, last_hessian, the landmark-only step, its retraction and the residual sums against the FACTOR (and the
                   per-pose sums, rows) the judged side itself reports -- the factor's error does not loosen an assembly bar.

The measure is componentwise: every entry's error over the sum of the absolute values of the terms that form it, so a wrong entry
cannot hide behind a larger one of the same array.  The denominators come from the same restatement run on absolute values (every
structural sign +, every difference a sum).  An entry whose denominator is 0 (the off-diagonal attitude block of an end pose, a
velocity row of a landmark-only system, an off-diagonal block of a landmark-only call) must be exactly 0: reported apart (``exact``).
For Phi and x_hat the measure is the per-edge one of tests/test_gpu_long_gaps.py (``exact_orbit.edge_errors``: position and
velocity of x_hat over their own maximum, position and velocity columns of Phi over theirs), with x_hat = x_next + r_orbit / D.

Every figure is an array whose first axis is the pose (the edge for the factor's orbit part), so ``judge`` names pose and entry.
A figure passes at K x 2^-53 with K = max(16, 4 x the figure of the fp64 NumPy oracle on the same case) -- the rule and the
reasons of tests/accumulate_reference.py; ``oracle_levels`` measures the oracle.  No bar comes from a device run.

The long edges (more than 64 steps) belong to the kernels of vba_long.hip and to tests/test_gpu_long_gaps.py: ``factor_layer``
leaves their Phi / x_hat / r_orbit out (``skip``), the assembly layer and the sums take what the device reports for them like any
other edge."""
from dataclasses import dataclass, field

import numpy as np

import exact_orbit as X
from oracle import ba_oracle as O

LD = np.longdouble
U = 2.0 ** -53
K_FLOOR, K_FACTOR, K_CASE_MAX = 16.0, 4.0, 1024.0
D6 = np.array([1.0, 1.0, 1.0, O.VEL_COEFF, O.VEL_COEFF, O.VEL_COEFF])
KQ = LD(O.QUAT_COEFF)
LONG_GAP = 64                   # kLongGap: edges of more steps are vba_long.hip's


def _ld(a):
    return np.asarray(a).astype(LD)


# ------------------------------------------------------------------------------------------------ orbit factor
def propagate_hop(x, steps):
    """``O.propagate_orbit(hop=True)`` in longdouble: floor(d / 100) steps of 100 s, then one of d % 100 s (none if that is 0)."""
    x = np.array(x, dtype=LD).reshape(-1, 6)
    steps = np.asarray(steps, dtype=np.int64).reshape(-1)
    n = x.shape[0]
    Phi = np.broadcast_to(np.eye(6, dtype=LD), (n, 6, 6)).copy()
    hops = steps // 100
    for s in range(int(hops.max()) + 1 if n else 0):
        h = np.where(hops == s, steps % 100, np.where(hops > s, 100, 0))
        for hv in np.unique(h[h > 0]):
            act = h == hv
            x[act], Phi[act] = X.rk4_step_stm(x[act], Phi[act], int(hv))
    return x, Phi


def orbit_ld(states, time_idx, hop=False):
    """(x [n, 6], x_hat [n - 1, 6], Phi [n - 1, 6, 6]) of the edges in longdouble: the last pose's propagation is discarded
    (BA_utils.py:476), so there are n - 1 of each."""
    st = np.asarray(states, dtype=np.float64)
    x = np.concatenate([st[:, :3], st[:, 7:10]], -1)
    steps = O.step_counts(time_idx)[:-1]
    xh, Phi = (propagate_hop if hop else X.propagate)(x[:-1], steps)
    return _ld(x), xh, Phi


# ------------------------------------------------------------------------------------------------ attitude term
def _qmul(a, b):
    x1, y1, z1, w1 = np.moveaxis(a, -1, 0)
    x2, y2, z2, w2 = np.moveaxis(b, -1, 0)
    return np.stack([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                     w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2], -1)


def _qmul_abs(a, b):
    a, b = np.abs(a), np.abs(b)
    x1, y1, z1, w1 = np.moveaxis(a, -1, 0)
    x2, y2, z2, w2 = np.moveaxis(b, -1, 0)
    return np.stack([w1 * x2 + x1 * w2 + y1 * z2 + z1 * y2, w1 * y2 + x1 * z2 + y1 * w2 + z1 * x2,
                     w1 * z2 + x1 * y2 + y1 * x2 + z1 * w2, w1 * w2 + x1 * x2 + y1 * y2 + z1 * z2], -1)


@dataclass
class Attitude:
    f: np.ndarray               # [n - 1]
    qgrad: np.ndarray           # [n, 3]
    Hd: np.ndarray              # [n, 3, 3]
    Hu: np.ndarray              # [n, 3, 3] block (i, i + 1); zeros for the last pose
    Hl: np.ndarray              # [n, 3, 3] block (i, i - 1); zeros for the first pose


def attitude_ld(states, cumrot, absolute=False):
    """``O.attitude_factor`` widened, the end poses included (Hu of the last and Hl of the first pose are zeros).  ``absolute``:
    the same sums over the absolute values of their terms (the sign s taken as 1, 1 - |d| as 1 + |d|): the denominators."""
    q, c = _ld(np.asarray(states)[:, 3:7]), _ld(cumrot)
    n = q.shape[0]
    G = O.attitude_jacobian(q)
    Rm = O.right_mult_matrix(c)
    if absolute:
        G, Rm, q = np.abs(G), np.abs(Rm), np.abs(q)
        d = (_qmul_abs(q, c)[:-1] * q[1:]).sum(-1)
        s = np.ones(n - 1, dtype=LD)
        f = KQ * (1 + d)
    else:
        d = (_qmul(q, c)[:-1] * q[1:]).sum(-1)
        s = -np.sign(d)
        f = KQ * (1 - np.abs(d))
    grad = np.zeros((n, 4), dtype=LD)
    grad[:-1] += KQ * s[:, None] * np.einsum("iba,ib->ia", Rm[:-1], q[1:])
    grad[1:] += KQ * s[:, None] * np.einsum("iab,ib->ia", Rm[:-1], q[:-1])
    qgrad = np.einsum("ika,ik->ia", G, grad)
    g0, g1, g2, g3 = grad[:, 0], grad[:, 1], grad[:, 2], grad[:, 3]
    sg = 1 if absolute else -1
    B = np.stack([np.stack([sg * g3, sg * g2, g1, g0], -1), np.stack([g2, sg * g3, sg * g0, g1], -1),
                  np.stack([sg * g1, g0, sg * g3, g2], -1)], -2)
    Hd = B @ G
    Hu, Hl = np.zeros((n, 3, 3), dtype=LD), np.zeros((n, 3, 3), dtype=LD)
    Hu[:-1] = KQ * s[:, None, None] * np.einsum("ika,ilk,ilb->iab", G[:-1], Rm[:-1], G[1:])
    Hl[1:] = KQ * s[:, None, None] * np.einsum("ika,ikl,ilb->iab", G[1:], Rm[:-1], G[:-1])
    return Attitude(f, qgrad, Hd, Hu, Hl)


def _ratio(err, den, name, exact):
    """err / den entry by entry (0 where den == 0; such an entry must have err == 0: noted in ``exact``)."""
    err, den = np.asarray(err, dtype=LD), np.asarray(den, dtype=LD)
    z = den == 0
    out = np.zeros(err.shape, dtype=np.float64)
    np.divide(err, den, out=out, where=~z, casting="unsafe")
    out[~np.isfinite(out)] = np.inf
    if z.any() and (err[z] != 0).any():
        k = np.unravel_index(int(np.argmax(np.where(z, err, 0))), err.shape)
        exact.append(f"{name}: entry {tuple(int(v) for v in k)} is {float(err[k]):.3e} off where nothing is summed")
    return out


def factor_layer(states, time_idx, cumrot, Phi, r_pred, qgrad, Hq, hop=False):
    """Figures of a factor ``Phi`` [n, 6, 6] (row n - 1 ignored), ``r_pred`` [n - 1, 7], ``qgrad`` [n, 3], ``Hq`` [n, 3, 3, 3] =
    (Hl, Hd, Hu) against the longdouble factor at ``states``: (dict name -> array [poses or edges, ...], exact)."""
    st = np.asarray(states, dtype=np.float64)
    n = st.shape[0]
    Phi, r_pred, qgrad, Hq = (np.asarray(a, dtype=np.float64) for a in (Phi, r_pred, qgrad, Hq))
    x, xh, Pe = orbit_ld(st, time_idx, hop)
    steps = O.step_counts(time_idx)[:-1]
    short = (steps <= LONG_GAP) | bool(hop)
    exact, figs = [], {}
    xh_dev = x[1:] + _ld(r_pred[:, :6]) / _ld(D6)
    e = X.edge_errors(xh_dev, Phi[:-1], xh, Pe)
    for name, v in zip(("xhat_p", "xhat_v", "Phi_p", "Phi_v"), e):
        figs[name] = np.where(short, v, 0.0)
    r_ref = (xh - x[1:]) * _ld(D6)
    # the terms behind an entry of r_orbit: the start state, the increments of the steps (the gap times the derivative, taken as
    # the mean of its absolute value at both ends of the edge) and the next state -- where a coordinate passes through zero the
    # increments are what its rounding is relative to, not the coordinate
    inc = _ld(steps)[:, None] * (np.abs(X._deriv(x[:-1])) + np.abs(X._deriv(xh))) / 2
    fr = _ratio(np.abs(_ld(r_pred[:, :6]) - r_ref), (np.abs(x[:-1]) + inc + np.abs(x[1:])) * _ld(D6), "r_orbit", exact)
    figs["r_orbit"] = np.where(short[:, None], fr, 0.0)
    a, d = attitude_ld(st, cumrot), attitude_ld(st, cumrot, absolute=True)
    figs["f"] = _ratio(np.abs(_ld(r_pred[:, 6]) - a.f), d.f, "f", exact)
    figs["qgrad"] = _ratio(np.abs(_ld(qgrad) - a.qgrad), d.qgrad, "qgrad", exact)
    for k, name in enumerate(("Hl", "Hd", "Hu")):
        figs[name] = _ratio(np.abs(_ld(Hq[:, k]) - getattr(a, name)), getattr(d, name), name, exact)
    if not all(np.isfinite(v).all() for v in (Phi[:-1][short], r_pred, qgrad, Hq)):
        exact.append("non-finite factor")
    return figs, exact


# ------------------------------------------------------------------------------------------------ assembly
def prior_ld(states, prior, absolute=False):
    """(r [n, 6], Jp [n, 6, 9]) of ``O.prior_factor`` (vel_coeff = 1) in longdouble."""
    sp, Hs = _ld(prior[0]), _ld(prior[1]).reshape(-1, 6, 6)
    st = _ld(states)
    d = np.concatenate([sp[:, :3] - st[:, :3], sp[:, 7:] - st[:, 7:]], -1)
    n = st.shape[0]
    Jp = np.zeros((n, 6, 9), dtype=LD)
    if absolute:
        Hs, d = np.abs(Hs), np.abs(d)
        Jp[:, :, 0:3], Jp[:, :, 6:9] = Hs[:, :, :3], Hs[:, :, 3:]
    else:
        Jp[:, :, 0:3], Jp[:, :, 6:9] = -Hs[:, :, :3], -Hs[:, :, 3:]
    return np.einsum("iab,ib->ia", Hs, d), Jp


def assemble_ld(H, b, sigma, Phi, r_pred, qgrad, Hq, initialize, prior=None, states=None, absolute=False):
    """``O.assemble`` (w_max scale 1: ``H``, ``b`` are the normalised sums a fetch hands out) and the prior terms of
    ``ba_iteration`` in longdouble: (bands [n, 3, 9, 9], rhs [n, 9]).  The last pose has no edge: ``Phi[n - 1]`` is never read.
    ``absolute``: the sums of the absolute values of the terms."""
    conv = (lambda a: np.abs(_ld(a))) if absolute else _ld
    H, b = conv(H), conv(b)
    n = H.shape[0]
    bands = np.zeros((n, 3, 9, 9), dtype=LD)
    rhs = np.zeros((n, 9), dtype=LD)
    bands[:, 1, :6, :6] = H
    rhs[:, :6] = b
    sg = 1 if absolute else -1
    if not initialize:
        Phi, r_orb, qgrad, Hq = conv(Phi), conv(np.asarray(r_pred)[:, :6]), conv(qgrad), conv(Hq)
        sigma = LD(sigma)
        D = _ld(D6)
        E = np.zeros((n - 1, 6, 9), dtype=LD)
        DPhi = D[None, :, None] * Phi[:-1]
        E[:, :, 0:3], E[:, :, 6:9] = DPhi[:, :, 0:3], DPhi[:, :, 3:6]
        F = np.zeros((6, 9), dtype=LD)
        F[0:3, 0:3] = sg * np.eye(3, dtype=LD)
        F[3:6, 6:9] = sg * LD(O.VEL_COEFF) * np.eye(3, dtype=LD)
        bands[:-1, 1] += np.einsum("irc,ird->icd", E * sigma, E)
        bands[1:, 1] += (F * sigma).T @ F
        bands[:-1, 2] += np.einsum("irc,rd->icd", E * sigma, F)
        bands[1:, 0] += np.einsum("rc,ird->icd", F * sigma, E)
        rhs[:-1] += sg * np.einsum("irc,ir->ic", E * sigma, r_orb)
        rhs[1:] += sg * np.einsum("rc,ir->ic", F * sigma, r_orb)
        bands[:, 1, 3:6, 3:6] += sigma * Hq[:, 1]
        bands[:-1, 2, 3:6, 3:6] += sigma * Hq[:-1, 2]
        bands[1:, 0, 3:6, 3:6] += sigma * Hq[1:, 0]
        rhs[:, 3:6] += sg * sigma * qgrad
        if prior is not None:
            rp, Jp = prior_ld(states, prior, absolute)
            bands[:, 1] += np.einsum("irc,ird->icd", Jp, Jp)
            rhs += sg * np.einsum("irc,ir->ic", Jp, rp)
    return bands, rhs


def assembly_layer(bands, rhs, last_hessian, lam32, H, b, sigma, Phi, r_pred, qgrad, Hq, initialize, prior=None, states=None):
    """Figures of ``bands`` [n, 3, 9, 9], ``rhs`` [n, 9] and ``last_hessian`` [9, 9] (the last pose's DAMPED diagonal block) against
    the longdouble assembly of the factor given: (dict, exact)."""
    ref = assemble_ld(H, b, sigma, Phi, r_pred, qgrad, Hq, initialize, prior, states)
    den = assemble_ld(H, b, sigma, Phi, r_pred, qgrad, Hq, initialize, prior, states, absolute=True)
    exact, figs = [], {}
    bands, rhs = np.asarray(bands, dtype=np.float64), np.asarray(rhs, dtype=np.float64)
    figs["bands"] = _ratio(np.abs(_ld(bands) - ref[0]), den[0], "bands", exact)
    figs["rhs"] = _ratio(np.abs(_ld(rhs) - ref[1]), den[1], "rhs", exact)
    if last_hessian is not None:
        lh_ref = ref[0][-1, 1] + LD(lam32) * np.eye(9, dtype=LD)
        lh_den = den[0][-1, 1] + LD(lam32) * np.eye(9, dtype=LD)
        figs["last_hessian"] = _ratio(np.abs(_ld(last_hessian) - lh_ref), lh_den, "last_hessian", exact)[None]
    if not (np.isfinite(bands).all() and np.isfinite(rhs).all()):
        exact.append("non-finite system")
    return figs, exact


# ------------------------------------------------------------------------------------------------ landmark-only step
def _solve_ld(A, B, pivot=True):
    """A^-1 B for a batch A [n, k, k], B [n, k, r] in the dtype given (longdouble for the reference): Gauss-Jordan elimination,
    with partial pivoting unless ``pivot`` is off."""
    A, B = A.copy(), B.copy()
    n, k = A.shape[:2]
    rows = np.arange(n)
    for c in range(k):
        p = c + np.argmax(np.abs(A[:, c:, c]), axis=1) if pivot else np.full(n, c)
        for M in (A, B):
            tmp = M[rows, p].copy()
            M[rows, p] = M[:, c]
            M[:, c] = tmp
        piv = A[:, c, c][:, None]
        B[:, c] = B[:, c] / piv
        A[:, c] = A[:, c] / piv
        for r in range(k):
            if r != c:
                f = A[:, r, c][:, None].copy()
                A[:, r] -= f * A[:, c]
                B[:, r] -= f * B[:, c]
    return B


def retract_ld(states, dpose, absolute=False):
    """``O.retract`` in longdouble (``absolute``: the sums of absolute values behind every entry)."""
    st, dp = _ld(states), _ld(dpose)
    th = np.sqrt((dp[:, 3:6] ** 2).sum(-1))[:, None]
    small = th < LD(1e-16)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.concatenate([dp[:, 3:6] * np.sin(th / 2) / (th + LD(1e-16)), np.cos(th / 2)], -1)
    e = np.where(small, np.concatenate([np.zeros_like(dp[:, 3:6]), np.ones_like(th)], -1), e)
    if absolute:
        rot = _qmul_abs(st[:, 3:7], e)
        rot = rot / np.sqrt((_qmul(st[:, 3:7], e) ** 2).sum(-1, keepdims=True))
        return np.concatenate([np.abs(st[:, :3]) + np.abs(dp[:, :3]), rot, np.abs(st[:, 7:]) + np.abs(dp[:, 6:])], -1)
    rot = _qmul(st[:, 3:7], e)
    rot = rot / np.sqrt((rot ** 2).sum(-1, keepdims=True))
    return np.concatenate([st[:, :3] + dp[:, :3], rot, st[:, 7:] + dp[:, 6:]], -1)


def landmark_step_ld(H, b, lam32):
    """Per pose the solution of (H_i + lam32 I) x = b_i (``H``, ``b`` normalised by w_max as fetched), velocity rows zero: [n, 9]."""
    H, b = _ld(H), _ld(b)
    n = H.shape[0]
    A = H + LD(lam32) * np.eye(6, dtype=LD)
    x = np.zeros((n, 9), dtype=LD)
    x[:, :6] = _solve_ld(A, b[:, :, None])[:, :, 0]
    return x


def step_layer(dpose, states_new, H, b, lam32, states):
    """Figures of a landmark-only step ``dpose`` [n, 9] and trial state ``states_new`` [n, 10] from the sums ``H``, ``b`` given:
      step_fwd  |x - x*|_k / (|A^-1| (|A| |x*| + |b|))_k against the longdouble solution x* of A = H_i + lam32 I: what a componentwise
                backward error of one unit moves entry k by, to first order (Skeel), so the condition of a pose's block is in the
                measure, not in the bar.  (The componentwise backward error itself is no figure here: Gauss-Jordan elimination is
                not componentwise backward stable -- the same elimination with its operations in another order gives 5.6 and 25
                units on the first landmark-only call of c2 -- while the forward figure stays near 1 for every order tried.)
      retract   the trial state against the longdouble retraction of ``states`` by ``dpose`` itself.
    The velocity rows of the step must be exactly 0."""
    H, b, x = _ld(H), _ld(b), _ld(dpose)
    n = H.shape[0]
    A = H + LD(lam32) * np.eye(6, dtype=LD)
    exact, figs = [], {}
    xs = landmark_step_ld(H, b, lam32)
    Ainv = _solve_ld(A, np.broadcast_to(np.eye(6, dtype=LD), (n, 6, 6)).copy())
    scale = np.einsum("iab,ib->ia", np.abs(Ainv), np.einsum("iab,ib->ia", np.abs(A), np.abs(xs[:, :6])) + np.abs(b))
    figs["step_fwd"] = _ratio(np.abs(x[:, :6] - xs[:, :6]), scale, "step_fwd", exact)
    if (np.asarray(dpose)[:, 6:] != 0).any():
        exact.append(f"step: velocity rows of pose {int(np.argmax((np.asarray(dpose)[:, 6:] != 0).any(1)))} are not zero")
    figs["retract"] = _ratio(np.abs(_ld(states_new) - retract_ld(states, dpose)), retract_ld(states, dpose, absolute=True), "retract", exact)
    if not np.isfinite(np.asarray(dpose, dtype=np.float64)).all():
        exact.append("non-finite step")
    return figs, exact


# ------------------------------------------------------------------------------------------------ residual sums
def residual_sums_ld(uv, est, weight, r_pred, sigma, n, initialize, prior_r=None, trial=False, prior_den=None):
    """The mean of the accept test (vba_decide.h decide_finish; ``ba_iteration``: init_residual, residual) in longdouble, and
    the mean of the absolute values of the terms behind it: (value, den).

    ``trial`` False: mean |[uv - est ; sqrt(sigma) r_pred ; r_prior, 1 per pose]| with UNweighted rows (BA_filtering.py:51);
    True: the rows weighted by ``weight``, the attitude residual over 100 under BA_reg and 100 per pose for the prior's constant
    (:172-180).  Landmark-only calls have no dynamics terms but count 6 zeros per edge (and per pose under BA_reg).  ``r_pred`` [n - 1, 7] holds
    exactly the edges that count; ``prior_r`` [n, 6] switches BA_reg on (``prior_den``: sum of |terms| of each of its entries).
    A row's term is |fl(uv - est)|, the one fp64 subtraction both the kernels and the oracle make; its denominator is the same
    for the initial mean (the sum is judged against the rows given) and |uv| + |est| where ``trial`` (the rows come from another
    kernel than the sum)."""
    reg = prior_r is not None
    r = np.abs(_ld(np.asarray(uv, dtype=np.float64) - np.asarray(est, dtype=np.float64)))
    m = r.shape[0]
    if trial:
        w = _ld(weight)[:, None]
        so, so_den = (r * w).sum(), ((np.abs(_ld(uv)) + np.abs(_ld(est))) * w).sum()
    else:
        so = so_den = r.sum()
    per = 6 if initialize else 7
    denom = LD(2 * m + per * (n - 1) + (per * n if reg else 0))
    tot, den = so, so_den
    if not initialize:
        rp = np.abs(_ld(r_pred)).copy()
        if trial and reg:
            rp[:, 6] = rp[:, 6] / KQ
        sp = np.sqrt(LD(sigma)) * rp.sum()
        tot, den = tot + sp, den + sp
        if reg:
            c = LD(100 * n if trial else n)
            tot = tot + np.abs(_ld(prior_r)).sum() + c
            den = den + (np.abs(_ld(prior_r)) if prior_den is None else _ld(prior_den)).sum() + c
    return tot / denom, den / denom


def sums_figure(value, ref, den):
    return np.array([float(abs(LD(value) - ref) / den)])


def pred_shares(r_pred, sigma, total_sum):
    """Per edge, sqrt(sigma) sum |r_pred_i| over the whole sum of the initial mean: what dropping that edge moves the mean by."""
    return (np.sqrt(float(sigma)) * np.abs(np.asarray(r_pred, dtype=np.float64)).sum(-1)) / float(total_sum)


# ------------------------------------------------------------------------------------------------ bars
@dataclass
class Levels:
    units: dict                 # name -> the oracle's largest figure in units of 2^-53
    oracle: dict = field(repr=False, default=None)

    def K(self, name):
        return max(K_FLOOR, K_FACTOR * self.units[name])


def _units(figs):
    return {k: (float(np.max(v)) / U if np.size(v) else 0.0) for k, v in figs.items()}


def oracle_factor(states, time_idx, cumrot, hop=False):
    """The fp64 NumPy oracle's factor as the arrays a device fetch hands out: dict(Phi [n, 6, 6], r_pred, qgrad, Hq)."""
    st = np.asarray(states, dtype=np.float64)
    n = st.shape[0]
    r, E, _F = O.orbit_factor(st, time_idx, jacobian=True, hop=hop)
    f, qg, Hd, Hu, Hl = O.attitude_factor(st, cumrot, jacobian=True)
    x = np.concatenate([st[:, :3], st[:, 7:10]], -1)
    _xh, Phi = O.propagate_orbit(x, O.step_counts(time_idx), stm=True, hop=hop)
    Phi[-1] = 0.0
    Hq = np.zeros((n, 3, 3, 3))
    Hq[:, 1], Hq[:-1, 2], Hq[1:, 0] = Hd, Hu, Hl
    return dict(Phi=Phi, r_pred=np.concatenate([r, f[:, None]], -1), qgrad=qg, Hq=Hq, E=E)


def oracle_levels(case_args, it, lam, initialize, hop=False, prior=None, need_accept=True):
    """``Levels`` of a call of the oracle at ``case_args`` = (states, cumrot, uv, xyz, ii, time_idx, K, conf): the oracle's own
    factor, assembly, first trial and means through the layers above.  Asserts the conditions on the case: no oracle figure above
    1024 units, nothing where nothing is summed, the first trial accepted (``need_accept``)."""
    states, cumrot, uv, xyz, ii, t, K, conf = case_args
    st = np.asarray(states, dtype=np.float64)
    n = st.shape[0]
    dbg = {}
    out, lam_out, hess, ntr = O.ba_iteration(it, st, cumrot, uv, xyz, ii, t, K, conf, lam, initialize=initialize, debug=dbg, hop=hop,
                                             prior=prior)
    accepted = ntr == 1 and dbg["trials"][0]["residual"] < dbg["init_residual"]
    assert accepted or not need_accept, "a badly chosen case: the oracle rejects the first trial"
    _, sigma = O.lm_schedule(it)
    lam32 = dbg["trials"][0]["lam32"]
    figs, exact = {}, []
    if initialize:
        fac = dict(Phi=np.zeros((n, 6, 6)), r_pred=np.zeros((n - 1, 7)), qgrad=np.zeros((n, 3)), Hq=np.zeros((n, 3, 3, 3)))
        # the fp64 step the bars come from is Gauss-Jordan elimination without row exchanges on each pose's 6x6 block (positive
        # definite: H_i + lam32 I) in NumPy: what the issue's "6x6 solve per pose" is in fp64.  (The oracle's banded LU of the 9n
        # system stands at 4.2 units by the same measure: its bar would be 16.7 instead of 16.)
        dp6 = np.zeros((n, 9))
        dp6[:, :6] = _solve_ld(dbg["H"] + lam32 * np.eye(6), dbg["b"][:, :, None].copy(), pivot=False)[:, :, 0]
        g, e = step_layer(dp6, O.retract(st, dp6), dbg["H"], dbg["b"], lam32, st)
        figs.update(g)
        exact += e
    else:
        fac = oracle_factor(st, t, cumrot, hop)
        g, e = factor_layer(st, t, cumrot, fac["Phi"], fac["r_pred"], fac["qgrad"], fac["Hq"], hop)
        figs.update(g)
        exact += e
    g, e = assembly_layer(dbg["bands"], dbg["rhs"], hess, lam32, dbg["H"], dbg["b"], sigma, fac["Phi"], fac["r_pred"], fac["qgrad"],
                          fac["Hq"], initialize, prior, st)
    figs.update(g)
    exact += e
    reg = prior is not None
    pr = prior_ld(st, prior)[0] if reg and not initialize else (np.zeros((n, 6)) if reg else None)
    pden = prior_ld(st, prior, absolute=True)[0] if reg and not initialize else None
    ref, den = residual_sums_ld(uv, dbg["est"], None, fac["r_pred"], sigma, n, initialize, pr, prior_den=pden)
    figs["sum_init"] = sums_figure(dbg["init_residual"], ref, den)
    units = _units(figs)
    assert not exact, exact
    bad = {k: v for k, v in units.items() if not v <= K_CASE_MAX}
    assert not bad, f"a badly chosen case: the oracle's own figures {bad} exceed {K_CASE_MAX:g} x 2^-53"
    return Levels(units, dict(dbg=dbg, out=out, hess=hess, lam32=lam32, sigma=sigma, fac=fac, lam_out=lam_out,
                              sum_total=float(ref * (2 * len(ii) + (6 if initialize else 7) * (n - 1) + ((6 if initialize else 7) * n if reg else 0)))))


@dataclass
class Verdict:
    units: dict
    bars: dict
    where: dict                 # name -> index tuple of the largest figure: (pose, entry ...)
    exact: list

    @property
    def failures(self):
        return [f"{k}: {self.units[k]:.3g} > K = {self.bars[k]:.3g} (x 2^-53) at pose {self.where[k][0] if self.where[k] else -1}, "
                f"entry {self.where[k][1:] if self.where[k] else ()}" for k in self.units if not self.units[k] <= self.bars[k]] + self.exact

    @property
    def ok(self):
        return not self.failures


def judge(levels, figs, exact=(), bars=None):
    """``figs`` (dict name -> array, pose first) against the bars of ``levels``; a name the oracle has no figure for (the trial
    mean of the second call) answers to the bar of ``bars[name]``, another name of ``levels``."""
    units, K, where = {}, {}, {}
    for k, v in figs.items():
        v = np.asarray(v)
        units[k] = float(v.max()) / U if v.size else 0.0
        where[k] = tuple(int(q) for q in np.unravel_index(int(np.argmax(v)), v.shape)) if v.size else ()
        K[k] = levels.K((bars or {}).get(k, k))
    return Verdict(units, K, where, list(exact))
