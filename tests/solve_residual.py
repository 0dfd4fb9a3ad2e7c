"""Judging a block-tridiagonal solve by the system it was given (no GPU needed).

The damped 9x9 block-tridiagonal systems of a BA call have condition numbers of 1e11 .. 1e14, so a forward bar against a recorded
``dpose`` has to be loose (tests/test_gpu_parity.py, DPOSE_TOL).  The backward error does not depend on the condition number:
``omega`` below is the componentwise (Oettli-Prager) figure

    omega(x) = max_k |b - A x|_k / (|A| |x| + |b|)_k

with everything formed in ``np.longdouble``.  The componentwise form, not the normwise ``|r| / (|A| |x| + |b|)`` over norms: the nine
slots of a pose mix km, rotation and km/s, and a relative error of 1e-9 planted in one component moves the normwise figure of the
recorded systems only to ~1e-14 while the figure of a correct solve is 1e-20 .. 1e-17 -- blind.

Bands are ``[n, 3, 9, 9]`` = (sub, diag, super) as ``VBA_DBG_BANDS`` / ``oracle.ba_oracle.assemble`` return them; every function
here takes the DAMPED bands (``damped(bands, lam32)``).

What a bar is set against: ``cpu_solves`` -- three fp64 CPU solves of the same system (dense LU, LAPACK's banded LU, an unpivoted
block Thomas recurrence) -- and ``x_star``, the dense LU solution refined with longdouble residuals.  ``judge`` forms both bars of
tests/test_gpu_solve_paths.py from them, so the host test of the planted faults and the GPU test share one rule."""
from dataclasses import dataclass

import numpy as np
import scipy.linalg

from oracle import ba_oracle as O

LD = np.longdouble
GROUPS = (("dp", slice(0, 3)), ("dtheta", slice(3, 6)), ("dv", slice(6, 9)))
EPS = 2.0 ** -52


def dense_from_bands(bands):
    """The [9n, 9n] matrix of bands [n, 3, 9, 9]."""
    return O.bands_to_dense(np.asarray(bands))


def damped(bands, lam32):
    """Copy of the undamped bands with ``lam32`` added to the diagonal of every diagonal block."""
    out = np.array(bands, dtype=np.float64, copy=True)
    out[:, 1] += float(lam32) * np.eye(9)
    return out


def _matvec(A, x):
    """A x block-wise from the bands, in the dtype of the arguments: [n, 9]."""
    y = np.einsum("iab,ib->ia", A[:, 1], x)
    if x.shape[0] > 1:
        y[1:] += np.einsum("iab,ib->ia", A[1:, 0], x[:-1])
        y[:-1] += np.einsum("iab,ib->ia", A[:-1, 2], x[1:])
    return y


def residual_ld(bands_damped, x, rhs):
    """(b - A x, |A| |x| + |b|) in longdouble, both [n, 9], formed block-wise from the bands."""
    n = bands_damped.shape[0]
    A = np.asarray(bands_damped).astype(LD)
    xl = np.asarray(x).astype(LD).reshape(n, 9)
    b = np.asarray(rhs).astype(LD).reshape(n, 9)
    return b - _matvec(A, xl), _matvec(np.abs(A), np.abs(xl)) + np.abs(b)


@dataclass
class Omega:
    value: float                # max over the rows with a non-zero denominator
    per_pose: np.ndarray        # [n] the same per pose (0 for a pose whose nine denominators all vanish)
    zero_rows: np.ndarray       # [n, 9] bool: rows whose denominator is exactly 0
    zero_rows_residual: float   # max |r| over those rows: must be exactly 0

    @property
    def worst_pose(self):
        return int(np.argmax(self.per_pose))


def omega(bands_damped, x, rhs):
    """Componentwise backward error of ``x`` for ``A x = rhs`` (module docstring).  Rows whose denominator is 0 -- velocity slots
    of a landmark-only call: zero right-hand side, zero solution -- are left out of the maximum and reported apart; a non-finite
    ``x`` gives ``inf``."""
    r, den = residual_ld(bands_damped, x, rhs)
    zero = den == 0
    if not (np.isfinite(r.astype(np.float64)).all() and np.isfinite(den.astype(np.float64)).all()):
        n = r.shape[0]
        return Omega(float("inf"), np.full(n, np.inf), zero, float("inf"))
    ratio = np.zeros(r.shape, dtype=LD)
    np.divide(np.abs(r), den, out=ratio, where=~zero)
    zr = float(np.abs(r[zero]).max()) if zero.any() else 0.0
    return Omega(float(ratio.max()), ratio.max(axis=1).astype(np.float64), zero, zr)


def x_star(bands_damped, rhs, lu=None):
    """Reference solution [n, 9] in longdouble: dense fp64 LU (``lu``: its factors, if the caller has them), then iterative
    refinement with longdouble residuals until the correction stops shrinking."""
    n = bands_damped.shape[0]
    lu = lu or scipy.linalg.lu_factor(dense_from_bands(bands_damped))
    b = np.asarray(rhs, dtype=np.float64).reshape(-1)
    x = scipy.linalg.lu_solve(lu, b).astype(LD).reshape(n, 9)
    last = np.inf
    for _ in range(40):
        r, _den = residual_ld(bands_damped, x, rhs)
        d = scipy.linalg.lu_solve(lu, r.astype(np.float64).reshape(-1)).reshape(n, 9)
        size = float(np.abs(d).max())
        if not size < last:
            break
        x = x + d.astype(LD)
        last = size
        if size == 0.0:
            break
    return x


def forward_err(x, xs):
    """Per slot group (dp, dtheta, dv): max |x - x*| / max |x*| over the window, as a dict.  A group whose reference is all zero
    (dv of a landmark-only call) gives 0 for an exact zero and inf otherwise."""
    n = xs.shape[0]
    d = np.abs(np.asarray(x).astype(LD).reshape(n, 9) - xs)
    out = {}
    for name, sl in GROUPS:
        num, den = float(d[:, sl].max()), float(np.abs(xs[:, sl]).max())
        if not np.isfinite(num):
            out[name] = float("inf")
        elif den == 0.0:
            out[name] = 0.0 if num == 0.0 else float("inf")
        else:
            out[name] = num / den
    return out


def _solve9_unpivoted(D, B):
    """D^-1 B for a 9x9 ``D`` by Gaussian elimination without row exchanges."""
    M = np.concatenate([D, B], axis=1).astype(np.float64)
    for k in range(9):
        M[k] /= M[k, k]
        rows = np.arange(9) != k
        M[rows] -= np.outer(M[rows, k], M[k])
    return M[:, 9:]


def thomas_unpivoted(bands_damped, rhs):
    """The sequential algorithm restated: D_i = A_ii - L_i D_{i-1}^-1 U_{i-1}, forward along the chain and back, no row
    exchanges anywhere."""
    n = bands_damped.shape[0]
    A = np.asarray(bands_damped, dtype=np.float64)
    b = np.asarray(rhs, dtype=np.float64).reshape(n, 9)
    Y = np.zeros((n, 9, 9))             # D_i^-1 U_i
    z = np.zeros((n, 9))                # D_i^-1 (b_i - L_i z_{i-1})
    with np.errstate(all="ignore"):
        for i in range(n):
            D, g = A[i, 1].copy(), b[i].copy()
            if i > 0:
                D -= A[i, 0] @ Y[i - 1]
                g -= A[i, 0] @ z[i - 1]
            S = _solve9_unpivoted(D, np.concatenate([A[i, 2], g[:, None]], axis=1))
            Y[i], z[i] = S[:, :9], S[:, 9]
        x = np.zeros((n, 9))
        x[n - 1] = z[n - 1]
        for i in range(n - 2, -1, -1):
            x[i] = z[i] - Y[i] @ x[i + 1]
    return x


def cpu_solves(bands_damped, rhs, lu=None):
    """{"dense": LAPACK's dense LU with partial pivoting (what ``np.linalg.solve`` runs; ``lu``: its factors, if the caller has
    them), "banded": LAPACK's banded LU, "thomas": the unpivoted block recurrence}, each [n, 9] fp64."""
    n = bands_damped.shape[0]
    b = np.asarray(rhs, dtype=np.float64).reshape(n, 9)
    lu = lu or scipy.linalg.lu_factor(dense_from_bands(bands_damped))
    return {"dense": scipy.linalg.lu_solve(lu, b.reshape(-1)).reshape(n, 9),
            "banded": O.solve_tridiag(np.asarray(bands_damped), b, "banded"),
            "thomas": thomas_unpivoted(bands_damped, b)}


@dataclass
class Levels:
    """Reference levels of one system: the worst of the three CPU solves."""
    omega: float
    fwd: dict
    xs: np.ndarray
    solves: dict

    def bar_omega(self, M):
        return max(M * self.omega, M * EPS)

    def bar_fwd(self, M):
        return {g: M * v for g, v in self.fwd.items()}


def levels(bands_damped, rhs):
    lu = scipy.linalg.lu_factor(dense_from_bands(bands_damped))
    xs = x_star(bands_damped, rhs, lu)
    sol = cpu_solves(bands_damped, rhs, lu)
    om = max(omega(bands_damped, x, rhs).value for x in sol.values())
    fw = {g: max(forward_err(x, xs)[g] for x in sol.values()) for g, _ in GROUPS}
    return Levels(om, fw, xs, sol)


@dataclass
class Verdict:
    omega: Omega
    fwd: dict
    bar_omega: float
    bar_fwd: dict
    ratio_omega: float          # omega / max(omega of the CPU solves, 2^-52): the bar is M times the denominator
    ratio_fwd: float            # the largest over the groups of forward_err / that of the CPU solves

    @property
    def ok(self):
        return (self.omega.zero_rows_residual == 0.0 and self.omega.value <= self.bar_omega
                and all(self.fwd[g] <= self.bar_fwd[g] for g in self.fwd))


def _ratio(a, b):
    if a == 0.0:
        return 0.0
    return float("inf") if b == 0.0 else a / b


def judge(bands_damped, x, rhs, M, lv=None, M_fwd=None):
    """``x`` against the two bars formed from the CPU solves of the same system: omega <= max(M omega_cpu, M 2^-52) and, per slot
    group, forward_err <= M_fwd forward_err_cpu (``M_fwd``: M unless given)."""
    lv = lv or levels(bands_damped, rhs)
    om = omega(bands_damped, x, rhs)
    fw = forward_err(x, lv.xs)
    return Verdict(om, fw, lv.bar_omega(M), lv.bar_fwd(M if M_fwd is None else M_fwd), _ratio(om.value, max(lv.omega, EPS)),
                   max(_ratio(fw[g], lv.fwd[g]) for g in fw))


def window_for(n, rows_per_pose=3, seed=0, gaps=None):
    """A synthetic window of exactly ``n`` poses with ``rows_per_pose`` rows each: (window, time_idx, initial states).  ``gaps``
    [n - 1] (seconds) replaces the 5 s spacing of the frames, the way tests/random_windows.py does."""
    from vinsat_amd import od_pipe, synth
    det, orb = synth.make_sequence(synth.WindowConfig(f"res{n}", n, rows_per_pose, 5), seed=seed)
    win = od_pipe.prepare_window(det, orb)
    assert win.time_idx.size == n, (n, win.time_idx.size, seed)
    t = win.time_idx
    if gaps is not None:
        t = np.cumsum(np.concatenate([[10], np.asarray(gaps)])).astype(np.int64)
        assert t.size == n
    return win, t, od_pipe.initial_guess(win, seed=seed)
