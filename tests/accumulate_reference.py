"""Judging the accumulation stage of a BA call (A1 .. A3b) in extended precision (no GPU needed).

A restatement in ``np.longdouble`` of the reprojection and its 2x6 Jacobian (``BA_utils.py:7-50``), of the robust weights
(``BA_filtering.py:21-25``) and of the per-pose sums ``H_i = sum w J^T J``, ``b_i = sum w J^T r`` (``BA_filtering.py:30-37, 44``),
written from the formulas; nothing here calls ``oracle/ba_oracle.py`` except ``oracle_run`` / ``oracle_levels``, which measure the
oracle AGAINST this reference to set the bars.

Layer A (``layer_a``): the sums of the rows a device (or the oracle) itself reports.  From its ``est``, final ``weight`` and ``Jg``
and the uploaded ``uv``, ``ii`` the sums are formed in longdouble; per pose and block group (t = columns 0..2, r = 3..5)

    phi_H(i, g1, g2) = max_{a in g1, b in g2} |H - H_A|_ab / sum_{k in pose i} w_k |J_k[:, g1]|_F |J_k[:, g2]|_F
    phi_b(i, g)      = max_{a in g} |b - b_A|_a            / sum_k w_k |J_k[:, g]|_F |r_k|_2

The denominators do not change under the pose's rotation, so a kernel that sums in the camera frame and rotates once answers to
the same figure as one that sums world-frame rows.  A block whose denominator is 0 (a pose without rows, or with rows of weight 0
only) must hold exact zeros; such blocks are left out of the maximum and reported apart (``zero_residual``), as ``Omega.zero_rows``
of tests/solve_residual.py.  Rounding of the reference itself: every term is rounded to 2^-64 and a segment of 201 rows is summed
in sequence, <= 201 * 2^-64 = 0.1 units of 2^-53 of the denominator.

Layer B (``layer_b``): the rows themselves from the input states, intrinsics and observations:

    est     |d est|_inf / (f d |X - t|_2),  d = 1 / max(z, 0.1)
    J_t/J_r |d J_g|_F / |J_g|_F per column group; the z-derivative is off at z <= 0.1 and the true z stays in hat(p_c)
    w       |d w| / w of the final weight (w_raw / w_max) conf, from the judged side's own residual uv - est, its own median
            c and its own w_max: the closed forms alone, not the select.  A row of confidence 0 must have weight exactly 0
            (``zero_conf_bad`` counts the ones that do not).

``judge``: a figure passes if it is <= K * 2^-53 with K = max(16, 4 x the figure of the fp64 NumPy oracle functions
(``landmark_project``, ``robust_weights``, ``accumulate``) against this reference on the same case).  4 x: a device differs from
NumPy by fma contraction, a reciprocal refined to 1 ulp and another summation tree -- each moves the constant, none the order;
16: a case on which NumPy happens to be exact.  An oracle figure above 1024 x 2^-53 is a badly chosen case (``oracle_levels``
asserts it), never a looser bar.  No bar comes from a device run."""
from dataclasses import dataclass, field

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
Z_MIN = LD(np.float64(0.1))          # BA_utils.py:13, the double the kernels compare with
T, R = slice(0, 3), slice(3, 6)
H_GROUPS = (("H_tt", T, T), ("H_tr", T, R), ("H_rr", R, R))
B_GROUPS = (("b_t", T), ("b_r", R))
ROW_FIGURES = ("est", "J_t", "J_r", "w")
K_FLOOR, K_FACTOR, K_CASE_MAX = 16.0, 4.0, 1024.0


def lm_alpha(it):
    """BA_filtering.py:22."""
    return min(max(1 - (2 * (it / 5) - 1), 1), 2)


# ------------------------------------------------------------------------------------------------ the rows (A1, A2)
def rotation_ld(q):
    """Rotation matrices [.., 3, 3] (camera -> ECI) of the normalised quaternions q [.., 4] (scalar last), longdouble."""
    q = np.asarray(q).astype(LD)
    q = q / np.sqrt((q * q).sum(-1, keepdims=True))
    x, y, z, w = np.moveaxis(q, -1, 0)
    return np.stack([
        np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
        np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
        np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1),
    ], -2)


@dataclass
class Rows:
    est: np.ndarray         # [m, 2]
    Jg: np.ndarray          # [m, 2, 6] over [dp, dtheta]
    pc: np.ndarray          # [m, 3] camera-frame point
    scale: np.ndarray       # [m] f d |X - t|_2: what one relative rounding of the point is worth in pixels
    live: np.ndarray        # [m] bool: z > 0.1


def rows_ld(states, xyz, intr, ii):
    """Reprojection and Jacobian of every row in longdouble (BA_utils.py:7-17, 30-50, 1052-1069)."""
    states, xyz, intr = np.asarray(states), np.asarray(xyz), np.asarray(intr)
    ii = np.asarray(ii, dtype=np.int64)
    Rm = rotation_ld(states[:, 3:7])[ii]                                # [m, 3, 3]
    dX = xyz.astype(LD) - states[ii, :3].astype(LD)
    pc = np.einsum("kji,kj->ki", Rm, dX)                                # R^T (X - t)
    K = intr[ii].astype(LD)
    x, y, z = pc[:, 0], pc[:, 1], pc[:, 2]
    live = z > Z_MIN
    d = 1 / np.where(live, z, Z_MIN)
    est = np.stack([K[:, 0] * (d * x) + K[:, 2], K[:, 1] * (d * y) + K[:, 3]], -1)
    m = xyz.shape[0]
    A = np.zeros((m, 2, 3), dtype=LD)                                   # d uv / d p_c
    A[:, 0, 0] = K[:, 0] * d
    A[:, 1, 1] = K[:, 1] * d
    A[:, 0, 2] = np.where(live, -K[:, 0] * x * d * d, LD(0))
    A[:, 1, 2] = np.where(live, -K[:, 1] * y * d * d, LD(0))
    hat = np.zeros((m, 3, 3), dtype=LD)                                 # of the TRUE point, clamped or not
    hat[:, 0, 1], hat[:, 0, 2] = -z, y
    hat[:, 1, 0], hat[:, 1, 2] = z, -x
    hat[:, 2, 0], hat[:, 2, 1] = -y, x
    Jt = -np.einsum("kab,kcb->kac", A, Rm)
    Jr = 2 * np.einsum("kab,kbc->kac", A, hat)
    f = np.maximum(K[:, 0], K[:, 1])
    return Rows(est, np.concatenate([Jt, Jr], -1), pc, f * d * np.sqrt((dX * dX).sum(-1)), np.asarray(live))


def weights_ld(r, conf, c, wmax, it):
    """Final weights (w_raw / wmax) conf in longdouble from residuals r [m, 2], the median c and the largest raw weight wmax as
    given (BA_filtering.py:21-25; alpha == 2: ((r/c)^2 / 0 + 1)^0 == 1)."""
    r, conf, c, wmax = np.asarray(r).astype(LD), np.asarray(conf).astype(LD), LD(c), LD(wmax)
    alpha = lm_alpha(it)
    if alpha == 2:
        raw = np.full(r.shape[0], 1 / (c * c), dtype=LD)
    else:
        s = r / c
        per = np.power(s * s / LD(abs(alpha - 2)) + 1, LD(alpha) / 2 - 1) / (c * c)
        raw = per.sum(-1) / 2
    return raw / wmax * conf


# ------------------------------------------------------------------------------------------------ layer A
def _segments(ii, n):
    order = np.argsort(np.asarray(ii, dtype=np.int64), kind="stable")
    counts = np.bincount(np.asarray(ii, dtype=np.int64), minlength=n)
    return order, counts


def _seg_sum(terms, order, counts):
    """Per-pose sums [n, ...] of per-row terms [m, ...], rows added in sequence."""
    n = counts.size
    out = np.zeros((n,) + terms.shape[1:], dtype=terms.dtype)
    if terms.shape[0] == 0:
        return out
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    has = counts > 0
    out[has] = np.add.reduceat(terms[order], starts[has], axis=0)
    return out


def sums_ld(Jg, w, r, ii, n):
    """(H [n, 6, 6], b [n, 6]) in longdouble and the denominators (den_H [n, 3], den_b [n, 2]) of the figures."""
    J, w, r = np.asarray(Jg).astype(LD), np.asarray(w).astype(LD), np.asarray(r).astype(LD)
    order, counts = _segments(ii, n)
    wJ = J * w[:, None, None]
    H = _seg_sum(np.einsum("kca,kcb->kab", wJ, J), order, counts)
    b = _seg_sum(np.einsum("kca,kc->ka", wJ, r), order, counts)
    nt = np.sqrt((J[:, :, T] ** 2).sum((1, 2)))
    nr = np.sqrt((J[:, :, R] ** 2).sum((1, 2)))
    rn = np.sqrt((r * r).sum(-1))
    aw = np.abs(w)
    den_H = _seg_sum(np.stack([aw * nt * nt, aw * nt * nr, aw * nr * nr], -1), order, counts)
    den_b = _seg_sum(np.stack([aw * nt * rn, aw * nr * rn], -1), order, counts)
    return H, b, den_H, den_b


@dataclass
class FigA:
    H: np.ndarray               # [n, 3] phi_H per pose for (tt, tr, rr); 0 where the denominator vanishes
    b: np.ndarray               # [n, 2] phi_b per pose for (t, r)
    zero_H: np.ndarray          # [n, 3] bool: denominator exactly 0
    zero_b: np.ndarray          # [n, 2]
    zero_residual: float        # max |entry| over the blocks without denominator: must be exactly 0

    def figures(self):
        out = {name: self.H[:, k] for k, (name, _, _) in enumerate(H_GROUPS)}
        out.update({name: self.b[:, k] for k, (name, _) in enumerate(B_GROUPS)})
        return out


def layer_a(H, b, est, weight, Jg, uv, ii, n):
    """The figures of sums ``H`` [n, 6, 6], ``b`` [n, 6] against the longdouble sums of the rows ``est``, ``weight``, ``Jg``."""
    H, b = np.asarray(H, dtype=np.float64), np.asarray(b, dtype=np.float64)
    # the residual as both the kernels and the oracle form it: one fp64 subtraction (its rounding belongs to the row, not the sum)
    r = np.asarray(uv, dtype=np.float64) - np.asarray(est, dtype=np.float64)
    HA, bA, den_H, den_b = sums_ld(Jg, weight, r, ii, n)
    dH, db = np.abs(H.astype(LD) - HA), np.abs(b.astype(LD) - bA)
    if not (np.isfinite(H).all() and np.isfinite(b).all()):
        inf = np.full((n, 3), np.inf)
        return FigA(inf, inf[:, :2], den_H == 0, den_b == 0, float("inf"))
    fH, fb = np.zeros((n, 3)), np.zeros((n, 2))
    zres = 0.0
    for k, (_, g1, g2) in enumerate(H_GROUPS):
        num = np.maximum(dH[:, g1, g2].max((1, 2)), dH[:, g2, g1].max((1, 2)))
        z = den_H[:, k] == 0
        fH[~z, k] = (num[~z] / den_H[~z, k]).astype(np.float64)
        if z.any():
            zres = max(zres, float(np.abs(H[z][:, g1, g2]).max()), float(np.abs(H[z][:, g2, g1]).max()))
    for k, (_, g) in enumerate(B_GROUPS):
        num = db[:, g].max(1)
        z = den_b[:, k] == 0
        fb[~z, k] = (num[~z] / den_b[~z, k]).astype(np.float64)
        if z.any():
            zres = max(zres, float(np.abs(b[z][:, g]).max()))
    return FigA(fH, fb, den_H == 0, den_b == 0, zres)


# ------------------------------------------------------------------------------------------------ layer B
@dataclass
class FigB:
    est: np.ndarray             # [m]
    J_t: np.ndarray             # [m]
    J_r: np.ndarray             # [m]
    w: np.ndarray               # [m] (0 for rows of confidence 0)
    zero_conf_bad: int          # rows of confidence 0 whose weight is not exactly 0

    def figures(self):
        return {k: getattr(self, k) for k in ROW_FIGURES}


def layer_b(states, xyz, intr, uv, ii, conf, it, est, Jg, weight, c, wmax, rows=None):
    """The rows ``est`` [m, 2], ``Jg`` [m, 2, 6], ``weight`` [m] of a device (or the oracle) against the longdouble rows; ``c`` and
    ``wmax`` are that side's own median and largest raw weight.  ``rows``: ``rows_ld`` of the case, if the caller has it."""
    ref = rows or rows_ld(states, xyz, intr, ii)
    est, Jg, weight = np.asarray(est, dtype=np.float64), np.asarray(Jg, dtype=np.float64), np.asarray(weight, dtype=np.float64)
    conf = np.asarray(conf, dtype=np.float64)
    f_est = (np.abs(est.astype(LD) - ref.est).max(-1) / ref.scale).astype(np.float64)
    dJ = Jg.astype(LD) - ref.Jg
    fro = lambda a: np.sqrt((a * a).sum((1, 2)))
    f_t = (fro(dJ[:, :, T]) / fro(ref.Jg[:, :, T])).astype(np.float64)
    f_r = (fro(dJ[:, :, R]) / fro(ref.Jg[:, :, R])).astype(np.float64)
    w_ref = weights_ld(np.asarray(uv, dtype=np.float64) - est, conf, c, wmax, it)
    pos = conf != 0
    f_w = np.zeros(weight.shape[0])
    f_w[pos] = (np.abs(weight.astype(LD) - w_ref)[pos] / np.abs(w_ref[pos])).astype(np.float64)
    for f in (f_est, f_t, f_r, f_w):
        f[~np.isfinite(f)] = np.inf
    return FigB(f_est, f_t, f_r, f_w, int(np.count_nonzero(weight[~pos] != 0.0)))


# ------------------------------------------------------------------------------------------------ the bars
def oracle_run(states, xyz, intr, uv, ii, conf, it, n):
    """The fp64 NumPy oracle's A1 .. A3b on a case: dict(est, Jg, r, w, c, wmax, H, b)."""
    from oracle import ba_oracle as O
    est, Jg = O.landmark_project(np.asarray(states, dtype=np.float64), xyz, intr, np.asarray(ii, dtype=np.int64))
    r = uv - est
    w, c, wmax = O.robust_weights(r, it, conf)
    H, b = O.accumulate(Jg, w, r, np.asarray(ii, dtype=np.int64), n)
    return dict(est=est, Jg=Jg, r=r, w=w, c=c, wmax=wmax, H=H, b=b)


@dataclass
class Levels:
    """Largest figure of the oracle functions per name, in units of 2^-53, and the oracle's arrays."""
    units: dict
    oracle: dict = field(repr=False, default=None)
    rows: Rows = field(repr=False, default=None)

    def K(self, name):
        return max(K_FLOOR, K_FACTOR * self.units[name])


def oracle_levels(states, xyz, intr, uv, ii, conf, it, n):
    """``Levels`` of a case.  Asserts the condition on the case: no oracle figure above 1024 x 2^-53, exact zeros where a
    denominator vanishes, weight 0 at confidence 0."""
    o = oracle_run(states, xyz, intr, uv, ii, conf, it, n)
    rows = rows_ld(states, xyz, intr, ii)
    a = layer_a(o["H"], o["b"], o["est"], o["w"], o["Jg"], uv, ii, n)
    b = layer_b(states, xyz, intr, uv, ii, conf, it, o["est"], o["Jg"], o["w"], o["c"], o["wmax"], rows)
    units = {k: (float(v.max()) / U if v.size else 0.0) for k, v in {**a.figures(), **b.figures()}.items()}
    assert a.zero_residual == 0.0 and b.zero_conf_bad == 0, "the oracle leaves something where there is nothing to sum"
    bad = {k: v for k, v in units.items() if not v <= K_CASE_MAX}
    assert not bad, f"a badly chosen case: the oracle's own figures {bad} exceed {K_CASE_MAX:g} x 2^-53"
    return Levels(units, o, rows)


@dataclass
class Verdict:
    units: dict                 # name -> largest figure in units of 2^-53
    bars: dict                  # name -> K
    where: dict                 # name -> index (pose for layer A, row for layer B) of the largest figure
    exact: list                 # what is not exactly zero although it must be

    @property
    def failures(self):
        return [f"{k}: {self.units[k]:.3g} > K = {self.bars[k]:.3g} (x 2^-53) at index {self.where[k]}"
                for k in self.units if not self.units[k] <= self.bars[k]] + self.exact

    @property
    def ok(self):
        return not self.failures


def judge(levels, a=None, b=None):
    """Layer-A figures ``a`` (FigA) and / or layer-B figures ``b`` (FigB) against the bars of ``levels``."""
    units, bars, where, exact = {}, {}, {}, []
    figs = {}
    if a is not None:
        figs.update(a.figures())
        if a.zero_residual != 0.0:
            exact.append(f"|entry| {a.zero_residual:.3e} in a block whose rows sum to nothing")
    if b is not None:
        figs.update(b.figures())
        if b.zero_conf_bad:
            exact.append(f"{b.zero_conf_bad} rows of confidence 0 with a non-zero weight")
    for k, v in figs.items():
        units[k] = float(v.max()) / U if v.size else 0.0
        where[k] = int(np.argmax(v)) if v.size else -1
        bars[k] = levels.K(k)
    return Verdict(units, bars, where, exact)
