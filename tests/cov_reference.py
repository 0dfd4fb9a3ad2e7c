"""Judging the covariance query (vba_covariance) per component, against the system it inverted (no GPU needed).

Reference: the selected inverse -- the blocks Sigma_ii and Sigma_i,i+1 of ((A + A^T) / 2 + lam32 I)^-1 -- from bands [n, 3, 9, 9]
(sub, diag, super as ``VBA_DBG_BANDS`` / ``oracle.ba_oracle.assemble`` return them) in ``np.longdouble``: the block LDL^T
recurrence forward and backward (``selected_inverse_ld``) and, for small windows, the dense inverse (``dense_inverse_ld``), both on a
hand-written elimination with row exchanges (``solve_ld``: LAPACK takes no longdouble).

Metric (``scaled_err``): componentwise, every entry scaled by the sigmas of its own row and column,

    diagonal block   |dSigma_ii[a, b]|    / sqrt(Sigma_ii[a, a] Sigma_ii[b, b])
    super block      |dSigma_i,i+1[a, b]| / sqrt(Sigma_ii[a, a] Sigma_i+1,i+1[b, b])

i.e. the error of the correlation coefficient where the variances are right, and the relative error of a variance on the diagonal.
``max|dS| / max|S|`` per block (tests/cov_oracle.py) is led by the position variances (km^2); velocity entries and most cross terms
are orders of magnitude smaller and a wrong one passes.  The largest figure is kept per pose and per group pair (position,
attitude, velocity: six pairs for a diagonal block, nine for a super block), so a failure names the pose and the component group.

fp64 CPU references for the bars (``cpu_references``): the three of tests/cov_oracle.py (LU inverse, Cholesky on identity
columns, block recurrence) and ``partitioned_fp64``, the partitioned algorithm of csrc/vba_cov.hip at a given chunk size, so that
a bar carries the method's own rounding and not only the sequential recurrence's.  ``judge`` forms the bars from them:
bar[group] = max(M * max(error[group] of the four references), M * 2^-52)."""
from dataclasses import dataclass

import numpy as np

import cov_oracle as C

LD = np.longdouble
EPS = 2.0 ** -52
GROUPS = (("pos", slice(0, 3)), ("att", slice(3, 6)), ("vel", slice(6, 9)))
DIAG_PAIRS = tuple((a, b) for a in range(3) for b in range(a, 3))      # six: the block is symmetric
SUPER_PAIRS = tuple((a, b) for a in range(3) for b in range(3))        # nine
KEYS = tuple(f"diag {GROUPS[a][0]}-{GROUPS[b][0]}" for a, b in DIAG_PAIRS) + tuple(f"super {GROUPS[a][0]}-{GROUPS[b][0]}" for a, b in SUPER_PAIRS)


def sym_blocks(bands, lam32=0.0, dtype=np.float64):
    """(Ad [n, 9, 9], B [n, 9, 9]) of the symmetrised system in ``dtype``: A^_ii and A^_i,i+1 (zeros for the last pose)."""
    b = np.asarray(bands).astype(dtype)
    n = b.shape[0]
    Ad = (b[:, 1] + b[:, 1].transpose(0, 2, 1)) / dtype(2) + dtype(lam32) * np.eye(9, dtype=dtype)
    B = np.zeros((n, 9, 9), dtype=dtype)
    B[:-1] = (b[:-1, 2] + b[1:, 0].transpose(0, 2, 1)) / dtype(2)
    return Ad, B


def solve_ld(D, R):
    """D^-1 R in longdouble: Gauss-Jordan elimination with row exchanges on [D | R], any size."""
    N = D.shape[0]
    M = np.concatenate([np.asarray(D).astype(LD), np.asarray(R).astype(LD)], axis=1)
    for k in range(N):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        if p != k:
            M[[k, p]] = M[[p, k]]
        M[k] = M[k] / M[k, k]
        rows = np.arange(N) != k
        M[rows] -= np.outer(M[rows, k], M[k])
    return M[:, N:]


def selected_inverse_ld(bands, lam32=0.0):
    """(diag [n, 9, 9], super [n, 9, 9]) in longdouble by the block recurrence: D_i = A^_ii - B_i-1^T Y_i-1, Y_i = D_i^-1 B_i forward;
    S_n-1 = D_n-1^-1, S_i,i+1 = -Y_i S_i+1, S_ii = D_i^-1 - S_i,i+1 Y_i^T backward.  super[n - 1] = 0."""
    Ad, B = sym_blocks(bands, lam32, LD)
    n = Ad.shape[0]
    I9 = np.eye(9, dtype=LD)
    Dinv = np.zeros((n, 9, 9), dtype=LD)
    Y = np.zeros((n, 9, 9), dtype=LD)
    for i in range(n):
        D = Ad[i] - (B[i - 1].T @ Y[i - 1] if i > 0 else 0)
        S = solve_ld(D, np.concatenate([B[i], I9], axis=1))
        Y[i], Dinv[i] = S[:, :9], S[:, 9:]
    diag = np.zeros((n, 9, 9), dtype=LD)
    sup = np.zeros((n, 9, 9), dtype=LD)
    diag[n - 1] = Dinv[n - 1]
    for i in range(n - 2, -1, -1):
        sup[i] = -Y[i] @ diag[i + 1]
        diag[i] = Dinv[i] - sup[i] @ Y[i].T
    return (diag + diag.transpose(0, 2, 1)) / LD(2), sup


def dense_ld(bands, lam32=0.0):
    """The symmetrised matrix as a dense [9n, 9n] in longdouble."""
    Ad, B = sym_blocks(bands, lam32, LD)
    n = Ad.shape[0]
    A = np.zeros((9 * n, 9 * n), dtype=LD)
    for i in range(n):
        A[9 * i:9 * i + 9, 9 * i:9 * i + 9] = Ad[i]
        if i + 1 < n:
            A[9 * i:9 * i + 9, 9 * i + 9:9 * i + 18] = B[i]
            A[9 * i + 9:9 * i + 18, 9 * i:9 * i + 9] = B[i].T
    return A


def dense_inverse_ld(bands, lam32=0.0):
    """(A^, A^^-1) dense in longdouble by the same elimination (small n only: 9n Python steps over a [9n, 18n] array)."""
    A = dense_ld(bands, lam32)
    return A, solve_ld(A, np.eye(A.shape[0], dtype=LD))


def identity_residual(bands, lam32, diag, sup):
    """max over poses and entries of |(A^ Sigma)_ii - I| / (|A^| |Sigma|)_ii, in longdouble, from the selected blocks alone:
    (A^ Sigma)_ii = B_i-1^T Sigma_i-1,i + A^_ii Sigma_ii + B_i Sigma_i,i+1^T."""
    Ad, B = sym_blocks(bands, lam32, LD)
    n = Ad.shape[0]
    d, s = np.asarray(diag).astype(LD), np.asarray(sup).astype(LD)
    worst = 0.0
    for i in range(n):
        R = Ad[i] @ d[i] - np.eye(9, dtype=LD)
        den = np.abs(Ad[i]) @ np.abs(d[i])
        if i > 0:
            R = R + B[i - 1].T @ s[i - 1]
            den = den + np.abs(B[i - 1].T) @ np.abs(s[i - 1])
        if i + 1 < n:
            R = R + B[i] @ s[i].T
            den = den + np.abs(B[i]) @ np.abs(s[i].T)
        worst = max(worst, float((np.abs(R) / den).max()))
    return worst


# ---------------------------------------------------------------------------------------------------------------- metric
@dataclass
class Scaled:
    diag: np.ndarray            # [n, 6]  largest scaled error per pose and group pair (DIAG_PAIRS)
    sup: np.ndarray             # [n - 1, 9]  the same for the super blocks (SUPER_PAIRS)

    @property
    def groups(self):
        """{key: (largest figure, its pose)} over KEYS."""
        out = {}
        for k, _ in enumerate(DIAG_PAIRS):
            out[KEYS[k]] = (float(self.diag[:, k].max()), int(np.argmax(self.diag[:, k])))
        for k, _ in enumerate(SUPER_PAIRS):
            col = self.sup[:, k] if self.sup.shape[0] else np.zeros(1)
            out[KEYS[6 + k]] = (float(col.max()), int(np.argmax(col)))
        return out

    @property
    def worst(self):
        g = self.groups
        k = max(g, key=lambda key: g[key][0])
        return g[k][0], k, g[k][1]


def scaled_err(got_diag, got_sup, ref_diag, ref_sup):
    """``Scaled`` of (got_diag [n, 9, 9], got_sup [>= n - 1, 9, 9]) against the reference blocks (longdouble or fp64), the scales
    taken from the reference's variances.  A non-finite entry gives inf."""
    rd, rs = np.asarray(ref_diag).astype(LD), np.asarray(ref_sup).astype(LD)
    n = rd.shape[0]
    sig = np.sqrt(np.abs(np.diagonal(rd, axis1=-2, axis2=-1)))          # [n, 9]
    with np.errstate(all="ignore"):
        ed = np.abs(np.asarray(got_diag).astype(LD)[:n] - rd) / (sig[:, :, None] * sig[:, None, :])
        es = np.abs(np.asarray(got_sup).astype(LD)[:n - 1] - rs[:n - 1]) / (sig[:-1, :, None] * sig[1:, None, :])
    ed = np.where(np.isfinite(ed.astype(np.float64)), ed, np.inf).astype(np.float64)
    es = np.where(np.isfinite(es.astype(np.float64)), es, np.inf).astype(np.float64)
    D = np.zeros((n, 6))
    for k, (a, b) in enumerate(DIAG_PAIRS):
        sa, sb = GROUPS[a][1], GROUPS[b][1]
        D[:, k] = np.maximum(ed[:, sa, sb].reshape(n, -1).max(1), ed[:, sb, sa].reshape(n, -1).max(1))
    S = np.zeros((n - 1, 9))
    for k, (a, b) in enumerate(SUPER_PAIRS):
        S[:, k] = es[:, GROUPS[a][1], GROUPS[b][1]].reshape(n - 1, -1).max(1)
    return Scaled(D, S)


# ---------------------------------------------------------------------------------------------------------------- fp64 references
def chunks_of(n, s):
    """[(first, last, hasL, hasR)] of the partition of csrc/vba_cov.hip: chunks of ``s`` poses whose last pose is a separator
    (pose (j + 1) s - 1 for j < P - 1, P = ceil(n / s)); the last chunk keeps all its poses."""
    P = (n + s - 1) // s
    return [(ch * s, (ch + 1) * s - 2 if ch < P - 1 else n - 1, ch > 0, ch < P - 1) for ch in range(P)]


def partitioned_fp64(bands, lam32, s, fault=None):
    """The partitioned selected inversion in NumPy fp64.  With I the interior poses (T_c per chunk), S the separators:
    X = T^-1 A_IS, Sigma_SS = (A_SS - A_SI X)^-1, Sigma_II = T^-1 + X Sigma_SS X^T, Sigma_IS = -X Sigma_SS.  Returns (diag, super).

    ``fault`` plants an index error of the kind this path can have (tests/test_cov_reference_host.py proves the metric sees each):
      ("a", j)       the Sigma_SS block of separator j is taken from separator j + 1 (j - 1 for the last one)
      ("b", "first") the X Sigma_SS X^T correction is left out for the first chunk (right neighbour only); "last": the last chunk
      ("c",)         the pose of a one-pose last chunk is left at D^-1 (= its T^-1)
      ("d", i)       the super block of pose i is transposed
      ("e", i)       a relative error of 1e-6 in the velocity-velocity part of Sigma_ii"""
    Ad, B = sym_blocks(bands, lam32)
    n = Ad.shape[0]
    parts = chunks_of(n, s)
    P = len(parts)
    q = P - 1
    kind = fault[0] if fault else None
    Tinv, X = [], []
    for first, last, hasL, hasR in parts:
        m = last - first + 1
        T = np.zeros((9 * m, 9 * m))
        for i in range(m):
            T[9 * i:9 * i + 9, 9 * i:9 * i + 9] = Ad[first + i]
            if i + 1 < m:
                T[9 * i:9 * i + 9, 9 * i + 9:9 * i + 18] = B[first + i]
                T[9 * i + 9:9 * i + 18, 9 * i:9 * i + 9] = B[first + i].T
        Ti = np.linalg.inv(T)
        Cc = np.zeros((9 * m, 18))
        if hasL:
            Cc[:9, :9] = B[first - 1].T             # A^_first,sL
        if hasR:
            Cc[9 * m - 9:, 9:] = B[last]            # A^_last,sR
        Tinv.append(Ti)
        X.append(Ti @ Cc)
    SS = np.zeros((max(q, 1), 9, 9))
    SSs = np.zeros((max(q, 1), 9, 9))
    if q > 0:
        R = np.zeros((9 * q, 9 * q))
        for j in range(q):
            f0, l0, _, _ = parts[j]
            f1, l1, _, _ = parts[j + 1]
            sep = l0 + 1
            R[9 * j:9 * j + 9, 9 * j:9 * j + 9] = Ad[sep] - B[l0].T @ X[j][-9:, 9:] - B[sep] @ X[j + 1][:9, :9]
            if j + 1 < q:
                off = -B[sep] @ X[j + 1][:9, 9:]
                R[9 * j:9 * j + 9, 9 * j + 9:9 * j + 18] = off
                R[9 * j + 9:9 * j + 18, 9 * j:9 * j + 9] = off.T
        Ri = np.linalg.inv(0.5 * (R + R.T))
        for j in range(q):
            SS[j] = Ri[9 * j:9 * j + 9, 9 * j:9 * j + 9]
            if j + 1 < q:
                SSs[j] = Ri[9 * j:9 * j + 9, 9 * j + 9:9 * j + 18]
        if kind == "a":
            j = fault[1]
            SS[j] = SS[j + 1] if j + 1 < q else SS[j - 1]
    diag = np.zeros((n, 9, 9))
    sup = np.zeros((n, 9, 9))
    for ch, (first, last, hasL, hasR) in enumerate(parts):
        m = last - first + 1
        M = np.zeros((18, 18))
        if hasL:
            M[:9, :9] = SS[ch - 1]
        if hasR:
            M[9:, 9:] = SS[ch]
        if hasL and hasR:
            M[:9, 9:] = SSs[ch - 1]
            M[9:, :9] = SSs[ch - 1].T
        XM = X[ch] @ M
        full = Tinv[ch] + XM @ X[ch].T
        if (kind == "b" and ((fault[1] == "first" and ch == 0) or (fault[1] == "last" and ch == P - 1))) or \
                (kind == "c" and ch == P - 1 and m == 1 and P > 1):
            full = Tinv[ch]
        for i in range(m):
            diag[first + i] = full[9 * i:9 * i + 9, 9 * i:9 * i + 9]
            if i + 1 < m:
                sup[first + i] = full[9 * i:9 * i + 9, 9 * i + 9:9 * i + 18]
        if hasR:
            sup[last] = -XM[-9:, 9:]                # Sigma_last,sR
            diag[last + 1] = SS[ch]
        if hasL:
            sup[first - 1] = -XM[:9, :9].T          # Sigma_sL,first
    diag = 0.5 * (diag + diag.transpose(0, 2, 1))
    if kind == "d":
        sup[fault[1]] = sup[fault[1]].T.copy()
    if kind == "e":
        diag[fault[1], 6:9, 6:9] *= 1.0 + 1e-6
    return diag, sup


ZERO_PIVOT, INDEFINITE = 4, 8


def recurrence_flags(bands, lam32=0.0):
    """The pivot checks of the device's forward sweep (cov_pivots, csrc/vba_cov_walk.h) on the fp64 block recurrence without row exchanges: ZERO_PIVOT
    if a pivot is not above 1e-10 of the diagonal entry it started from, INDEFINITE if one is negative."""
    Ad, B = sym_blocks(bands, lam32)
    n = Ad.shape[0]
    fl = 0
    Y = np.zeros((9, 9))
    for i in range(n):
        D = Ad[i] - (B[i - 1].T @ Y if i > 0 else 0.0)
        d0 = np.diagonal(Ad[i]).copy()
        M = np.concatenate([D, B[i]], axis=1)
        for k in range(9):
            piv = M[k, k]
            if not abs(piv) > 1e-10 * abs(d0[k]):
                return fl | ZERO_PIVOT
            if piv < 0.0:
                fl |= INDEFINITE
            M[k] /= piv
            rows = np.arange(9) != k
            M[rows] -= np.outer(M[rows, k], M[k])
        Y = M[:, 9:]
    return fl


def cpu_references(bands, lam32, s):
    """{name: (diag, super)} of the four fp64 references; ``s``: the chunk size of the partitioned one (s >= n: one chunk, the
    dense inverse of the whole chain -- what the sequential cases take)."""
    return {"inv": C.marginal_dense(bands, lam32, "inv"), "chol": C.marginal_dense(bands, lam32, "chol"),
            "blocks": C.marginal_blocks(bands, lam32), "partitioned": partitioned_fp64(bands, lam32, s)}


@dataclass
class Levels:
    ref: tuple                  # (diag, super) longdouble
    cpu: dict                   # {key: largest figure of the four fp64 references}
    by_ref: dict                # {name: worst figure of that reference}

    def bars(self, M):
        return {k: max(M * v, M * EPS) for k, v in self.cpu.items()}


def levels(bands, lam32, s, ref=None):
    """``ref``: the longdouble selected inverse of the same system, if the caller has it."""
    ref = ref or selected_inverse_ld(bands, lam32)
    cpu = dict.fromkeys(KEYS, 0.0)
    by_ref = {}
    for name, (d, sp) in cpu_references(bands, lam32, s).items():
        g = scaled_err(d, sp, *ref).groups
        by_ref[name] = max(v for v, _ in g.values())
        for k in KEYS:
            cpu[k] = max(cpu[k], g[k][0])
    return Levels(ref, cpu, by_ref)


@dataclass
class Verdict:
    err: Scaled
    bars: dict
    ratio: float                # largest over the groups of figure / max(CPU figure, 2^-52): the bar is M times the denominator
    ratio_at: str
    bad: list                   # ["diag vel-vel 3.1e-7 > 2.0e-12 at pose 4", ...]

    @property
    def ok(self):
        return not self.bad


def judge(got_diag, got_sup, lv, M):
    """(got_diag, got_sup) of one window against the longdouble reference of ``lv``, per group pair, by bars of M times the fp64
    references' own figures (floor M 2^-52)."""
    err = scaled_err(got_diag, got_sup, *lv.ref)
    bars = lv.bars(M)
    bad, ratio, at = [], 0.0, ""
    for k, (v, pose) in err.groups.items():
        r = v / max(lv.cpu[k], EPS)
        if r > ratio:
            ratio, at = r, f"{k} pose {pose}"
        if not v <= bars[k]:
            bad.append(f"{k} {v:.3e} > {bars[k]:.3e} ({r:.3g} x CPU) at pose {pose}")
    return Verdict(err, bars, ratio, at, bad)
