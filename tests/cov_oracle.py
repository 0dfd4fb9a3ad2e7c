"""NumPy restatements of the covariance query (vba_covariance): the symmetrised full-phase matrix from its bands, its inverse as a
dense matrix, and the selected inversion as a block recurrence for windows too big for a dense inverse."""
import numpy as np


def symmetrised_dense(bands, lam32=0.0):
    """bands [n,3,9,9] (sub, diag, super as VBA_DBG_BANDS / oracle assemble) -> (A + A^T) / 2 + lam32 I as a dense [9n, 9n]."""
    n = bands.shape[0]
    A = np.zeros((9 * n, 9 * n))
    for i in range(n):
        A[9 * i:9 * i + 9, 9 * i:9 * i + 9] = bands[i, 1]
        if i + 1 < n:
            A[9 * i:9 * i + 9, 9 * i + 9:9 * i + 18] = bands[i, 2]
        if i > 0:
            A[9 * i:9 * i + 9, 9 * i - 9:9 * i] = bands[i, 0]
    return 0.5 * (A + A.T) + lam32 * np.eye(9 * n)


def blocks_of(inv, n):
    """diag [n,9,9] and super [n,9,9] (block (i, i+1); zeros for the last pose) of a dense [9n, 9n]."""
    diag = np.stack([inv[9 * i:9 * i + 9, 9 * i:9 * i + 9] for i in range(n)])
    sup = np.zeros((n, 9, 9))
    for i in range(n - 1):
        sup[i] = inv[9 * i:9 * i + 9, 9 * i + 9:9 * i + 18]
    return diag, sup


def marginal_dense(bands, lam32=0.0, method="inv"):
    """Blocks of the inverse by a dense factorisation: method "inv" (LU), "chol" (Cholesky, identity columns), "solve"."""
    n = bands.shape[0]
    A = symmetrised_dense(bands, lam32)
    if method == "inv":
        inv = np.linalg.inv(A)
    elif method == "chol":
        L = np.linalg.cholesky(A)
        Li = np.linalg.solve(L, np.eye(9 * n))
        inv = Li.T @ Li
    else:
        inv = np.linalg.solve(A, np.eye(9 * n))
    return blocks_of(inv, n)


def marginal_blocks(bands, lam32=0.0):
    """The selected inversion as a block recurrence (the algorithm of csrc/vba_cov.hip, in NumPy):
    D_i = A_ii - B_{i-1}^T Y_{i-1}, Y_i = D_i^-1 B_i;  S_n-1 = D_n-1^-1, S_i,i+1 = -Y_i S_i+1, S_ii = D_i^-1 - S_i,i+1 Y_i^T."""
    n = bands.shape[0]
    Ad = 0.5 * (bands[:, 1] + bands[:, 1].transpose(0, 2, 1)) + lam32 * np.eye(9)
    B = np.zeros((n, 9, 9))
    B[:-1] = 0.5 * (bands[:-1, 2] + bands[1:, 0].transpose(0, 2, 1))
    Dinv = np.zeros((n, 9, 9))
    Y = np.zeros((n, 9, 9))
    for i in range(n):
        D = Ad[i] - (B[i - 1].T @ Y[i - 1] if i > 0 else 0.0)
        Dinv[i] = np.linalg.inv(D)
        Y[i] = Dinv[i] @ B[i]
    diag = np.zeros((n, 9, 9))
    sup = np.zeros((n, 9, 9))
    diag[n - 1] = Dinv[n - 1]
    for i in range(n - 2, -1, -1):
        sup[i] = -Y[i] @ diag[i + 1]
        diag[i] = Dinv[i] - sup[i] @ Y[i].T
    diag = 0.5 * (diag + diag.transpose(0, 2, 1))
    return diag, sup


def block_rel_err(got, ref):
    """Largest over poses of max|got_i - ref_i| / max|ref_i|."""
    num = np.abs(got - ref).reshape(got.shape[0], -1).max(1)
    den = np.maximum(np.abs(ref).reshape(ref.shape[0], -1).max(1), 1e-300)
    return float((num / den).max())


def sigma_rel_err(got, ref):
    """Per-component 1-sigma (sqrt of the diagonal) of every pose, largest relative error."""
    a = np.sqrt(np.abs(np.diagonal(got, axis1=-2, axis2=-1)))
    b = np.sqrt(np.abs(np.diagonal(ref, axis1=-2, axis2=-1)))
    return float((np.abs(a - b) / np.maximum(b, 1e-300)).max())
