// vba_schur_power_math.h -- the closed forms of the free-landmark outlier power query (vba_schur_outlier_power, vba_schur_power.hip),
// fp64, on top of the 2x2 forms of vba_power_math.h: the largest eigenvalue of a symmetric 3x3, the 3x3 adjugate solve, and the
// arithmetic of a row and of a catalogue prior.  Pure functions: the kernels call them on the device,
// tests/hostcheck/hostcheck_schur_power.cpp compiles them for the host and tests/test_schur_power_host.py compares them with LAPACK
// and with the reference of tests/schur_power_cases.py.
//
// A symmetric 3x3 is passed as (00, 01, 02, 11, 12, 22), as vba_schur_rel_math.h passes it.
#pragma once

#include "vba_math.h"
#include "vba_power_math.h"

namespace vba {

constexpr int kSym3Sweeps = 5;

// One Jacobi rotation on the pair (p, q) of a symmetric 3x3: app, aqq the diagonal, apq the entry it annihilates, arp, arq the
// entries of the third index against p and q.  t = tan of the angle is the smaller root, |t| <= 1: with d = aqq - app,
// t = 2 apq / (d + sign(d) sqrt(d^2 + 4 apq^2)), a sum of equal signs over a sum of squares.  An entry that is already 0 turns
// nothing (t = 0, also where d = 0 as well: the one select, and both of its sides are the limit of the other).
VBA_HD void sym3_rotate(double& app, double& aqq, double& apq, double& arp, double& arq) {
#pragma clang fp contract(off)
    const double d = aqq - app;
    const double h = sqrt(d * d + 4.0 * (apq * apq));
    const double den = d + copysign(h, d);
    const double t = den != 0.0 ? (apq + apq) / den : 0.0;
    const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.0;
    const double xp = c * arp - s * arq, xq = s * arp + c * arq;
    arp = xp;
    arq = xq;
}

// The largest eigenvalue of a symmetric 3x3 by kSym3Sweeps cyclic Jacobi sweeps, (0,1), (0,2), (1,2) each: the same fifteen
// rotations for every input, no branch on it and no eigenvector.  Convergence is quadratic, three sweeps reach rounding on a 3x3
// and the others cost nothing beside a row's gather.  Where eigenvalues coincide the rotations are arbitrary or none and the
// diagonal is right all the same (a multiple of I is returned as it came); a diagonal entry moves by t apq only, so an eigenvalue
// p -> 1 keeps the absolute accuracy of an ulp of |P|, which the trigonometric closed form (a difference of cubes under an acos)
// does not.  Input that is not finite gives NaN.
VBA_HD double sym3_mu_max(const double* m) {
    double a00 = m[0], a01 = m[1], a02 = m[2], a11 = m[3], a12 = m[4], a22 = m[5];
#pragma unroll
    for (int s = 0; s < kSym3Sweeps; ++s) {
        sym3_rotate(a00, a11, a01, a02, a12);
        sym3_rotate(a00, a22, a02, a01, a12);
        sym3_rotate(a11, a22, a12, a01, a02);
    }
    const double hi = a00 > a11 ? a00 : a11, mx = hi > a22 ? hi : a22;
    return (a00 == a00 && a11 == a11 && a22 == a22) ? mx : __builtin_nan("");
}

// z = scale M^-1 e for the symmetric 3x3 M by the cofactors rel_wtest3 forms, in its order; returns det M (the caller tests it).
VBA_HD double sym3_adj_solve(const double* m, const double* e, double scale, double* z) {
#pragma clang fp contract(off)
    const double c00 = m[0], c01 = m[1], c02 = m[2], c11 = m[3], c12 = m[4], c22 = m[5];
    const double a00 = c11 * c22 - c12 * c12, a01 = c02 * c12 - c01 * c22, a02 = c01 * c12 - c02 * c11;
    const double a11 = c00 * c22 - c02 * c02, a12 = c01 * c02 - c00 * c12, a22 = c00 * c11 - c01 * c01;
    const double det = c00 * a00 + c01 * a01 + c02 * a02;
    z[0] = scale * ((a00 * e[0] + a01 * e[1] + a02 * e[2]) / det);
    z[1] = scale * ((a01 * e[0] + a11 * e[1] + a12 * e[2]) / det);
    z[2] = scale * ((a02 * e[0] + a12 * e[1] + a22 * e[2]) / det);
    return det;
}

// The six figures of a row of non-zero weight w: P_k = [p00, p01; p01, p11], residual (ru, rv), and T = Sigma_k J_k^T (9x2: column
// u in tu, column v in tv; rows 0..2 position, 3..5 attitude, 6..8 the row's landmark), so B_k = w T.  out = mdb, ext_pos,
// ext_att, ext_lm, del_pos, del_lm.  R_k = I - P_k with det R_k <= 0 or mu_min(R_k) <= 0 (NaN included): NaN in all six.
VBA_HD void schur_pow_row(double w, double p00, double p01, double p11, double ru, double rv, const double* tu, const double* tv, double ncp,
                          double* out) {
#pragma clang fp contract(off)
    const double m00 = 1.0 - p00, m11 = 1.0 - p11, rb = -p01;
    const double det = fma(m00, m11, -(p01 * p01));                 // (as rel_wtest2 forms it)
    const double mu = sym2_mu_min(m00, rb, m11);
    double z0, z1;
    sym2_solve(m00, rb, m11, ru, rv, z0, z1);
    const bool ok = det > 0.0 && mu > 0.0;                          // (false for NaN)
    const double nan = __builtin_nan(""), scale = ncp / w;
    out[0] = ok ? sqrt(ncp / (w * mu)) : nan;
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        double g00 = 0.0, g01 = 0.0, g11 = 0.0, d2 = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double b0 = w * tu[3 * g + a], b1 = w * tv[3 * g + a];
            g00 = fma(b0, b0, g00);
            g01 = fma(b0, b1, g01);
            g11 = fma(b1, b1, g11);
            const double e = fma(b0, z0, b1 * z1);
            d2 = fma(e, e, d2);
        }
        const double ext = sqrt(scale * pair_mu_max(g00, g01, g11, m00, rb, m11));
        out[1 + g] = ok ? (g == 1 ? 2.0 * ext : ext) : nan;         // (attitude: the 2 |dtheta| convention)
        if (g != 1) out[g == 0 ? 4 : 5] = ok ? sqrt(d2) : nan;
    }
}

// Catalogue prior of a landmark with rows: P_l = Sigma_ll / sigma^2 (symmetric), p_max its largest eigenvalue, q = 1 - p_max.
// lm_mdb = sigma sqrt(ncp / q); lm_ext = sigma sqrt(ncp) p_max / sqrt(q): P_l and I - P_l commute, so the generalised eigenvalues
// of (P_l^T P_l, I - P_l) are p^2 / (1 - p) over the eigenvalues p of P_l, and p^2 / (1 - p) rises on [0, 1).  q <= 0 or not
// finite: NaN in both.
VBA_HD void schur_pow_prior(const double* P, double sigma, double ncp, double& lm_mdb, double& lm_ext) {
#pragma clang fp contract(off)
    const double pmax = sym3_mu_max(P), q = 1.0 - pmax;
    const bool ok = q > 0.0 && q <= 1.79e308;
    lm_mdb = ok ? sigma * sqrt(ncp / q) : __builtin_nan("");
    lm_ext = ok ? (sigma * sqrt(ncp)) * pmax / sqrt(q) : __builtin_nan("");
}

// |Sigma_il[0:3,:] z_l| with z_l = (I - P_l)^-1 e_l / sigma^2: how far the position of pose i moves if the prior of landmark l is
// taken away.  G3 = the first three rows of -Sigma_il (3x3 row major; the sign does not reach the norm).  det(I - P_l) <= 0: NaN.
VBA_HD double schur_pow_pull(const double* G3, const double* P, const double* e, double inv_sigma2) {
#pragma clang fp contract(off)
    const double mI[6] = {1.0 - P[0], -P[1], -P[2], 1.0 - P[3], -P[4], 1.0 - P[5]};
    double z[3];
    const double det = sym3_adj_solve(mI, e, inv_sigma2, z);
    double s2 = 0.0;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        const double x = G3[3 * p] * z[0] + G3[3 * p + 1] * z[1] + G3[3 * p + 2] * z[2];
        s2 = s2 + x * x;
    }
    return det > 0.0 ? sqrt(s2) : __builtin_nan("");
}

// det(I - P_l) as schur_pow_pull forms it
VBA_HD double schur_pow_prior_det(const double* P) {
    const double mI[6] = {1.0 - P[0], -P[1], -P[2], 1.0 - P[3], -P[4], 1.0 - P[5]};
    const double e[3] = {0.0, 0.0, 0.0};
    double z[3];
    return sym3_adj_solve(mI, e, 0.0, z);
}

}  // namespace vba
