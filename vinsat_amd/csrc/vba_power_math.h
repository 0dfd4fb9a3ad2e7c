// vba_power_math.h -- the closed forms of the outlier power query (vba_outlier_power, vba_power.hip) on symmetric 2x2 matrices,
// fp64.  Pure functions: the row pass calls them on the device, tests/hostcheck/hostcheck_power.cpp compiles them for the host
// and compares them with LAPACK (tests/test_outlier_power_host.py).
//
// A symmetric 2x2 [a, b; b, d] is passed as its three numbers.  No function here branches on its input, so every result is a
// continuous function of it: coincident eigenvalues (b = 0, a = d) need no tie rule, and no eigenvector is formed.
#pragma once

#include "vba_math.h"

namespace vba {

// The smaller eigenvalue of [a, b; b, d]: (tr - sqrt((a - d)^2 + 4 b^2)) / 2.  The discriminant is a sum of squares (no
// cancellation); what remains is the difference tr - sqrt(...), whose relative error is that of a number of size |mu_max|:
// the result is good to an ulp of the LARGER eigenvalue, which is the conditioning of the smaller one.
VBA_HD double sym2_mu_min(double a, double b, double d) {
    const double h = a - d;
    return 0.5 * ((a + d) - sqrt(h * h + 4.0 * (b * b)));
}

// The larger eigenvalue, same form with the other sign: no cancellation at all for a positive semi-definite matrix.
VBA_HD double sym2_mu_max(double a, double b, double d) {
    const double h = a - d;
    return 0.5 * ((a + d) + sqrt(h * h + 4.0 * (b * b)));
}

// z = R^-1 r for R = [a, b; b, d]: the adjugate over the determinant.
VBA_HD void sym2_solve(double a, double b, double d, double r0, double r1, double& z0, double& z1) {
    const double det = a * d - b * b;
    z0 = (d * r0 - b * r1) / det;
    z1 = (a * r1 - b * r0) / det;
}

// The larger root mu of det(M - mu R) = 0 for symmetric M = [m00, m01; m01, m11] (positive semi-definite) and R = [a, b; b, d]
// (positive definite): the quadratic det(R) mu^2 - tr(M adj R) mu + det(M) = 0.  Its discriminant tr(M adj R)^2 - 4 det R det M
// cancels to nothing where the two roots meet, so the quadratic is solved in the coordinates that make R the identity: with the
// 2x2 Cholesky factor R = L L^T in closed form, N = L^-1 M L^-T is symmetric, has the same roots, and its discriminant is the
// sum of squares (n00 - n11)^2 + 4 n01^2.  R not positive definite gives NaN (the square root of a negative number) or inf; the
// caller tests det R and mu_min(R) itself.
VBA_HD double pair_mu_max(double m00, double m01, double m11, double a, double b, double d) {
    const double l00 = sqrt(a), l10 = b / l00, l11 = sqrt(d - l10 * l10);
    // X = L^-1 M, then N = X L^-T (n10 = n01: one triangle)
    const double x01 = m01 / l00, x11 = (m11 - l10 * x01) / l11;
    const double n00 = m00 / a, n01 = (x01 - l10 * n00) / l11, n11 = (x11 - l10 * n01) / l11;
    return sym2_mu_max(n00, n01, n11);
}

}  // namespace vba
