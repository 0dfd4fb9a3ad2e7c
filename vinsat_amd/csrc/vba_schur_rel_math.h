// vba_schur_rel_math.h -- the closed forms of the free-landmark reliability query (vba_schur_reliability, vba_schur.hip), fp64:
// the w-test of a 2-vector and of a 3-vector against a symmetric matrix I - P, by the adjugate over the determinant.  Pure
// functions: the kernels call them on the device, tests/hostcheck/hostcheck_schur_rel.cpp compiles them for the host and
// tests/test_schur_rel_host.py compares them with LAPACK.
//
// Degenerate input follows vba_reliability (vba_rowpass.h, row_lev_wtest): a determinant that is not positive, or a quadratic
// form that is negative or not finite, gives NaN -- I - P is then not the positive definite matrix the test presumes.
#pragma once

#include "vba_math.h"

namespace vba {

// sqrt(w r^T (I - P)^-1 r) for the symmetric P = [p00, p01; p01, p11] and r = (ru, rv)
VBA_HD double rel_wtest2(double p00, double p01, double p11, double ru, double rv, double w) {
#pragma clang fp contract(off)
    const double m00 = 1.0 - p00, m11 = 1.0 - p11;
    const double det = fma(m00, m11, -(p01 * p01));
    // (I - P)^-1 = [m11, p01; p01, m00] / det
    const double ruv = ru * rv;
    const double qf = fma(rv * rv, m00, fma(ruv + ruv, p01, (ru * ru) * m11)) / det;
    const double t2 = w * qf;
    return (det > 0.0 && t2 >= 0.0 && t2 <= 1.79e308) ? sqrt(t2) : __builtin_nan("");
}

// sqrt(scale e^T M^-1 e) for the symmetric 3x3 M given as (00, 01, 02, 11, 12, 22): cofactors, as k_lm_blocks inverts C_l
VBA_HD double rel_wtest3(const double* m, const double* e, double scale) {
#pragma clang fp contract(off)
    const double c00 = m[0], c01 = m[1], c02 = m[2], c11 = m[3], c12 = m[4], c22 = m[5];
    const double a00 = c11 * c22 - c12 * c12, a01 = c02 * c12 - c01 * c22, a02 = c01 * c12 - c02 * c11;
    const double a11 = c00 * c22 - c02 * c02, a12 = c01 * c02 - c00 * c12, a22 = c00 * c11 - c01 * c01;
    const double det = c00 * a00 + c01 * a01 + c02 * a02;
    const double z0 = a00 * e[0] + a01 * e[1] + a02 * e[2];
    const double z1 = a01 * e[0] + a11 * e[1] + a12 * e[2];
    const double z2 = a02 * e[0] + a12 * e[1] + a22 * e[2];
    const double t2 = scale * ((e[0] * z0 + e[1] * z1 + e[2] * z2) / det);
    return (det > 0.0 && t2 >= 0.0 && t2 <= 1.79e308) ? sqrt(t2) : __builtin_nan("");
}

}  // namespace vba
