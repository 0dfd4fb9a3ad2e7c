// vba_schur_att_rel.h -- the closed forms of one attitude edge of vba_schur_reliability_att (vba_schur_rel.hip: k_rel_att_edges), as
// host/device functions so that the CPU test-suite can compile and run them (tests/hostcheck/sanitize_schur_att_rel_main.cpp).
// Internal.
//
// Edge i (pose i -> pose i + 1) of the attitude factor is a 3-row observation of weight sigma_att with the Jacobian
//     J_i = [J_own | J_next]   (3 x 6)   over   x = [dtheta_i, dtheta_{i+1}]      (vba_schur_att_math.h; J [kSchurAttJ] row major,
//                                                                                  J_own first)
// and the residual a_i.  Its covariance Sigma6 (6 x 6) is read from the outputs of vba_schur_covariance_dyn: components {3, 4, 5} of
// state_cov[i] (top left), edge_cov[i] (top right: rows of pose i, columns of pose i + 1; bottom left its transpose, read from the
// same stored block as k_rel_edges reads it) and state_cov[i + 1] (bottom right).
//     P_a        = sigma_att J_i Sigma6 J_i^T                                  (3 x 3)
//     leverage_i = tr P_a  in (0, 3]                                           (each diagonal entry on its own, summed in index order)
//     wtest_i    = sqrt(sigma_att a_i^T (I - P_a)^-1 a_i)                      (symmetric part of I - P_a; rel_wtest3: cofactors, NaN
//                                                                               where the determinant is not positive or the form negative)
// Unlike the orbit edge (vba_schur_dyn_rel.h) the attitude edge keeps nearly all of its redundancy: I - P_a is well conditioned
// (smallest eigenvalue >= 0.49 on every case of the test-suite), so the w-test is returned.
#pragma once

#include "vba_math.h"
#include "vba_schur_rel_math.h"

namespace vba {

// Sigma6[a][b], a, b in 0 .. 5, from the three 9x9 blocks
VBA_HD double schur_att_rel_sigma(const double* st_i, const double* ed_i, const double* st_n, int a, int b) {
    const int ca = 3 + a % 3, cb = 3 + b % 3;
    if (a < 3) return b < 3 ? st_i[9 * ca + cb] : ed_i[9 * ca + cb];
    return b < 3 ? ed_i[9 * cb + ca] : st_n[9 * ca + cb];
}

// P [9] = sigma J Sigma6 J^T, row major.  Row r of J against the six columns of Sigma6 (a upwards: the J_own half, then the J_next
// half), then that row against the rows of J (b upwards).  J: the edge's pair [kSchurAttJ], J_own [3][3] then J_next [3][3].
VBA_HD void schur_att_rel_P(const double* J, const double* st_i, const double* ed_i, const double* st_n, double sigma, double* P) {
    double S6[36];
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) S6[6 * a + b] = schur_att_rel_sigma(st_i, ed_i, st_n, a, b);
    for (int r = 0; r < 3; ++r) {
        double t[6];
        for (int b = 0; b < 6; ++b) {
            double s = 0.0;
            for (int a = 0; a < 3; ++a) s = fma(J[3 * r + a], S6[6 * a + b], s);
            for (int a = 0; a < 3; ++a) s = fma(J[9 + 3 * r + a], S6[6 * (3 + a) + b], s);
            t[b] = s;
        }
        for (int c = 0; c < 3; ++c) {
            double s = 0.0;
            for (int b = 0; b < 3; ++b) s = fma(t[b], J[3 * c + b], s);
            for (int b = 0; b < 3; ++b) s = fma(t[3 + b], J[9 + 3 * c + b], s);
            P[3 * r + c] = sigma * s;
        }
    }
}

// the trace, in index order
VBA_HD double schur_att_rel_leverage(const double* P) { return (P[0] + P[4]) + P[8]; }

// sqrt(sigma a^T (I - P)^-1 a) with the symmetric part of I - P, by rel_wtest3
VBA_HD double schur_att_rel_wtest(const double* P, const double* a, double sigma) {
    const double m[6] = {1.0 - P[0],          -(0.5 * (P[1] + P[3])), -(0.5 * (P[2] + P[6])),
                         1.0 - P[4],          -(0.5 * (P[5] + P[7])), 1.0 - P[8]};
    return rel_wtest3(m, a, sigma);
}

}  // namespace vba
