// vba_schur_dyn_rel.h -- the closed form of the edge leverage of vba_schur_reliability_dyn (vba_schur_rel.hip: k_rel_edges), as
// host/device functions so that the CPU test-suite can compile and run them (tests/hostcheck/sanitize_schur_dyn_rel_main.cpp).
// Internal.
//
// Edge i (pose i -> pose i + 1) of the dynamics factor is a 6-row observation of weight sigma_dyn with the Jacobian
//     J_i = [A_i | -D]   (6 x 12)   over   x = [dp_i, dv_i, dp_{i+1}, dv_{i+1}],   A_i = D Phi_i,   D = diag(1, 1, 1, kVelCoeff ...)
// (vba_schur_dyn_math.h).  Its covariance Sigma12 (12 x 12) is read from the outputs of vba_schur_covariance_dyn: components
// {0, 1, 2, 6, 7, 8} of state_cov[i] (top left), edge_cov[i] (top right: rows of pose i, columns of pose i + 1; bottom left its
// transpose) and state_cov[i + 1] (bottom right).
//     leverage_i = sigma_dyn tr(J_i Sigma12 J_i^T),  in (0, 6]
// There is NO w-test of an edge: at the weights of this project I - P_e is singular to rounding (vinsat_ba.h says why).
#pragma once

#include "vba_math.h"

namespace vba {

// component a (0 .. 5) of the dynamics state (p, v) in the 9-vector [dp, dtheta, dv] of vba_schur_covariance_dyn
VBA_HD int schur_dyn_rel_comp(int a) { return a < 3 ? a : a + 3; }

// Sigma12[a][b], a, b in 0 .. 11, from the three 9x9 blocks
VBA_HD double schur_dyn_rel_sigma(const double* st_i, const double* ed_i, const double* st_n, int a, int b) {
    const int ca = schur_dyn_rel_comp(a % 6), cb = schur_dyn_rel_comp(b % 6);
    if (a < 6) return b < 6 ? st_i[9 * ca + cb] : ed_i[9 * ca + cb];
    return b < 6 ? ed_i[9 * cb + ca] : st_n[9 * ca + cb];
}

// Diagonal entry c (0 .. 5) of J Sigma12 J^T.  Row c of J is (A[c][0 .. 5], then -D_c at column 6 + c and zeros): t_b = the row
// against column b of Sigma12, the A part a upwards and the -D term last; then the dot product with the row itself, b upwards,
// the -D term last.  Only the seven columns the row is non-zero at are formed.  A: the edge's D Phi [36], row major.
VBA_HD double schur_dyn_rel_edge_diag(const double* A, const double* st_i, const double* ed_i, const double* st_n, int c) {
    const double* Ac = A + 6 * c;
    const double md = -(c < 3 ? 1.0 : kVelCoeff);
    double d = 0.0, t = 0.0;
    for (int b = 0; b < 7; ++b) {
        const int col = b < 6 ? b : 6 + c;
        double s = 0.0;
        for (int a = 0; a < 6; ++a) s = fma(Ac[a], schur_dyn_rel_sigma(st_i, ed_i, st_n, a, col), s);
        s = fma(md, schur_dyn_rel_sigma(st_i, ed_i, st_n, 6 + c, col), s);
        if (b < 6) d = fma(s, Ac[b], d);
        else t = s;
    }
    return fma(t, md, d);
}

// the trace from the six diagonal entries, in index order, times the weight
VBA_HD double schur_dyn_rel_edge_leverage(double sigma, const double* diag) {
    return sigma * (((((diag[0] + diag[1]) + diag[2]) + diag[3]) + diag[4]) + diag[5]);
}

}  // namespace vba
