// vba_schur_att_math.h -- the Gauss-Newton attitude factor of the free-landmark mode (vba_schur_enable_attitude): the per-edge body
// and the index arithmetic of the scatter into the reduced system, as host/device functions so that the CPU test-suite can compile
// and run them (tests/hostcheck/sanitize_schur_att_main.cpp).  Internal.
//
// Model.  Quaternions scalar last, (x) = quat_mul.  For every edge e = (i -> i + 1), c_i = cumrot[i] the rotation
// accumulated over the gap after pose i:
//     qp_i   = q_i (x) c_i
//     [e, d] = conj(qp_i) (x) q_{i+1}            (d is the reference's d = <qp_i, q_{i+1}>, BA_utils.py:481-487)
//     s      = d >= 0 ? +1 : -1
//     a_i    = s e                                (3-vector; |a_i|^2 = 1 - d^2 on unit quaternions)
//     J_next = d a_i / d theta_{i+1} =  1/2 s (d I + [e]x)
//     J_own  = d a_i / d theta_i     = -1/2 s (L(conj c_i) R(m_i))[0:3, 0:3],   m_i = conj(q_i) (x) q_{i+1}
// with L(p) q = p (x) q, R(m) q = q (x) m, along the mode's own retraction q <- normalise(q (x) qexp(dtheta)) (vba_math.h: retract;
// qexp is the half-angle exponential, hence the 1/2).  Gauss-Newton with weight sigma_att:  H += sigma J^T J,  g -= sigma J^T a,
// cost += sigma |a|^2 -- symmetric positive semidefinite, where the fixed-landmark path's Newton blocks (attitude_term) are not.
// The reference's term is sigma kQuatCoeff (1 - |d|) = sigma kQuatCoeff |a|^2 / (1 + |d|): sigma_att = sigma_dyn kQuatCoeff / 2
// weights the attitude as the reference does near the solution (the caller's choice: sigma_att is an argument).
//
// The attitude unknowns of pose i are 6 i + 3 .. 6 i + 5 of the reduced system [6 n pose | 3 n velocity]; the block
// (theta_{i+1}, theta_i) lies in the stored lower triangle as it is.
#pragma once

#include "vba_math.h"

namespace vba {

constexpr int kSchurAttItems = 21;      // work items of the scatter per pose: 9 diagonal (6 at work), 9 sub-diagonal block entries, 3 of g
constexpr int kSchurAttJ = 18;          // doubles of an edge's Jacobian pair: J_own [3][3], then J_next [3][3], row major

// w [4] = conj(q_i (x) c) (x) q_next = [e, d], a [3] = s e; returns |a|^2 summed in index order
VBA_HD double schur_att_residual(const double* qi, const double* c, const double* qn, double* w, double* a) {
    double qp[4];
    quat_mul(qi, c, qp);
    const double cq[4] = {-qp[0], -qp[1], -qp[2], qp[3]};
    quat_mul(cq, qn, w);
    const double s = w[3] >= 0.0 ? 1.0 : -1.0;
    double n2 = 0.0;
    for (int k = 0; k < 3; ++k) { a[k] = s * w[k]; n2 = fma(a[k], a[k], n2); }
    return n2;
}

// One edge: a [3], J [kSchurAttJ] (J_own, then J_next), returns |a|^2 with the bits of schur_att_residual
VBA_HD double schur_att_edge(const double* qi, const double* c, const double* qn, double* a, double* J) {
    double w[4];
    const double n2 = schur_att_residual(qi, c, qn, w, a);
    const double d = w[3], s = d >= 0.0 ? 1.0 : -1.0, hs = 0.5 * s;
    double* Jn = J + 9;
    Jn[0] = hs * d;     Jn[1] = -hs * w[2]; Jn[2] = hs * w[1];
    Jn[3] = hs * w[2];  Jn[4] = hs * d;     Jn[5] = -hs * w[0];
    Jn[6] = -hs * w[1]; Jn[7] = hs * w[0];  Jn[8] = hs * d;
    const double ci[4] = {-qi[0], -qi[1], -qi[2], qi[3]}, cc[4] = {-c[0], -c[1], -c[2], c[3]};
    double m[4];
    quat_mul(ci, qn, m);
    for (int k = 0; k < 3; ++k) {           // column k: conj(c) (x) (e_k (x) m)
        double u[4] = {0.0, 0.0, 0.0, 0.0}, t[4], o[4];
        u[k] = 1.0;
        quat_mul(u, m, t);
        quat_mul(cc, t, o);
        for (int r = 0; r < 3; ++r) J[3 * r + k] = -hs * o[r];
    }
    return n2;
}

// (X^T Y)_ab of two row-major 3x3 blocks, summed in row order
VBA_HD double schur_att_xty(const double* X, const double* Y, int a, int b) {
    double s = 0.0;
    for (int k = 0; k < 3; ++k) s = fma(X[3 * k + a], Y[3 * k + b], s);
    return s;
}

// Work item t (0 .. kSchurAttItems - 1) of pose i of the scatter.  J [n-1][kSchurAttJ], av [n-1][3].  Every target entry of S and g
// belongs to exactly one item; an item adds the share of edge i - 1 (pose i is its end: J_next), then the share of edge i (pose i is
// its start: J_own), in that order, to what the reprojection kernels and the orbit factor's scatter left there.
//   t <  9: entry (a, b) = (t / 3, t % 3) of the block (theta_i, theta_i), lower part (a >= b):
//           sigma (J_next_{i-1}^T J_next_{i-1})_ab  +  sigma (J_own_i^T J_own_i)_ab
//   t < 18: entry (a, b) of the block (theta_i, theta_{i-1}), i > 0:  sigma (J_next_{i-1}^T J_own_{i-1})_ab
//   t < 21: entry c = t - 18 of g at theta_i:  -sigma (J_next_{i-1}^T a_{i-1})_c  -  sigma (J_own_i^T a_i)_c
VBA_HD void schur_att_scatter_item(int n, int Npad, int i, int t, double sigma, const double* J, const double* av, double* S, double* g) {
    const double* Jp = i > 0 ? J + (size_t)(i - 1) * kSchurAttJ : nullptr;         // edge i - 1
    const double* Ji = i < n - 1 ? J + (size_t)i * kSchurAttJ : nullptr;           // edge i
    if (t < 9) {
        const int a = t / 3, b = t % 3;
        if (a < b) return;
        const size_t at = (size_t)(6 * i + 3 + a) * Npad + (6 * i + 3 + b);
        double v = S[at];
        if (Jp) v += sigma * schur_att_xty(Jp + 9, Jp + 9, a, b);
        if (Ji) v += sigma * schur_att_xty(Ji, Ji, a, b);
        S[at] = v;
    } else if (t < 18) {
        if (!Jp) return;
        const int a = (t - 9) / 3, b = (t - 9) % 3;
        S[(size_t)(6 * i + 3 + a) * Npad + (6 * (i - 1) + 3 + b)] += sigma * schur_att_xty(Jp + 9, Jp, a, b);
    } else if (t < kSchurAttItems) {
        const int c = t - 18;
        double v = g[6 * i + 3 + c];
        if (Jp) {
            const double* ap = av + (size_t)(i - 1) * 3;
            double s = 0.0;
            for (int k = 0; k < 3; ++k) s = fma(Jp[9 + 3 * k + c], ap[k], s);
            v -= sigma * s;
        }
        if (Ji) {
            const double* ai = av + (size_t)i * 3;
            double s = 0.0;
            for (int k = 0; k < 3; ++k) s = fma(Ji[3 * k + c], ai[k], s);
            v -= sigma * s;
        }
        g[6 * i + 3 + c] = v;
    }
}

}  // namespace vba
