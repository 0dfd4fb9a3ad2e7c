// vba_schur_prior_math.h -- the state prior factor of the free-landmark mode (vba_schur_enable_state_prior) and the window hand-off
// that feeds it (vba_schur_handoff): the per-prior body, the index arithmetic of the scatter into the reduced system and the 9x9
// algebra of the hand-off, as host/device functions so that the CPU test-suite can compile and run them
// (tests/hostcheck/sanitize_schur_prior_main.cpp).  Internal.
//
// Model.  Coordinates are those of state_cov (vba_schur_covariance_dyn): x = [dp (km), dtheta, dv (km/s)], component c
// of pose i is unknown u(i, c) = 6 i + c for c < 6 and 6 n + 3 i + (c - 6) for c >= 6.  Quaternions scalar last, (x) = quat_mul.
// For prior k on pose i with anchor (pbar, qbar, vbar) and information matrix Lambda (symmetric, 9x9):
//     [eps, d] = conj(qbar) (x) q_i,   s = d >= 0 ? +1 : -1
//     e        = [p_i - pbar, 2 s eps, v_i - vbar]
//     F        = blockdiag(I, J, I),   J = d (2 s eps) / d theta_i = s (d I + [eps]x)
// along the mode's retraction q <- normalise(q (x) qexp(dtheta)) (vba_math.h: retract), so that J = I at q_i = +-qbar.
// Gauss-Newton:  H += F^T Lambda F,  g -= F^T Lambda e,  cost += e^T Lambda e.
//
// The hand-off propagates the 9x9 marginal Sigma of a pose over a gap: G = Phi on the [dp, dv] components and R on dtheta, R the
// matrix of dtheta' = conj(c) dtheta c (c the rotation accumulated over the gap: q (x) qexp(d) (x) c = (q (x) c) (x) qexp(conj(c) d c)),
// Sigma' = G Sigma G^T + steps diag(process noise per group), Lambda' = Sigma'^-1 by a Cholesky.
#pragma once

#include "vba_math.h"

namespace vba {

constexpr int kSchurPriorItems = 54;    // work items of the scatter per prior: 45 of S (lower triangle of the 9x9 block), 9 of g

// unknown of component c (0..8) of the state [dp, dtheta, dv] of pose i
VBA_HD int schur_prior_index(int n, int i, int c) { return c < 6 ? 6 * i + c : 6 * n + 3 * i + (c - 6); }

// e [9] of state st [10] against anchor an [10]; w [4] = conj(qbar) (x) q_i = [eps, d]
VBA_HD void schur_prior_residual(const double* st, const double* an, double* w, double* e) {
    const double cq[4] = {-an[3], -an[4], -an[5], an[6]};
    quat_mul(cq, st + 3, w);
    const double s2 = w[3] >= 0.0 ? 2.0 : -2.0;
    for (int k = 0; k < 3; ++k) {
        e[k] = st[k] - an[k];
        e[3 + k] = s2 * w[k];
        e[6 + k] = st[7 + k] - an[7 + k];
    }
}

// Le [9] = Lambda e (rows of Lambda, summed in index order); returns e^T Lambda e = sum_r e_r Le_r in index order
VBA_HD double schur_prior_cost(const double* L, const double* e, double* Le) {
    double c = 0.0;
    for (int r = 0; r < 9; ++r) {
        double s = 0.0;
        for (int k = 0; k < 9; ++k) s = fma(L[9 * r + k], e[k], s);
        Le[r] = s;
        c = fma(e[r], s, c);
    }
    return c;
}

// One prior: e [9], J [9] (row major 3x3), LF [81] = Lambda F, Le [9] = Lambda e; returns the cost share with the bits of
// schur_prior_cost
VBA_HD double schur_prior_terms(const double* st, const double* an, const double* L, double* e, double* J, double* LF, double* Le) {
    double w[4];
    schur_prior_residual(st, an, w, e);
    const double d = w[3], s = d >= 0.0 ? 1.0 : -1.0;
    J[0] = s * d;     J[1] = -s * w[2]; J[2] = s * w[1];
    J[3] = s * w[2];  J[4] = s * d;     J[5] = -s * w[0];
    J[6] = -s * w[1]; J[7] = s * w[0];  J[8] = s * d;
    for (int r = 0; r < 9; ++r)
        for (int c = 0; c < 9; ++c) {
            if (c < 3 || c >= 6) { LF[9 * r + c] = L[9 * r + c]; continue; }
            double v = 0.0;
            for (int k = 0; k < 3; ++k) v = fma(L[9 * r + 3 + k], J[3 * k + (c - 3)], v);
            LF[9 * r + c] = v;
        }
    return schur_prior_cost(L, e, Le);
}

// row a of F^T applied to a column x [9] read with stride ld:  (F^T x)_a
VBA_HD double schur_prior_ft_row(const double* J, const double* x, int ld, int a) {
    if (a < 3 || a >= 6) return x[(size_t)a * ld];
    double v = 0.0;
    for (int k = 0; k < 3; ++k) v = fma(J[3 * k + (a - 3)], x[(size_t)(3 + k) * ld], v);
    return v;
}

// Work item t (0 .. kSchurPriorItems - 1) of prior k on pose i of the scatter.  J [9], LF [81], Le [9] of that prior.  Every target
// entry of S and g belongs to exactly one item of exactly one prior (two priors on one pose are refused), which adds its share to
// what the reprojection kernels and the scatters of the other factors left there.
//   t < 45: entry (a, b), a >= b, of the 9x9 block of x_i in row order (0,0), (1,0), (1,1), (2,0) ..:  (F^T Lambda F)_ab at
//           (u(i, a), u(i, b)) -- u grows with the component, so this is the stored lower triangle: the lower triangles of the
//           pose and of the velocity block and the whole 3x6 velocity-pose block
//   t < 54: entry c = t - 45 of g at u(i, c):  -(F^T Lambda e)_c
VBA_HD void schur_prior_scatter_item(int n, int Npad, int i, int t, const double* J, const double* LF, const double* Le, double* S, double* g) {
    if (t < 45) {
        int a = 0, b = t;
        while (b > a) { b -= a + 1; ++a; }
        const int R = schur_prior_index(n, i, a), C = schur_prior_index(n, i, b);
        S[(size_t)R * Npad + C] += schur_prior_ft_row(J, LF + b, 9, a);
    } else if (t < kSchurPriorItems) {
        const int c = t - 45;
        g[schur_prior_index(n, i, c)] -= schur_prior_ft_row(J, Le, 1, c);
    }
}

// ---- the hand-off
// R [9] row major: the matrix of x -> vec(conj(c) (x) [x, 0] (x) c), column by column through the quaternion products themselves
VBA_HD void schur_handoff_rotation(const double* c, double* R) {
    const double cc[4] = {-c[0], -c[1], -c[2], c[3]};
    for (int k = 0; k < 3; ++k) {
        double u[4] = {0.0, 0.0, 0.0, 0.0}, t[4], o[4];
        u[k] = 1.0;
        quat_mul(cc, u, t);
        quat_mul(t, c, o);
        for (int r = 0; r < 3; ++r) R[3 * r + k] = o[r];
    }
}

// G [81] from Phi [36] (row major over (p, v)) and R [9]: Phi on the components {0, 1, 2, 6, 7, 8}, R on {3, 4, 5}
VBA_HD void schur_handoff_transition(const double* Phi, const double* R, double* G) {
    for (int k = 0; k < 81; ++k) G[k] = 0.0;
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) G[9 * (a < 3 ? a : a + 3) + (b < 3 ? b : b + 3)] = Phi[6 * a + b];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) G[9 * (3 + a) + 3 + b] = R[3 * a + b];
}

// out = G Sigma G^T + steps diag(noise[group]), group = component / 3 (position, attitude, velocity); T [81] is work space.  The
// lower triangle is computed and mirrored: exactly symmetric.
VBA_HD void schur_handoff_congruence(const double* G, const double* Sigma, int steps, const double* noise, double* T, double* out) {
    for (int a = 0; a < 9; ++a)
        for (int b = 0; b < 9; ++b) {
            double s = 0.0;
            for (int k = 0; k < 9; ++k) s = fma(G[9 * a + k], Sigma[9 * k + b], s);
            T[9 * a + b] = s;
        }
    for (int a = 0; a < 9; ++a)
        for (int b = 0; b <= a; ++b) {
            double s = 0.0;
            for (int k = 0; k < 9; ++k) s = fma(T[9 * a + k], G[9 * b + k], s);
            if (a == b) s += (double)steps * noise[a / 3];
            out[9 * a + b] = s;
            out[9 * b + a] = s;
        }
}

// inv = A^-1 of a symmetric positive definite 9x9 by A = L L^T, W = L^-1, A^-1 = W^T W; the lower triangle is computed and mirrored.
// L and W [81] are work space.  false (inv untouched) if a pivot is not positive and finite.
VBA_HD bool schur_handoff_cholinv(const double* A, double* L, double* W, double* inv) {
    for (int k = 0; k < 81; ++k) { L[k] = 0.0; W[k] = 0.0; }
    for (int j = 0; j < 9; ++j) {
        double d = A[9 * j + j];
        for (int k = 0; k < j; ++k) d = fma(-L[9 * j + k], L[9 * j + k], d);
        if (!(d > 0.0) || !(d <= 1.7976931348623157e308)) return false;
        const double lj = sqrt(d);
        L[9 * j + j] = lj;
        for (int r = j + 1; r < 9; ++r) {
            double s = A[9 * r + j];
            for (int k = 0; k < j; ++k) s = fma(-L[9 * r + k], L[9 * j + k], s);
            L[9 * r + j] = s / lj;
        }
    }
    for (int c = 0; c < 9; ++c) {           // column c of W: L w = e_c
        for (int r = c; r < 9; ++r) {
            double s = r == c ? 1.0 : 0.0;
            for (int k = c; k < r; ++k) s = fma(-L[9 * r + k], W[9 * k + c], s);
            W[9 * r + c] = s / L[9 * r + r];
        }
    }
    for (int a = 0; a < 9; ++a)
        for (int b = 0; b <= a; ++b) {
            double s = 0.0;
            for (int k = a; k < 9; ++k) s = fma(W[9 * k + a], W[9 * k + b], s);
            inv[9 * a + b] = s;
            inv[9 * b + a] = s;
        }
    return true;
}

}  // namespace vba
