// vba_schur_dyn_math.h -- the orbit-dynamics factor of the free-landmark mode (vba_schur_enable_dynamics): the per-edge body and the
// index arithmetic of the scatter into the reduced system, as host/device functions so that the CPU test-suite can compile and run
// them (tests/hostcheck/sanitize_schur_dyn_main.cpp).  Internal.
//
// Model (oracle/ba_oracle.py: orbit_factor and the orbit part of assemble, restated without the fixed-landmark path's wmax_scale).
// For every edge e = (i -> i + 1) with steps_e = time_idx[i + 1] - time_idx[i] one-second RK4 steps of the J2 model:
//     r_e = D (propagate(p_i, v_i; steps_e) - (p_{i+1}, v_{i+1})),   D = diag(1, 1, 1, kVelCoeff, kVelCoeff, kVelCoeff)
//     J_e = [A_e at pose i | -D at pose i + 1],   A_e = D Phi_e
// Gauss-Newton with weight sigma:  H += sigma J^T J,  g -= sigma J^T r,  cost += sigma |r|^2.
// The ATTITUDE factor of the fixed-landmark path is NOT part of this mode: its Newton blocks (Hd, Hu, Hl) are not symmetric and the
// reduced system of this mode is factorised by a Cholesky.  (vba_schur_att_math.h: the Gauss-Newton statement that is.)
//
// Unknowns of the reduced system: [6 n pose unknowns (dp, dtheta per pose) | 3 n velocity unknowns]; component c of the dynamics
// state x_i = (p_i, v_i) is unknown 6 i + c for c < 3 and 6 n + 3 i + (c - 3) for c >= 3.  Only the lower triangle is stored: an
// entry (R, C) with R < C goes to (C, R) -- that is where the block (p_{i+1}, v_i) lands transposed at (v_i, p_{i+1}).
#pragma once

#include "vba_math.h"

namespace vba {

// the domain of the sequential propagation (k_sdyn_edges, k_sdyn_cost) and all that vba_schur_enable_dynamics accepts; longer gaps, up
// to VBA_MAX_GAP, are vba_schur_enable_dynamics_long's: parallel in time, vba_schur_dyn_long.hip
constexpr int kSchurDynMaxGap = 64;
constexpr int kSchurDynItems = 78;      // work items of the scatter per pose: 36 diagonal, 36 sub-diagonal block entries, 6 of g

VBA_HD double schur_dyn_d(int c) { return c < 3 ? 1.0 : kVelCoeff; }

// unknown of component c (0..5) of the dynamics state of pose i
VBA_HD int schur_dyn_index(int n, int i, int c) { return c < 3 ? 6 * i + c : 6 * n + 3 * i + (c - 3); }

// Column c of an edge: the start state st [10] of pose i over `steps` one-second steps with the tangent e_c.  xhat [6] is the
// prediction (the same bits whatever c), col [6] = column c of A = D Phi.
VBA_HD void schur_dyn_edge_column(const double* st, int steps, int c, double* xhat, double* col) {
    double x[6] = {st[0], st[1], st[2], st[7], st[8], st[9]};
    double t[6] = {0, 0, 0, 0, 0, 0};
    t[c] = 1.0;
    propagate_gap<true>(x, t, steps, 0);
    for (int r = 0; r < 6; ++r) { xhat[r] = x[r]; col[r] = r < 3 ? t[r] : t[r] * kVelCoeff; }
}

// the same lane without D: col [6] = column c of Phi itself (vba_schur_handoff propagates a covariance with it)
VBA_HD void schur_dyn_phi_column(const double* st, int steps, int c, double* xhat, double* col) {
    double x[6] = {st[0], st[1], st[2], st[7], st[8], st[9]};
    double t[6] = {0, 0, 0, 0, 0, 0};
    t[c] = 1.0;
    propagate_gap<true>(x, t, steps, 0);
    for (int r = 0; r < 6; ++r) { xhat[r] = x[r]; col[r] = t[r]; }
}

// the prediction alone (the cost of a trial state)
VBA_HD void schur_dyn_predict(const double* st, int steps, double* xhat) {
    double x[6] = {st[0], st[1], st[2], st[7], st[8], st[9]};
    propagate_gap<false>(x, nullptr, steps, 0);
    for (int r = 0; r < 6; ++r) xhat[r] = x[r];
}

// r = D (xhat - x_next) from the next pose's state sn [10]; returns |r|^2 summed in index order
VBA_HD double schur_dyn_residual(const double* xhat, const double* sn, double* r) {
    r[0] = xhat[0] - sn[0];
    r[1] = xhat[1] - sn[1];
    r[2] = xhat[2] - sn[2];
    r[3] = (xhat[3] - sn[7]) * kVelCoeff;
    r[4] = (xhat[4] - sn[8]) * kVelCoeff;
    r[5] = (xhat[5] - sn[9]) * kVelCoeff;
    double s = 0.0;
    for (int k = 0; k < 6; ++k) s = fma(r[k], r[k], s);
    return s;
}

// Work item t (0 .. kSchurDynItems - 1) of pose i of the scatter.  A [n-1][36] (row major D Phi per edge), r [n-1][6].  Every
// target entry of S and g belongs to exactly one item; an item adds the share of edge i - 1 (pose i is its end), then the share
// of edge i (pose i is its start), in that order, to what the reprojection kernels left there.  lamda goes on the velocity
// diagonal (the pose diagonal got it from the reprojection build).
//   t <  36: entry (a, b) = (t / 6, t % 6) of the diagonal block of x_i, lower part (a >= b):  sigma D_a^2 [a == b]  +  sigma (A_i^T A_i)_ab
//   t <  72: entry (a, b) of the block (x_i, x_{i-1}), i > 0:  -sigma D_a A_{i-1}[a][b]
//   t <  78: entry c = t - 72 of g at x_i:  sigma D_c r_{i-1}[c]  -  sigma (A_i^T r_i)_c
VBA_HD void schur_dyn_scatter_item(int n, int Npad, int i, int t, double sigma, double lamda, const double* A, const double* r,
                                   double* S, double* g) {
    if (t < 36) {
        const int a = t / 6, b = t % 6;
        if (a < b) return;
        const int R = schur_dyn_index(n, i, a), C = schur_dyn_index(n, i, b);      // (R >= C: the index grows with the component)
        double v = S[(size_t)R * Npad + C];
        if (a == b && a >= 3) v += lamda;
        if (i > 0 && a == b) v += sigma * (schur_dyn_d(a) * schur_dyn_d(a));
        if (i < n - 1) {
            const double* Ai = A + (size_t)i * 36;
            double s = 0.0;
            for (int k = 0; k < 6; ++k) s = fma(Ai[6 * k + a], Ai[6 * k + b], s);
            v += sigma * s;
        }
        S[(size_t)R * Npad + C] = v;
    } else if (t < 72) {
        if (i == 0) return;
        const int a = (t - 36) / 6, b = (t - 36) % 6;
        const int R = schur_dyn_index(n, i, a), C = schur_dyn_index(n, i - 1, b);
        const double v = -(sigma * (schur_dyn_d(a) * A[(size_t)(i - 1) * 36 + 6 * a + b]));
        if (R >= C) S[(size_t)R * Npad + C] += v;
        else S[(size_t)C * Npad + R] += v;          // (p_i, v_{i-1}) is stored transposed at (v_{i-1}, p_i)
    } else if (t < kSchurDynItems) {
        const int c = t - 72;
        const int R = schur_dyn_index(n, i, c);
        double v = g[R];
        if (i > 0) v += sigma * (schur_dyn_d(c) * r[(size_t)(i - 1) * 6 + c]);
        if (i < n - 1) {
            const double* Ai = A + (size_t)i * 36;
            const double* ri = r + (size_t)i * 6;
            double s = 0.0;
            for (int k = 0; k < 6; ++k) s = fma(Ai[6 * k + c], ri[k], s);
            v -= sigma * s;
        }
        g[R] = v;
    }
}

}  // namespace vba
