// vba_schur_dyn.h -- what the units that build, step and cost a handle (vba_schur.hip, vba_schur_build.hip) and vba_schur_dyn.hip (the
// kernels of the orbit-dynamics factor of the free-landmark mode) share: the arrays of the factor and the launchers.  Internal.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vba {

struct SchurDynView {
    int n, Npad;
    double sigma;                   // sigma_dyn
    double lamda;                   // damping of the trial (velocity diagonal)
    const int* steps;               // [n - 1] one-second steps of edge i -> i + 1, each in 1 .. kSchurDynMaxGap (checked on the host); on a
                                    // handle of vba_schur_enable_dynamics_long a long edge holds MINUS its steps (vba_schur_dyn_long.h)
    double* r;                      // [n - 1][6] residual of the last build
    double* A;                      // [n - 1][36] D Phi of the last build, row major
    double* ecost;                  // [n - 1] sigma |r_e|^2 of the last build
    double* part;                   // [npart + nlong] block partials of the dynamics cost, one per 256 edges, then one per long edge
    int npart;
    double* S;                      // [Npad][Npad] the reduced system (lower triangle), N = 9 n
    double* g;                      // [Npad] right-hand side, then the step: [6 n of the poses | 3 n of the velocities]
    // long edges (vba_schur_dyn_long.hip; nlong = 0 on a handle without one: none of this is read)
    int nlong;
    int par;                        // parity of the pool the build reads its chains from (flips with every accepted trial)
    const int* long_idx;            // [nlong] pose i of long edge k, in index order
    const int* long_off;            // [nlong] offset of its slot in a pool, in states of six doubles
    double* long_pool;              // [2][long_pool_states][6] the chains, one pool per parity
    int long_pool_states;
};

inline int schur_dyn_partials(int n) { return (n - 1 + 255) / 256; }

// r, A, ecost at `states` [n][10]: six lanes per edge, one tangent column each
void schur_dyn_edges_launch(const SchurDynView& W, const double* states, hipStream_t s);
// the factor's blocks into S and g, after the reprojection kernels on the same stream; no atomics, fixed order
void schur_dyn_scatter_launch(const SchurDynView& W, hipStream_t s);
// the velocity columns of states_new = those of states + dv (after k_lm_update, which leaves them as they were)
void schur_dyn_update_launch(const SchurDynView& W, const double* states, double* states_new, hipStream_t s);
// part[b] = sum over the edges of block b of sigma |r_e|^2 at `states` (residual-only propagation), fixed order; a long edge adds nothing
void schur_dyn_cost_launch(const SchurDynView& W, const double* states, hipStream_t s);

// The Gauss-Newton attitude factor on top of it (vba_schur_enable_attitude; kernels: vba_schur_att.hip, bodies: vba_schur_att_math.h)
struct SchurAttView {
    int n, Npad;
    double sigma;                   // sigma_att
    const double* cumrot;           // [n][4] rotation accumulated over the gap after pose i (row n - 1 unused), checked on the host
    double* a;                      // [n - 1][3] residual of the last build
    double* J;                      // [n - 1][2][3][3] d a / d theta_i, then d a / d theta_{i+1}, of the last build
    double* ecost;                  // [n - 1] sigma |a_e|^2 of the last build
    double* part;                   // [npart] block partials of the attitude cost, one per 256 edges (schur_dyn_partials)
    int npart;
    double* S;                      // the reduced system and its right-hand side, as in SchurDynView
    double* g;
};

// a, J, ecost at `states` [n][10]: thread per edge
void schur_att_edges_launch(const SchurAttView& W, const double* states, hipStream_t s);
// the factor's blocks into S and g, after schur_dyn_scatter_launch on the same stream; no atomics, fixed order
void schur_att_scatter_launch(const SchurAttView& W, hipStream_t s);
// part[b] = sum over the edges of block b of sigma |a_e|^2 at `states`, fixed order
void schur_att_cost_launch(const SchurAttView& W, const double* states, hipStream_t s);

// The state prior factor on a handle with the dynamics factor (vba_schur_enable_state_prior; kernels: vba_schur_prior.hip, bodies:
// vba_schur_prior_math.h)
struct SchurPriorView {
    int n, Npad, count;
    const int* idx;                 // [count] pose of prior k: in 0 .. n - 1, no pose twice (checked on the host)
    const double* anchor;           // [count][10]
    const double* info;             // [count][81] Lambda, row major
    double* e;                      // [count][9] residual of the last build
    double* J;                      // [count][9] d (2 s eps) / d theta of the last build, row major
    double* LF;                     // [count][81] Lambda F of the last build
    double* Le;                     // [count][9] Lambda e of the last build
    double* share;                  // [count] e^T Lambda e of the last build
    double* part;                   // [npart] block partials of the prior's cost, one per 256 priors
    int npart;
    double* S;                      // the reduced system and its right-hand side, as in SchurDynView
    double* g;
};

// e, J, Lambda F, Lambda e, share at `states` [n][10]: thread per prior
void schur_prior_terms_launch(const SchurPriorView& W, const double* states, hipStream_t s);
// the factor's blocks into S and g, after the scatters of the other factors on the same stream; no atomics, one owner per entry
void schur_prior_scatter_launch(const SchurPriorView& W, hipStream_t s);
// part[b] = sum over the priors of block b of e^T Lambda e at `states`, fixed order
void schur_prior_cost_launch(const SchurPriorView& W, const double* states, hipStream_t s);

}  // namespace vba
