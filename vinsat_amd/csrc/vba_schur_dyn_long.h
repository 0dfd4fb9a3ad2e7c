// vba_schur_dyn_long.h -- long gaps of the orbit-dynamics factor of the free-landmark mode (vba_schur_enable_dynamics_long; kernels:
// vba_schur_dyn_long.hip): what the host plans when the factor is enabled -- which edges are long, where their chains live, how many
// cost partials the handle sums, how large the chain pool is -- as a host function that the CPU test-suite compiles and runs
// (tests/hostcheck/sanitize_schur_dyn_long_main.cpp), and the launchers of the kernels.  Internal.
//
// An edge is long when it spans more than kSchurDynLongGap one-second steps (the threshold of the fixed-landmark path, kLongGap of
// vba_device.h).  It is marked by a NEGATIVE step count (the convention of vba_upload.hip): k_sdyn_edges and k_sdyn_cost leave a
// marked edge alone, the kernels of vba_schur_dyn_long.hip write its r, A = D Phi and ecost at the edge's own index and its cost into
// a partial slot of its own behind the block partials.  Its chain (vba_long_body.h) lives in a slot of long_pool_states(long_plan(s))
// states of six doubles, one pool per call parity.
#pragma once

#include <cstddef>

#include "vba_math.h"

namespace vba {

constexpr int kSchurDynLongGap = 64;

struct SchurDynLongPlan {
    int nlong = 0;              // long edges of the window (n - 1 at most: no cap)
    int pool_states = 0;        // states of six doubles that their slots take, per parity
    int npart = 0;              // cost partials of the handle: the block partials, then one per long edge in index order
    size_t pool_bytes = 0;      // both parities
};

// steps [n - 1]: the step count of every edge, each >= 1 (checked by the caller).  With `parallel` the long edges are marked in place
// (negated), their poses go to idx [n - 1] in index order and the offsets of their slots (in states) to off [n - 1]; without it
// nothing is marked and the plan is that of a window without long edges (VBA_SCHUR_LONG_SERIAL: every edge on the serial lanes).
inline SchurDynLongPlan schur_dyn_long_plan(int n, int* steps, bool parallel, int* idx, int* off) {
    SchurDynLongPlan p;
    for (int i = 0; parallel && i + 1 < n; ++i) {
        if (steps[i] <= kSchurDynLongGap) continue;
        idx[p.nlong] = i;
        off[p.nlong] = p.pool_states;
        p.pool_states += long_pool_states(long_plan(steps[i]));
        steps[i] = -steps[i];
        ++p.nlong;
    }
    p.npart = (n - 1 + 255) / 256 + p.nlong;
    p.pool_bytes = (size_t)2 * p.pool_states * 6 * sizeof(double);
    return p;
}

}  // namespace vba

#ifdef __HIPCC__
#include "vba_schur_dyn.h"

namespace vba {

// r, A, ecost of the long edges at `states` [n][10] behind schur_dyn_edges_launch (which skips them): the chain of the view's
// parity where the pool does not hold it already, the tangent pass spread over kLongSplit workgroups per edge, the product
void schur_dyn_long_edges_launch(const SchurDynView& W, const double* states, hipStream_t s);
// part[npart + k] = sigma |r|^2 of long edge k at `states`; its chain stays in the pool of parity `slot_par`
void schur_dyn_long_cost_launch(const SchurDynView& W, const double* states, int slot_par, hipStream_t s);

}  // namespace vba
#endif
