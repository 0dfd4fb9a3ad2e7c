// vba_long.hip -- long gaps of the pose chain (A4 over hundreds of seconds), propagated PARALLEL IN TIME.
//
// The reference walks a gap of s seconds as s dependent RK4 steps of 1 s (propagate_orbit_dynamics, BA_utils.py:73-87) and
// differentiates that chain (predict, :457-509).  A window of a later pass of a sequence holds gaps of up to 1000 s
// (read_detections inserts a knot every 1000 s, od_pipe.py:213-221): on one lane that is a chain of ~10^5 dependent
// instructions per edge, per LM trial and once more (six times, with a tangent each) for the factor -- 1.28 ms per BA call
// at a 945 s gap in round 4, thirty times the 500-pose headline window.  Only the 6-vector state is a recurrence, and even
// that recurrence parallelises: the gap is cut into P ~ sqrt(s) chunks of L ~ sqrt(s) steps and the chunk-start states U_j are
// found by the parareal iteration (Lions, Maday, Turinici 2001) whose FINE propagator is the reference's own chain of 1 s
// steps and whose coarse propagator G is ONE RK4 step over the chunk:
//     U_0 = x0,  U_{j+1} <- F_j(U_j) + (G_j(U_j') - G_j(U_j))        (U' = the new iterate, swept left to right)
// The fixed point is U_{j+1} = F_j(U_j), the serial chain itself (after k iterations the first k chunks are the serial chain
// bit for bit).  The coarse step over ~27 s is wrong by ~1e-10 relative, so an iteration contracts the error by ~1e-8: the
// first one leaves ~1e-15 relative, and the fine pass of the second finds every chunk landing on the next chunk's start state
// to 2^-48 relative -- the chain's defect -- and stops there (one sweep and two fine passes up to ~1000 s, two or three
// sweeps at 3000 - 6000 s; prototype with convergence table: tools/parareal_prototype.py).  What comes out differs from the serial
// walk by rounding (<= 1e-15 relative measured, the size of the difference between this library's rsq-based acceleration and
// the reference's sqrt / division), is a function of the states and the step count only, and is the same in every kernel set
// -- both kernels below call the same long_states().
// Cost of a 935 s edge: 35 coarse steps + 2 * 27 fine steps + a 35-step matrix-vector recurrence instead of 935 fine steps.
//
// The transition matrix of a long edge is the ORDERED PRODUCT of the transition matrices of G <= 128 sub-chunks of ~10 steps (each
// from its start state on the converged chain, six tangent lanes per sub-chunk as in dynamics_block), multiplied pairwise in a
// fixed tree.  The start states are a by-product of the last fine pass -- and of the TRIAL kernel's: an accepted trial is evaluated
// at exactly the states the next call starts from, so its chain is carried (DevView::long_pool, the carried-keys argument applied
// to dynamics) and the next call's factor is the tangent pass and the product alone.
//
// Edges of at most kLongGap steps never come here: their arithmetic (and the bits of every window without a long gap) is
// what it was.  With the hop integrator (predict_gpu's <= 100 s steps) no edge is long.
#include "vba_device.h"
#include "vba_launch.h"
#include "vba_long_body.h"

namespace vba {

// where the chain of long edge k of window w lives for the call of parity `par` (every long edge has a slot: an edge the window's
// pool has no room for is not marked long, vba_upload_window)
__device__ __forceinline__ double* long_slot(const DevView& V, int w, int par, int k) {
    const int off = V.long_off[(size_t)w * kLongCap + k];
    return V.long_pool + (((size_t)w * 2 + par) * V.long_pool_cap + off) * 6;
}

// The orbit residual of the long edges at the TRIAL states (BA_filtering.py:63-67): sqrt(Sigma) sum |[x_hat - p', 100 (v_hat - v')]|
// of edge long_idx[k] into slot nblk_obs + nblk_dyn + k of part_trial (k_trial's pose-chain lanes left that edge's orbit part out
// and kept its attitude part).  One wavefront per long edge; gated as k_trial is.  The chain it walked is left for the next call
// (slot of the parity that reads it): x_hat, then the sub-chunk start states.
__global__ __launch_bounds__(64) void k_long_trial(DevView V) {
    const int w = blockIdx.y;
    VBA_SKIP_CALL(V, w);
    if (V.sc[w].done) return;
    const int k = blockIdx.x, lane = threadIdx.x;
    double* slot = V.part_trial + (size_t)w * V.trial_stride + V.nblk_obs + V.nblk_dyn + k;
    if (k >= V.n_long[w]) {
        if (lane == 0) *slot = 0.0;
        return;
    }
    const int i = V.long_idx[(size_t)w * kLongCap + k];
    const size_t sb = (size_t)w * V.n_max;
    const double* st = V.states_new + (sb + i) * 10;
    const double* sn = st + 10;
    const double x0[6] = {st[0], st[1], st[2], st[7], st[8], st[9]};
    const int s = -V.steps[sb + i];
    double* carry = long_slot(V, w, V.par ^ 1, k);
    double U[6], x[6];
    long_states(x0, s, long_plan(s), lane, U, x, carry + kLongHead * 6);
    if (lane == 0) {
        // header: x_hat, then the start state this chain belongs to (what the reader checks)
#pragma unroll
        for (int c = 0; c < 6; ++c) { carry[c] = x[c]; carry[6 + c] = x0[c]; }
        const double r = fabs(x[0] - sn[0]) + fabs(x[1] - sn[1]) + fabs(x[2] - sn[2]) +
                         fabs((x[3] - sn[7]) * kVelCoeff) + fabs((x[4] - sn[8]) * kVelCoeff) + fabs((x[5] - sn[9]) * kVelCoeff);
        *slot = r * V.prm.sqrt_sigma;
    }
}

// The chain of the long edges at the INPUT states of a call, where the pool does not hold it already.  The slot of the call's
// parity was written by the previous call's trial kernel; IF that chain started from the very bits of this call's state (the header
// says which state it belongs to; a chain is a function of that state and the step count alone, and an upload of the window clears
// the pool) there is nothing to do -- otherwise (fresh states from the host, a landmark-only call in front) one wavefront finds it.
__global__ __launch_bounds__(64) void k_long_chain(DevView V) {
    const int w = blockIdx.y;
    VBA_SKIP_CALL(V, w);
    const int k = blockIdx.x, lane = threadIdx.x;
    if (k >= V.n_long[w]) return;
    const int i = V.long_idx[(size_t)w * kLongCap + k];
    const size_t pb = (size_t)w * V.n_max + i;
    const double* st = V.states + pb * 10;
    const double x0[6] = {st[0], st[1], st[2], st[7], st[8], st[9]};
    double* chain = long_slot(V, w, V.par, k);
    bool same = true;
#pragma unroll
    for (int c = 0; c < 6; ++c) same = same && f64_bits(chain[6 + c]) == f64_bits(x0[c]);
    if (same) return;       // (every lane takes the same decision from the same six words)
    const int s = -V.steps[pb];
    double U[6], x[6];
    long_states(x0, s, long_plan(s), lane, U, x, chain + kLongHead * 6);
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 6; ++c) { chain[c] = x[c]; chain[6 + c] = x0[c]; }
    }
}

// The transition matrices of the sub-chunks of the long edges and their ordered product, first part.  kLongSplit workgroups of 128
// per long edge (on as many compute units: sixteen waves of fp64 arithmetic on ONE compute unit took 38 us for what is 6 us of
// instructions per wave), behind k_long_chain: a workgroup takes 16 consecutive sub-chunks -- 8 lanes each, 6 tangents as in
// dynamics_block, ~10 steps from the sub-chunk's start state in the pool -- and multiplies their matrices in order, pairwise, in
// place (both bodies: vba_long_body.h): its partial product M_{g0 + 15} ... M_{g0} goes behind the chain in the edge's slot.
__global__ __launch_bounds__(128) void k_long_tangent(DevView V) {
    __shared__ double M[kLongSubs][36];
    const int w = blockIdx.y;
    VBA_SKIP_CALL(V, w);
    const int k = blockIdx.x / kLongSplit, part = blockIdx.x % kLongSplit, tid = threadIdx.x;
    if (k >= V.n_long[w]) return;
    const int i = V.long_idx[(size_t)w * kLongCap + k];
    const size_t pb = (size_t)w * V.n_max + i;
    const int s = -V.steps[pb];
    const LongPlan pl = long_plan(s);
    const int g0 = part * 16;
    if (g0 >= pl.G) return;
    const int cnt = pl.G - g0 < 16 ? pl.G - g0 : 16;
    double* chain = long_slot(V, w, V.par, k);
    long_tangent_subchunks(chain, s, pl, g0, tid, M);
    __syncthreads();
    long_ordered_product<128>(M, cnt, tid);     // its partial product, in place
    if (tid < 36) chain[(size_t)(kLongHead + pl.G) * 6 + (size_t)part * 36 + tid] = M[0][tid];
}

// ... second part: the partial products of an edge multiplied in order -- Phi = M_{G-1} ... M_1 M_0 --, and with x_hat from the
// chain's header the prediction, the residual r_orbit of pose long_idx[k] and sum |r_orbit| into slot nblk_pred + k of part_pred
// (parity of the call).  One wavefront per long edge.
__global__ __launch_bounds__(64) void k_long_finish(DevView V) {
    __shared__ double M[kLongSplit][36];
    const int w = blockIdx.y;
    VBA_SKIP_CALL(V, w);
    const int k = blockIdx.x, tid = threadIdx.x;
    double* slot = V.part_pred + ((size_t)w * 2 + V.par) * V.pred_stride + V.nblk_pred + k;
    if (k >= V.n_long[w]) {
        if (tid == 0) *slot = 0.0;
        return;
    }
    const int i = V.long_idx[(size_t)w * kLongCap + k];
    const size_t pb = (size_t)w * V.n_max + i;
    const double* st = V.states + pb * 10;
    const int s = -V.steps[pb];
    const LongPlan pl = long_plan(s);
    const double* chain = long_slot(V, w, V.par, k);
    const int cnt = (pl.G + 15) / 16;
    for (int e = tid; e < cnt * 36; e += 64) (&M[0][0])[e] = chain[(size_t)(kLongHead + pl.G) * 6 + e];
    if (tid == 0) {
        const double* x = chain;
        const double* sn = st + 10;
        double* xh = V.xhat + pb * 6;
        double* ro = V.rorb + pb * 6;
#pragma unroll
        for (int r = 0; r < 6; ++r) xh[r] = x[r];
        ro[0] = x[0] - sn[0];
        ro[1] = x[1] - sn[1];
        ro[2] = x[2] - sn[2];
        ro[3] = (x[3] - sn[7]) * kVelCoeff;
        ro[4] = (x[4] - sn[8]) * kVelCoeff;
        ro[5] = (x[5] - sn[9]) * kVelCoeff;
        *slot = fabs(ro[0]) + fabs(ro[1]) + fabs(ro[2]) + fabs(ro[3]) + fabs(ro[4]) + fabs(ro[5]);
    }
    __syncthreads();
    long_ordered_product<64>(M, cnt, tid);
    if (tid < 36) V.Phi[pb * 36 + tid] = M[0][tid];
}

void launch_long_factor(const DevView& V, hipStream_t s) {
    if (V.nblk_long <= 0 || V.hop) return;
    hipLaunchKernelGGL(k_long_chain, dim3(V.nblk_long, V.W), dim3(64), 0, s, V);
    hipLaunchKernelGGL(k_long_tangent, dim3(V.nblk_long * kLongSplit, V.W), dim3(128), 0, s, V);
    hipLaunchKernelGGL(k_long_finish, dim3(V.nblk_long, V.W), dim3(64), 0, s, V);
}

void launch_long_trial(const DevView& V, hipStream_t s) {
    if (V.nblk_long <= 0 || V.hop || V.prm.initialize) return;
    hipLaunchKernelGGL(k_long_trial, dim3(V.nblk_long, V.W), dim3(64), 0, s, V);
}

}  // namespace vba
