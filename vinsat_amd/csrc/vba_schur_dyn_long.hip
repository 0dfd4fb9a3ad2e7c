// vba_schur_dyn_long.hip -- long gaps of the orbit-dynamics factor of the free-landmark mode (vba_schur_enable_dynamics_long; ADD-ON,
// PARITY UNPINNED as the rest of the mode: vba_schur.hip carries the map of the units).  A window of a later pass of a sequence holds
// gaps of hundreds of seconds (a knot every 1000 s); k_sdyn_edges walks an edge as one dependent RK4 chain per lane, ~10^5
// instructions at 935 s, in the build and again in every trial's cost.  Here an edge of more than kSchurDynLongGap steps is propagated
// PARALLEL IN TIME, exactly as the fixed-landmark path does it (vba_long.hip has the account of the method; the bodies are shared:
// vba_long_body.h): the parareal chain of one wavefront, the transition matrix as the ordered product of <= 128 sub-chunk matrices.
// Everything downstream (k_sdyn_scatter, the attitude factor, every _dyn / _att query) reads r, A = D Phi and ecost per edge and
// nothing else, so this unit writes those three at the edge's own index and the rest of the mode is as it was.
//
// The host's plan -- which edges are long, their slots, the partial count, the pool -- is schur_dyn_long_plan (vba_schur_dyn_long.h).
// A slot (vba_long_body.h): [0] x_hat, [1] the start state the chain belongs to, [2] the step count it belongs to (a pool is zeroed
// when the factor is enabled: an empty slot matches no edge), [3, 3 + G) the sub-chunk start states, then kLongSplit partial products.
// The chain is CONTENT-ADDRESSED: a function of the start state's bits and the step count alone, so a kernel that finds both in the
// header of the slot it would write has nothing to walk.  The cost of a trial leaves its chain in the pool of the other parity; an
// accepted trial flips the parity, and the next call's cost at the resident states and its build find the chain there: one walk
// per vba_schur_iterate, none in the build.  A rejected trial, vba_schur_set_state or a query at another state miss and walk.
//
// Kernels (no float atomics, every sum and product in a fixed order: two runs and two handles leave the same bits):
//   k_sdyn_long_chain    wave per long edge: long_states from (p_i, v_i) into the slot of the view's parity, unless it is there
//   k_sdyn_long_tangent  kLongSplit workgroups of 128 per long edge (on as many compute units): 8 lanes per sub-chunk, six tangents
//                        through rk4_step<true>, the partial ordered products in LDS
//   k_sdyn_long_finish   wave per long edge: Phi = the product of the partials; A[e] = D Phi, r[e], ecost[e] (vector stores)
//   k_sdyn_long_cost     wave per long edge: the chain at the states given (or its header), sigma |r|^2 into partial slot npart + k
#include <hip/hip_runtime.h>

#include "vba_schur_context.h"
#include "vba_schur_dyn_long.h"
#include "vba_schur_dyn_math.h"
#include "vba_long_body.h"

namespace vba {

static_assert(kSchurDynLongGap == kLongGap, "both modes call the same edges long");

namespace {

__device__ __forceinline__ double* sdyn_long_slot(const SchurDynView& W, int par, int k) {
    return W.long_pool + ((size_t)par * W.long_pool_states + W.long_off[k]) * 6;
}

// the chain in `slot` is that of start state x0 over s steps (every lane takes the same decision from the same seven words)
__device__ __forceinline__ bool sdyn_long_holds(const double* slot, const double* x0, int s) {
    bool same = slot[12] == (double)s;
#pragma unroll
    for (int c = 0; c < 6; ++c) same = same && f64_bits(slot[6 + c]) == f64_bits(x0[c]);
    return same;
}

// the chain of edge i over s steps at `states` into `slot`, header last (lane 0); a slot that holds it already is left as it is
__device__ __forceinline__ void sdyn_long_walk(double* slot, const double* states, int i, int s, int lane) {
    const double* st = states + (size_t)i * 10;
    const double x0[6] = {st[0], st[1], st[2], st[7], st[8], st[9]};
    if (sdyn_long_holds(slot, x0, s)) return;
    double U[6], x[6];
    long_states(x0, s, long_plan(s), lane, U, x, slot + kLongHead * 6);
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 6; ++c) { slot[c] = x[c]; slot[6 + c] = x0[c]; }
        slot[12] = (double)s;
    }
}

__global__ __launch_bounds__(64) void k_sdyn_long_chain(SchurDynView W, const double* states) {
    const int k = blockIdx.x, lane = threadIdx.x;
    if (k >= W.nlong) return;
    const int i = W.long_idx[k];
    sdyn_long_walk(sdyn_long_slot(W, W.par, k), states, i, -W.steps[i], lane);
}

__global__ __launch_bounds__(128) void k_sdyn_long_tangent(SchurDynView W) {
    __shared__ double M[kLongSubs][36];
    const int k = blockIdx.x / kLongSplit, part = blockIdx.x % kLongSplit, tid = threadIdx.x;
    if (k >= W.nlong) return;
    const int s = -W.steps[W.long_idx[k]];
    const LongPlan pl = long_plan(s);
    const int g0 = part * kLongSubs;
    if (g0 >= pl.G) return;             // (block uniform)
    const int cnt = pl.G - g0 < kLongSubs ? pl.G - g0 : kLongSubs;
    double* chain = sdyn_long_slot(W, W.par, k);
    long_tangent_subchunks(chain, s, pl, g0, tid, M);
    __syncthreads();
    long_ordered_product<128>(M, cnt, tid);
    if (tid < 36) chain[(size_t)(kLongHead + pl.G) * 6 + (size_t)part * 36 + tid] = M[0][tid];
}

__global__ __launch_bounds__(64) void k_sdyn_long_finish(SchurDynView W, const double* states) {
    __shared__ double M[kLongSplit][36];
    const int k = blockIdx.x, tid = threadIdx.x;
    if (k >= W.nlong) return;
    const int e = W.long_idx[k];
    const LongPlan pl = long_plan(-W.steps[e]);
    const double* chain = sdyn_long_slot(W, W.par, k);
    const int cnt = (pl.G + kLongSubs - 1) / kLongSubs;     // <= kLongSplit: G <= 128
    for (int q = tid; q < cnt * 36; q += 64) (&M[0][0])[q] = chain[(size_t)(kLongHead + pl.G) * 6 + q];
    if (tid == 0) {
        double r6[6];
        const double s2 = schur_dyn_residual(chain, states + (size_t)(e + 1) * 10, r6);
#pragma unroll
        for (int r = 0; r < 6; ++r) W.r[(size_t)e * 6 + r] = r6[r];
        W.ecost[e] = W.sigma * s2;
    }
    __syncthreads();
    long_ordered_product<64>(M, cnt, tid);
    if (tid < 36) W.A[(size_t)e * 36 + tid] = tid < 18 ? M[0][tid] : M[0][tid] * kVelCoeff;      // rows 3 .. 5 of D Phi, as schur_dyn_edge_column scales them
}

__global__ __launch_bounds__(64) void k_sdyn_long_cost(SchurDynView W, const double* states, int slot_par) {
    const int k = blockIdx.x, lane = threadIdx.x;
    if (k >= W.nlong) return;
    const int i = W.long_idx[k];
    double* slot = sdyn_long_slot(W, slot_par, k);
    sdyn_long_walk(slot, states, i, -W.steps[i], lane);
    if (lane == 0) {        // (the header is this lane's own store, or older than the kernel)
        double r6[6];
        W.part[W.npart + k] = W.sigma * schur_dyn_residual(slot, states + (size_t)(i + 1) * 10, r6);
    }
}

}  // namespace

void schur_dyn_long_edges_launch(const SchurDynView& W, const double* states, hipStream_t s) {
    hipLaunchKernelGGL(k_sdyn_long_chain, dim3(W.nlong), dim3(64), 0, s, W, states);
    hipLaunchKernelGGL(k_sdyn_long_tangent, dim3(W.nlong * kLongSplit), dim3(128), 0, s, W);
    hipLaunchKernelGGL(k_sdyn_long_finish, dim3(W.nlong), dim3(64), 0, s, W, states);
}

void schur_dyn_long_cost_launch(const SchurDynView& W, const double* states, int slot_par, hipStream_t s) {
    hipLaunchKernelGGL(k_sdyn_long_cost, dim3(W.nlong), dim3(64), 0, s, W, states, slot_par);
}

}  // namespace vba

extern "C" {

int vba_schur_enable_dynamics_long(vba_schur_handle h, const int* time_idx, double sigma_dyn) {
    return schur_dyn_enable(h, time_idx, sigma_dyn, true);
}

int vba_schur_long_edges(vba_schur_handle h, int* idx, int cap, int* count) {
    if (!h || !count) return sfail(VBA_EINVAL, "null argument");
    if (!h->dyn.enabled) return sfail(VBA_ESTATE, "the dynamics factor is not enabled on this handle");
    const std::vector<int>& L = h->dyn.h_long_idx;
    *count = (int)L.size();
    if (idx) {
        if (cap < (int)L.size()) return sfail(VBA_EINVAL, "buffer too small");
        std::copy(L.begin(), L.end(), idx);
    }
    return VBA_OK;
}

}  // extern "C"
