// vba_schur_dyn.hip -- the orbit-dynamics factor of the free-landmark mode (vba_schur_enable_dynamics; ADD-ON, PARITY UNPINNED as
// the rest of the mode: vba_schur.hip carries the map of the units): its kernels, then the entry point.  Model, unknown order and the scatter's work items: vba_schur_dyn_math.h.  The attitude factor of the
// fixed-landmark path stays out (its Newton blocks are not symmetric; this mode's solver is a Cholesky); vba_schur_att.hip adds a
// Gauss-Newton statement of it, opt-in, on a handle that has this factor.
//
// Kernels (no float atomics; every sum in a fixed order, so two runs and two handles leave the same bits):
//   k_sdyn_edges    eight lanes per edge, six of them at work: lane c propagates the edge's start state with the tangent e_c
//                   (rk4_step<true>, the closed-form acceleration derivative of vba_math.h) and writes column c of D Phi; lane 0 also
//                   writes r and sigma |r|^2.  One tangent per lane as dynamics_block (vba_dyn_body.h) and not six tangents in one
//                   thread: the six-tangent step keeps 6 x 18 doubles of tangent state live on top of the trajectory, which is the
//                   register budget k_dynamics_pair already strains; the edges are few (n - 1) and the kernel is a latency chain of
//                   at most 64 steps either way.
//   k_sdyn_scatter  block per pose, thread per target entry (kSchurDynItems of them): edge i - 1's share, then edge i's
//   k_sdyn_update   thread per pose: v_new = v + dv
//   k_sdyn_cost     thread per edge: residual-only propagation at the given states, block partials
#include <hip/hip_runtime.h>

#include "vba_schur_context.h"
#include "vba_schur_dyn.h"
#include "vba_schur_dyn_long.h"
#include "vba_schur_dyn_math.h"

namespace vba {

namespace {

constexpr int kLanes = 8;           // lanes per edge (six columns; a power of two keeps an edge inside one wavefront)

__global__ __launch_bounds__(256) void k_sdyn_edges(SchurDynView W, const double* states) {
    const int gid = blockIdx.x * 256 + threadIdx.x;
    const int e = gid / kLanes, c = gid % kLanes;
    if (e >= W.n - 1 || c >= 6) return;
    if (W.steps[e] < 0) return;         // a long edge: vba_schur_dyn_long.hip writes its r, A, ecost
    const double* st = states + (size_t)e * 10;
    double xhat[6], col[6];
    schur_dyn_edge_column(st, W.steps[e], c, xhat, col);
    double* A = W.A + (size_t)e * 36;
#pragma unroll
    for (int r = 0; r < 6; ++r) A[6 * r + c] = col[r];
    if (c == 0) {
        double r6[6];
        const double s = schur_dyn_residual(xhat, st + 10, r6);
#pragma unroll
        for (int r = 0; r < 6; ++r) W.r[(size_t)e * 6 + r] = r6[r];
        W.ecost[e] = W.sigma * s;
    }
}

__global__ __launch_bounds__(128) void k_sdyn_scatter(SchurDynView W) {
    const int i = blockIdx.x, t = threadIdx.x;
    if (i >= W.n || t >= kSchurDynItems) return;
    schur_dyn_scatter_item(W.n, W.Npad, i, t, W.sigma, W.lamda, W.A, W.r, W.S, W.g);
}

__global__ __launch_bounds__(256) void k_sdyn_update(SchurDynView W, const double* states, double* states_new) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= W.n) return;
    const double* dv = W.g + (size_t)6 * W.n + 3 * i;
#pragma unroll
    for (int a = 0; a < 3; ++a) states_new[(size_t)i * 10 + 7 + a] = states[(size_t)i * 10 + 7 + a] + dv[a];
}

__global__ __launch_bounds__(256) void k_sdyn_cost(SchurDynView W, const double* states) {
    __shared__ double red[4];
    const int e = blockIdx.x * 256 + threadIdx.x;
    double s = 0.0;
    if (e < W.n - 1 && W.steps[e] > 0) {        // (a long edge has a partial slot of its own: vba_schur_dyn_long.hip)
        const double* st = states + (size_t)e * 10;
        double xhat[6], r6[6];
        schur_dyn_predict(st, W.steps[e], xhat);
        s = W.sigma * schur_dyn_residual(xhat, st + 10, r6);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) W.part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

}  // namespace

void schur_dyn_edges_launch(const SchurDynView& W, const double* states, hipStream_t s) {
    hipLaunchKernelGGL(k_sdyn_edges, dim3(((W.n - 1) * kLanes + 255) / 256), dim3(256), 0, s, W, states);
}

void schur_dyn_scatter_launch(const SchurDynView& W, hipStream_t s) {
    hipLaunchKernelGGL(k_sdyn_scatter, dim3(W.n), dim3(128), 0, s, W);
}

void schur_dyn_update_launch(const SchurDynView& W, const double* states, double* states_new, hipStream_t s) {
    hipLaunchKernelGGL(k_sdyn_update, dim3((W.n + 255) / 256), dim3(256), 0, s, W, states, states_new);
}

void schur_dyn_cost_launch(const SchurDynView& W, const double* states, hipStream_t s) {
    hipLaunchKernelGGL(k_sdyn_cost, dim3(W.npart), dim3(256), 0, s, W, states);
}

}  // namespace vba

SchurDynView schur_dyn_view(vba_schur_handle h, const SchurView& V) {
    const SchurDyn& D = h->dyn;
    SchurDynView W{};
    W.n = V.n; W.Npad = V.Npad; W.sigma = D.sigma; W.lamda = V.lamda;
    W.steps = D.steps; W.r = D.r; W.A = D.A; W.ecost = D.ecost; W.part = D.part; W.npart = D.npart;
    W.nlong = D.nlong; W.par = D.par; W.long_idx = D.long_idx; W.long_off = D.long_off; W.long_pool = D.long_pool;
    W.long_pool_states = D.long_pool_states;
    W.S = V.S; W.g = V.g;
    return W;
}

// The body of both entries.  long_gaps: gaps of kSchurDynMaxGap + 1 .. VBA_MAX_GAP steps are accepted (vba_schur_enable_dynamics_long)
// and, unless VBA_SCHUR_LONG_SERIAL=1 is set, propagated parallel in time by the kernels of vba_schur_dyn_long.hip.
int schur_dyn_enable(vba_schur_handle h, const int* time_idx, double sigma_dyn, bool long_gaps) {
    if (!h || !time_idx) return sfail(VBA_EINVAL, "null argument");
    if (!h->uploaded) return sfail(VBA_ESTATE, "upload the problem first");
    if (h->dyn.enabled) return sfail(VBA_ESTATE, "the dynamics factor is already enabled on this handle");
    if (!(sigma_dyn > 0.0) || !std::isfinite(sigma_dyn)) return sfail(VBA_EINVAL, "sigma_dyn must be positive and finite");
    SchurView& V = h->V;
    const int n = V.n;
    if (n < 2) return sfail(VBA_EINVAL, "the dynamics factor needs at least two poses");
    std::vector<int> steps(n - 1);
    for (int i = 0; i + 1 < n; ++i) {
        const int64_t d = (int64_t)time_idx[i + 1] - (int64_t)time_idx[i];
        if (d < 1) return sfail(VBA_EINVAL, "time_idx must increase: poses " + std::to_string(i) + " and " + std::to_string(i + 1));
        if (long_gaps && d > VBA_MAX_GAP)
            return sfail(VBA_EINVAL, "a gap of " + std::to_string(d) + " steps between poses " + std::to_string(i) + " and " + std::to_string(i + 1) +
                                         ": longer than VBA_MAX_GAP (2^20 steps)");
        if (!long_gaps && d > kSchurDynMaxGap)
            return sfail(VBA_EINVAL, "a gap of " + std::to_string(d) + " steps between poses " + std::to_string(i) + " and " + std::to_string(i + 1) +
                                         ": the dynamics factor of this mode covers gaps of 1 .. " + std::to_string(kSchurDynMaxGap) + " steps");
        steps[i] = (int)d;
    }
    SCHK(hipSetDevice(h->device));
    SCHK(hipStreamSynchronize(h->stream));
    const int N = 9 * n;
    int nb, Npad;
    schur_padded_size(N, nb, Npad);
    SchurDyn& D = h->dyn;
    const int npart = schur_dyn_partials(n);
    // long edges: marked in steps, a chain slot each in a pool per parity, a cost partial each behind the block partials
    bool serial = false;
    if (const char* e = std::getenv("VBA_SCHUR_LONG_SERIAL")) serial = std::atoi(e) != 0;
    std::vector<int> long_idx(n - 1), long_off(n - 1);
    const SchurDynLongPlan lp = schur_dyn_long_plan(n, steps.data(), long_gaps && !serial, long_idx.data(), long_off.data());
    SchurLayout lay;
    const size_t o_S = lay.need((size_t)Npad * Npad * 8), o_g = lay.need((size_t)Npad * 8), o_y = lay.need((size_t)Npad * 8),
                 o_iL = lay.need((size_t)nb * kT * kT * 8);
    const size_t o_st = lay.need((size_t)(n - 1) * 4), o_r = lay.need((size_t)(n - 1) * 48), o_A = lay.need((size_t)(n - 1) * 288),
                 o_ec = lay.need((size_t)(n - 1) * 8), o_part = lay.need((size_t)lp.npart * 8);
    const size_t o_li = lay.need((size_t)lp.nlong * 4), o_lo = lay.need((size_t)lp.nlong * 4), o_pool = lay.need(lp.pool_bytes);
    const size_t bytes = lay.bytes;
    char* A = nullptr;
    if (hipMalloc(&A, bytes) != hipSuccess) { (void)hipGetLastError(); return sfail(VBA_ENOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes for the dynamics factor failed"); }
    if (hipMemset(A, 0, bytes) != hipSuccess || hipMemcpy(A + o_st, steps.data(), (size_t)(n - 1) * 4, hipMemcpyHostToDevice) != hipSuccess ||
        (lp.nlong > 0 && (hipMemcpy(A + o_li, long_idx.data(), (size_t)lp.nlong * 4, hipMemcpyHostToDevice) != hipSuccess ||
                          hipMemcpy(A + o_lo, long_off.data(), (size_t)lp.nlong * 4, hipMemcpyHostToDevice) != hipSuccess)) ||
        hipStreamSynchronize(nullptr) != hipSuccess) {
        hipFree(A);
        return sfail(VBA_EHIP, "dynamics factor: hipMemset / upload failed");
    }
    // the scratch of the queries was sized for 6 n, so it goes: the three queries refuse this handle from now on, and
    // vba_schur_covariance_dyn allocates it anew for 9 n
    schur_scratch_release(h->rel.sc);
    h->rel = SchurRel{};
    schur_scratch_release(h->q.sc);
    h->q = SchurQuery{};
    D.arena = A; D.sigma = sigma_dyn; D.npart = npart;
    D.steps = (int*)(A + o_st); D.r = (double*)(A + o_r); D.A = (double*)(A + o_A); D.ecost = (double*)(A + o_ec); D.part = (double*)(A + o_part);
    D.nlong = lp.nlong; D.par = 0; D.long_pool_states = lp.pool_states;
    D.long_idx = (int*)(A + o_li); D.long_off = (int*)(A + o_lo); D.long_pool = (double*)(A + o_pool);
    D.h_long_idx.assign(long_idx.begin(), long_idx.begin() + lp.nlong);
    D.h_part.assign(lp.npart, 0.0);
    // (the 6 n arrays of vba_schur_create stay in the handle's arena, unused: one allocation, freed with the handle)
    V.N = N; V.nb = nb; V.Npad = Npad;
    V.S = (double*)(A + o_S); V.g = (double*)(A + o_g); V.ybuf = (double*)(A + o_y); V.invL = (double*)(A + o_iL);
    h->bw = nb - 1;             // velocity rows reach every pose column: the substitutions cover every tile of the factor
    D.enabled = true;
    return VBA_OK;
}

extern "C" int vba_schur_enable_dynamics(vba_schur_handle h, const int* time_idx, double sigma_dyn) {
    return schur_dyn_enable(h, time_idx, sigma_dyn, false);
}
