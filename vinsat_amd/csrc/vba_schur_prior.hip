// vba_schur_prior.hip -- the state prior factor of the free-landmark mode (vba_schur_enable_state_prior) and the window hand-off that
// feeds it (vba_schur_handoff); ADD-ON, PARITY UNPINNED as the rest of the mode: vba_schur.hip carries the map of the units.  Model,
// the scatter's work items and the 9x9 algebra of the hand-off: vba_schur_prior_math.h.
//
// Kernels (no float atomics; every sum in a fixed order, so two runs and two handles leave the same bits):
//   k_sprior_terms    thread per prior: e, J, Lambda F, Lambda e, e^T Lambda e
//   k_sprior_scatter  block per prior, thread per target entry (kSchurPriorItems of them); behind k_satt_scatter (or k_sdyn_scatter)
//                     on the same stream
//   k_sprior_cost     thread per prior: e^T Lambda e at the given states, block partials
//   k_shandoff        one workgroup of 128 behind the device part of vba_schur_covariance_dyn: (p, v) of pose n - 1 over the gap with
//                     Phi -- the lanes of k_sdyn_edges (schur_dyn_phi_column) at 64 steps or fewer, the chain, the sub-chunk tangent
//                     passes and the ordered products of vba_long_body.h beyond, as k_sdyn_long_* use them -- then G Sigma G^T + noise,
//                     its inverse by a 9x9 Cholesky and the anchor, by thread 0 in LDS
#include <hip/hip_runtime.h>

#include "vba_schur_context.h"
#include "vba_schur_dyn_long.h"
#include "vba_schur_dyn_math.h"
#include "vba_schur_prior_math.h"
#include "vba_long_body.h"

namespace vba {

namespace {

__global__ __launch_bounds__(256) void k_sprior_terms(SchurPriorView W, const double* states) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= W.count) return;
    W.share[k] = schur_prior_terms(states + (size_t)W.idx[k] * 10, W.anchor + (size_t)k * 10, W.info + (size_t)k * 81, W.e + (size_t)k * 9,
                                   W.J + (size_t)k * 9, W.LF + (size_t)k * 81, W.Le + (size_t)k * 9);
}

__global__ __launch_bounds__(64) void k_sprior_scatter(SchurPriorView W) {
    const int k = blockIdx.x, t = threadIdx.x;
    if (k >= W.count || t >= kSchurPriorItems) return;
    schur_prior_scatter_item(W.n, W.Npad, W.idx[k], t, W.J + (size_t)k * 9, W.LF + (size_t)k * 81, W.Le + (size_t)k * 9, W.S, W.g);
}

__global__ __launch_bounds__(256) void k_sprior_cost(SchurPriorView W, const double* states) {
    __shared__ double red[4];
    const int k = blockIdx.x * 256 + threadIdx.x;
    double s = 0.0;
    if (k < W.count) {
        double w[4], e[9], Le[9];
        schur_prior_residual(states + (size_t)W.idx[k] * 10, W.anchor + (size_t)k * 10, w, e);
        s = schur_prior_cost(W.info + (size_t)k * 81, e, Le);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) W.part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

struct HandoffArgs {
    int steps;
    double c[4];                    // cumrot_gap
    double noise[3];                // per second: position, attitude, velocity
    const double* st;               // the state of pose n - 1 [10]
    const double* Sigma;            // its 9x9 marginal
    double* pool;                   // a chain slot of long_pool_states(long_plan(VBA_MAX_GAP)) states at least (long gaps only)
    double* out;                    // [10] anchor, [81] info, [1] 0 or -1 (Sigma' not positive definite)
};

__global__ __launch_bounds__(128) void k_shandoff(HandoffArgs A) {
    __shared__ double M[kLongSubs][36];
    __shared__ double Pm[kLongSplit][36];
    __shared__ double Phi[36], xh[6];
    __shared__ double R[9], G[81], T[81], Sp[81], Lw[81], Ww[81];
    const int tid = threadIdx.x;
    const double* st = A.st;
    if (A.steps <= kSchurDynMaxGap) {
        if (tid < 6) {
            double xhat[6], col[6];
            schur_dyn_phi_column(st, A.steps, tid, xhat, col);
#pragma unroll
            for (int r = 0; r < 6; ++r) Phi[6 * r + tid] = col[r];
            if (tid == 0)
#pragma unroll
                for (int r = 0; r < 6; ++r) xh[r] = xhat[r];
        }
        __syncthreads();
    } else {
        const LongPlan pl = long_plan(A.steps);
        double* chain = A.pool;
        if (tid < 64) {             // (wave 0, whole: the chain is one wavefront's)
            const double x0[6] = {st[0], st[1], st[2], st[7], st[8], st[9]};
            double U[6], x[6];
            long_states(x0, A.steps, pl, tid, U, x, chain + kLongHead * 6);
            if (tid == 0)
#pragma unroll
                for (int r = 0; r < 6; ++r) xh[r] = x[r];
        }
        __syncthreads();
        const int cnt = (pl.G + kLongSubs - 1) / kLongSubs;     // <= kLongSplit: G <= 128
        for (int part = 0; part < cnt; ++part) {
            const int g0 = part * kLongSubs;
            const int c = pl.G - g0 < kLongSubs ? pl.G - g0 : kLongSubs;
            long_tangent_subchunks(chain, A.steps, pl, g0, tid, M);
            __syncthreads();
            long_ordered_product<128>(M, c, tid);
            if (tid < 36) Pm[part][tid] = M[0][tid];
            __syncthreads();
        }
        long_ordered_product<128>(Pm, cnt, tid);
        if (tid < 36) Phi[tid] = Pm[0][tid];
        __syncthreads();
    }
    if (tid != 0) return;
    schur_handoff_rotation(A.c, R);
    schur_handoff_transition(Phi, R, G);
    schur_handoff_congruence(G, A.Sigma, A.steps, A.noise, T, Sp);
    const bool ok = schur_handoff_cholinv(Sp, Lw, Ww, A.out + 10);
    double q[4];
    quat_mul(st + 3, A.c, q);
    const double inv = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int k = 0; k < 3; ++k) { A.out[k] = xh[k]; A.out[7 + k] = xh[3 + k]; }
    for (int k = 0; k < 4; ++k) A.out[3 + k] = q[k] * inv;
    A.out[91] = ok ? 0.0 : -1.0;
}

}  // namespace

void schur_prior_terms_launch(const SchurPriorView& W, const double* states, hipStream_t s) {
    hipLaunchKernelGGL(k_sprior_terms, dim3((W.count + 255) / 256), dim3(256), 0, s, W, states);
}

void schur_prior_scatter_launch(const SchurPriorView& W, hipStream_t s) {
    hipLaunchKernelGGL(k_sprior_scatter, dim3(W.count), dim3(64), 0, s, W);
}

void schur_prior_cost_launch(const SchurPriorView& W, const double* states, hipStream_t s) {
    hipLaunchKernelGGL(k_sprior_cost, dim3(W.npart), dim3(256), 0, s, W, states);
}

}  // namespace vba

SchurPriorView schur_prior_view(vba_schur_handle h, const SchurView& V, bool query) {
    const SchurPrior& P = h->prior;
    SchurPriorView W{};
    W.n = V.n; W.Npad = V.Npad; W.count = P.count; W.idx = P.idx; W.anchor = P.anchor; W.info = P.info;
    W.e = query ? P.q_e : P.e; W.J = query ? P.q_J : P.J; W.LF = query ? P.q_LF : P.LF; W.Le = query ? P.q_Le : P.Le;
    W.share = query ? P.q_share : P.share;
    W.part = P.part; W.npart = P.npart;     // (a query runs no cost kernel)
    W.S = V.S; W.g = V.g;
    return W;
}

static bool unit_quaternion(const double* q) {
    const double nn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    return std::isfinite(nn) && std::fabs(nn - 1.0) <= 1e-6;
}

extern "C" {

int vba_schur_enable_state_prior(vba_schur_handle h, int count, const int* pose_idx, const double* anchor, const double* info) {
    if (!h || !pose_idx || !anchor || !info) return sfail(VBA_EINVAL, "null argument");
    if (!h->uploaded) return sfail(VBA_ESTATE, "upload the problem first");
    if (!h->dyn.enabled) return sfail(VBA_ESTATE, "the state prior needs the dynamics factor: call vba_schur_enable_dynamics first");
    if (h->prior.enabled) return sfail(VBA_ESTATE, "the state prior is already enabled on this handle");
    const int n = h->V.n;
    if (count < 1 || count > n) return sfail(VBA_EINVAL, "count must be in 1 .. n");
    std::vector<char> seen(n, 0);
    for (int k = 0; k < count; ++k) {
        const std::string ks = std::to_string(k);
        const int i = pose_idx[k];
        if (i < 0 || i >= n) return sfail(VBA_EINVAL, "pose_idx entry " + ks + " is outside 0 .. n - 1");
        if (seen[i]) return sfail(VBA_EINVAL, "pose_idx entry " + ks + " repeats pose " + std::to_string(i) + ": one prior per pose");
        seen[i] = 1;
        const double* a = anchor + (size_t)k * 10;
        for (int c = 0; c < 10; ++c)
            if (!std::isfinite(a[c])) return sfail(VBA_EINVAL, "anchor " + ks + " is not finite");
        if (!unit_quaternion(a + 3)) return sfail(VBA_EINVAL, "the quaternion of anchor " + ks + " is not a unit quaternion (norm within 1e-6 of 1)");
        const double* L = info + (size_t)k * 81;
        double big = 0.0;
        for (int c = 0; c < 81; ++c) {
            if (!std::isfinite(L[c])) return sfail(VBA_EINVAL, "info block " + ks + " is not finite");
            big = std::max(big, std::fabs(L[c]));
        }
        for (int r = 0; r < 9; ++r) {
            if (L[9 * r + r] < 0.0) return sfail(VBA_EINVAL, "info block " + ks + " has a negative diagonal entry");
            for (int c = 0; c < r; ++c)
                if (std::fabs(L[9 * r + c] - L[9 * c + r]) > 1e-12 * big)
                    return sfail(VBA_EINVAL, "info block " + ks + " is not symmetric (to 1e-12 of its largest entry)");
        }
    }
    SCHK(hipSetDevice(h->device));
    SCHK(hipStreamSynchronize(h->stream));
    SchurPrior& P = h->prior;
    const size_t nc = (size_t)count;
    const int npart = (count + 255) / 256;
    SchurLayout lay;
    const size_t o_i = lay.need(nc * 4), o_an = lay.need(nc * 80), o_in = lay.need(nc * 648);
    const size_t o_e = lay.need(nc * 72), o_J = lay.need(nc * 72), o_LF = lay.need(nc * 648), o_Le = lay.need(nc * 72), o_sh = lay.need(nc * 8),
                 o_part = lay.need((size_t)npart * 8);
    const size_t o_qe = lay.need(nc * 72), o_qJ = lay.need(nc * 72), o_qLF = lay.need(nc * 648), o_qLe = lay.need(nc * 72), o_qsh = lay.need(nc * 8);
    const size_t bytes = lay.bytes;
    char* A = nullptr;
    if (hipMalloc(&A, bytes) != hipSuccess) { (void)hipGetLastError(); return sfail(VBA_ENOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes for the state prior failed"); }
    if (hipMemset(A, 0, bytes) != hipSuccess || hipMemcpy(A + o_i, pose_idx, nc * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(A + o_an, anchor, nc * 80, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(A + o_in, info, nc * 648, hipMemcpyHostToDevice) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess) {
        hipFree(A);
        return sfail(VBA_EHIP, "state prior: hipMemset / upload failed");
    }
    P.arena = A; P.count = count; P.npart = npart;
    P.idx = (int*)(A + o_i); P.anchor = (double*)(A + o_an); P.info = (double*)(A + o_in);
    P.e = (double*)(A + o_e); P.J = (double*)(A + o_J); P.LF = (double*)(A + o_LF); P.Le = (double*)(A + o_Le); P.share = (double*)(A + o_sh);
    P.part = (double*)(A + o_part);
    P.q_e = (double*)(A + o_qe); P.q_J = (double*)(A + o_qJ); P.q_LF = (double*)(A + o_qLF); P.q_Le = (double*)(A + o_qLe); P.q_share = (double*)(A + o_qsh);
    P.h_part.assign(npart, 0.0);
    P.enabled = true;
    return VBA_OK;
}

int vba_schur_handoff(vba_schur_handle h, double lamda, int steps, const double* cumrot_gap, const double* process_noise, double* anchor_out,
                      double* info_out, int* info) {
    if (!h || !cumrot_gap || !anchor_out || !info_out || !info) return sfail(VBA_EINVAL, "null argument");
    if (!(lamda >= 0.0)) return sfail(VBA_EINVAL, "lamda must be >= 0");
    if (steps < 1 || steps > VBA_MAX_GAP) return sfail(VBA_EINVAL, "steps must be in 1 .. VBA_MAX_GAP (2^20)");
    if (!unit_quaternion(cumrot_gap)) return sfail(VBA_EINVAL, "cumrot_gap is not a unit quaternion (finite, norm within 1e-6 of 1)");
    for (int k = 0; process_noise && k < 3; ++k)
        if (!(process_noise[k] >= 0.0) || !std::isfinite(process_noise[k])) return sfail(VBA_EINVAL, "process_noise must be non-negative and finite");
    if (int rc = schur_query_begin(h, kSchurDyn, nullptr)) return rc;
    SchurHandoff& H = h->handoff;
    if (!H.sc.arena) {
        SchurLayout lay;
        const size_t o_pool = lay.need((size_t)long_pool_states(long_plan(VBA_MAX_GAP)) * 48), o_out = lay.need(92 * 8);
        if (int rc = schur_scratch_alloc(H.sc, lay.bytes, "hand-off scratch")) return rc;
        H.pool = (double*)(H.sc.arena + o_pool); H.out = (double*)(H.sc.arena + o_out);
    }
    SchurQuery& Q = h->q;
    SchurView V;
    int bad = 0;
    if (int rc = schur_query_device(h, lamda, false, H.sc.ev[0], V, &bad)) return rc;
    double host[92];
    if (bad == 0) {
        vba::HandoffArgs A{};
        A.steps = steps;
        for (int k = 0; k < 4; ++k) A.c[k] = cumrot_gap[k];
        for (int k = 0; k < 3; ++k) A.noise[k] = process_noise ? process_noise[k] : 0.0;
        A.st = h->S0 + (size_t)(V.n - 1) * 10;
        A.Sigma = Q.state + (size_t)(V.n - 1) * 81;
        A.pool = H.pool; A.out = H.out;
        hipLaunchKernelGGL(vba::k_shandoff, dim3(1), dim3(128), 0, h->stream, A);
    }
    if (int rc = schur_scratch_finish(H.sc, h->stream, [&]() -> int {
            SCHK(hipGetLastError());
            if (bad == 0) SCHK(hipMemcpyAsync(host, H.out, sizeof(host), hipMemcpyDeviceToHost, h->stream));
            return VBA_OK;
        }))
        return rc;
    *info = bad != 0 ? bad : (host[91] != 0.0 ? -1 : 0);
    if (*info != 0) {
        std::fill(anchor_out, anchor_out + 10, std::nan(""));
        std::fill(info_out, info_out + 81, std::nan(""));
        return VBA_OK;
    }
    std::copy(host, host + 10, anchor_out);
    std::copy(host + 10, host + 91, info_out);
    return VBA_OK;
}

int vba_schur_last_handoff_ms(vba_schur_handle h, float* ms) { return schur_last_ms(h, &vba_schur_context::handoff, ms); }

}  // extern "C"
