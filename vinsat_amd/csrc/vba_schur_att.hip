// vba_schur_att.hip -- the Gauss-Newton attitude factor of the free-landmark mode (vba_schur_enable_attitude; ADD-ON, PARITY UNPINNED
// as the rest of the mode: vba_schur.hip carries the map of the units): its kernels, then the entry point.  Model, the relation to the
// reference's term and the scatter's work items: vba_schur_att_math.h.
//
// Kernels (no float atomics; every sum in a fixed order, so two runs and two handles leave the same bits):
//   k_satt_edges    thread per edge: a, J_own, J_next, sigma |a|^2 (a few quaternion products; the edges are few, n - 1)
//   k_satt_scatter  block per pose, thread per target entry (kSchurAttItems of them): edge i - 1's share, then edge i's; behind
//                   k_sdyn_scatter on the same stream
//   k_satt_cost     thread per edge: sigma |a|^2 at the given states, block partials
#include <hip/hip_runtime.h>

#include "vba_schur_context.h"
#include "vba_schur_att_math.h"

namespace vba {

namespace {

__global__ __launch_bounds__(256) void k_satt_edges(SchurAttView W, const double* states) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= W.n - 1) return;
    const double* st = states + (size_t)e * 10;
    double a[3], J[kSchurAttJ];
    const double n2 = schur_att_edge(st + 3, W.cumrot + (size_t)e * 4, st + 13, a, J);
#pragma unroll
    for (int k = 0; k < 3; ++k) W.a[(size_t)e * 3 + k] = a[k];
#pragma unroll
    for (int k = 0; k < kSchurAttJ; ++k) W.J[(size_t)e * kSchurAttJ + k] = J[k];
    W.ecost[e] = W.sigma * n2;
}

__global__ __launch_bounds__(64) void k_satt_scatter(SchurAttView W) {
    const int i = blockIdx.x, t = threadIdx.x;
    if (i >= W.n || t >= kSchurAttItems) return;
    schur_att_scatter_item(W.n, W.Npad, i, t, W.sigma, W.J, W.a, W.S, W.g);
}

__global__ __launch_bounds__(256) void k_satt_cost(SchurAttView W, const double* states) {
    __shared__ double red[4];
    const int e = blockIdx.x * 256 + threadIdx.x;
    double s = 0.0;
    if (e < W.n - 1) {
        const double* st = states + (size_t)e * 10;
        double w[4], a[3];
        s = W.sigma * schur_att_residual(st + 3, W.cumrot + (size_t)e * 4, st + 13, w, a);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) W.part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

}  // namespace

void schur_att_edges_launch(const SchurAttView& W, const double* states, hipStream_t s) {
    hipLaunchKernelGGL(k_satt_edges, dim3((W.n - 1 + 255) / 256), dim3(256), 0, s, W, states);
}

void schur_att_scatter_launch(const SchurAttView& W, hipStream_t s) {
    hipLaunchKernelGGL(k_satt_scatter, dim3(W.n), dim3(64), 0, s, W);
}

void schur_att_cost_launch(const SchurAttView& W, const double* states, hipStream_t s) {
    hipLaunchKernelGGL(k_satt_cost, dim3(W.npart), dim3(256), 0, s, W, states);
}

}  // namespace vba

SchurAttView schur_att_view(vba_schur_handle h, const SchurView& V, bool query) {
    const SchurAtt& T = h->att;
    SchurAttView W{};
    W.n = V.n; W.Npad = V.Npad; W.sigma = T.sigma; W.cumrot = T.cumrot;
    W.a = query ? T.q_a : T.a; W.J = query ? T.q_J : T.J; W.ecost = query ? T.q_ecost : T.ecost; W.part = query ? T.q_part : T.part;
    W.npart = T.npart;
    W.S = V.S; W.g = V.g;
    return W;
}

extern "C" int vba_schur_enable_attitude(vba_schur_handle h, const double* cumrot, double sigma_att) {
    if (!h || !cumrot) return sfail(VBA_EINVAL, "null argument");
    if (!h->uploaded) return sfail(VBA_ESTATE, "upload the problem first");
    if (!h->dyn.enabled) return sfail(VBA_ESTATE, "the attitude factor needs the dynamics factor: call vba_schur_enable_dynamics first");
    if (h->att.enabled) return sfail(VBA_ESTATE, "the attitude factor is already enabled on this handle");
    if (!(sigma_att > 0.0) || !std::isfinite(sigma_att)) return sfail(VBA_EINVAL, "sigma_att must be positive and finite");
    const int n = h->V.n;           // (>= 2: vba_schur_enable_dynamics refused less)
    for (int i = 0; i + 1 < n; ++i) {
        const double* c = cumrot + (size_t)i * 4;
        const double nn = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2] + c[3] * c[3]);
        if (!std::isfinite(nn) || std::fabs(nn - 1.0) > 1e-6)
            return sfail(VBA_EINVAL, "cumrot row " + std::to_string(i) + " is not a unit quaternion (finite, norm within 1e-6 of 1)");
    }
    SCHK(hipSetDevice(h->device));
    SCHK(hipStreamSynchronize(h->stream));
    SchurAtt& T = h->att;
    const size_t ne = (size_t)n - 1;
    const int npart = schur_dyn_partials(n);
    SchurLayout lay;
    const size_t o_c = lay.need((size_t)n * 32);
    const size_t o_a = lay.need(ne * 24), o_J = lay.need(ne * kSchurAttJ * 8), o_ec = lay.need(ne * 8), o_part = lay.need((size_t)npart * 8);
    const size_t o_qa = lay.need(ne * 24), o_qJ = lay.need(ne * kSchurAttJ * 8), o_qec = lay.need(ne * 8), o_qpart = lay.need((size_t)npart * 8);
    const size_t bytes = lay.bytes;
    char* A = nullptr;
    if (hipMalloc(&A, bytes) != hipSuccess) { (void)hipGetLastError(); return sfail(VBA_ENOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes for the attitude factor failed"); }
    // (row n - 1 of cumrot is ignored: it stays zero on the device and no kernel reads it)
    if (hipMemset(A, 0, bytes) != hipSuccess || hipMemcpy(A + o_c, cumrot, ne * 32, hipMemcpyHostToDevice) != hipSuccess ||
        hipStreamSynchronize(nullptr) != hipSuccess) {
        hipFree(A);
        return sfail(VBA_EHIP, "attitude factor: hipMemset / upload failed");
    }
    // the reliability scratch of a query before this call has no room for the attitude edges, so it goes: vba_schur_reliability_dyn
    // refuses this handle from now on, and vba_schur_reliability_att allocates it anew
    schur_scratch_release(h->rel.sc);
    h->rel = SchurRel{};
    T.arena = A; T.sigma = sigma_att; T.npart = npart;
    T.cumrot = (double*)(A + o_c);
    T.a = (double*)(A + o_a); T.J = (double*)(A + o_J); T.ecost = (double*)(A + o_ec); T.part = (double*)(A + o_part);
    T.q_a = (double*)(A + o_qa); T.q_J = (double*)(A + o_qJ); T.q_ecost = (double*)(A + o_qec); T.q_part = (double*)(A + o_qpart);
    T.h_part.assign(npart, 0.0);
    T.enabled = true;
    return VBA_OK;
}
