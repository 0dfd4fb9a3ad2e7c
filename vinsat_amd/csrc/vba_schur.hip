// vba_schur.hip -- free-landmark bundle adjustment with a Schur-complement solve (ADD-ON, PARITY UNPINNED).
//
// The reference keeps its landmarks fixed (estimation/BA/BA_filtering.py:32-37): every observation touches only the
// 6x6 block of its own pose and there is nothing to marginalise.  This file is the variant BASELINE.json's north_star
// describes on top of that: the landmarks become unknowns (3 each, held by a catalogue prior N(X0, sigma^2 I)), the
// normal equations
//        [ B   E ] [dc]   [v]        B: 6x6 per pose,   C: 3x3 per landmark,   E: 6x3 per observation
//        [ E^T C ] [dl] = [w]
// are reduced to the cameras,  S = B - E C^-1 E^T,  g = v - E C^-1 w,  the dense reduced camera system S dc = g is
// factorised on the matrix cores (blocked Cholesky, v_mfma_f64_16x16x4), and the landmarks follow by back substitution
// dl = C^-1 (w - E^T dc).  It has NO counterpart in the reference; it is checked against this repository's own CPU
// restatement (oracle/schur_oracle.py) only and never runs inside vba_iterate / BA().
//
// Reprojection and its pose Jacobian are the reference's (vba_math.h: BA_utils.py:30-49); the landmark Jacobian is
// d uv / d X = A R^T = -(translation part of the pose Jacobian).  Weights are the observation confidences (the
// reference's alpha = 2 case, BA_filtering.py:22-25, where the robust weight is constant) until vba_schur_reweight is called.
//
// Units (vba_schur_context.h is what they share: the view, the handle, error reporting, the scratch of a feature, the scaffold of
// the query entries):
//   vba_schur.hip         this file: the handle's lifecycle, one LM trial (vba_schur_iterate), substitutions, update, cost; the scaffold
//                         of the eleven query entries (schur_kind_check: which kind of handle an entry serves; schur_query_begin: what
//                         runs before a device part; schur_outputs_finish: NaN or the copies to the host; schur_last_ms in the header)
//   vba_schur_build.hip   k_lm_blocks, k_pose_blocks, k_pair_blocks, k_pad_identity
//   vba_schur_factor.hip  k_potrf64, k_potrf64b, k_gemm_abt, k_syrk_panel and the order of their launches
//   vba_schur_cov.hip     vba_schur_covariance, vba_schur_covariance_dyn behind one device part (schur_query_device, the handle decides):
//                         k_trinv_step, k_syrk_wtw, k_cov_gather, k_lm_cov; with the dynamics factor k_syrk_wtw_sel, k_state_gather (index
//                         map and tile list: vba_schur_dyn_cov.h)
//   vba_schur_rel.hip     vba_schur_reliability, _dyn, _att behind one body and one device part (schur_rel_call, schur_rel_device, folded
//                         over the kind of handle): k_rel_rows, k_rel_stats, k_rel_totals; with the dynamics factor k_rel_edges,
//                         k_rel_edge_totals (vba_schur_dyn_rel.h); with the attitude factor k_rel_att_edges, k_rel_att_totals
//                         (vba_schur_att_rel.h)
//   vba_schur_power.hip   vba_schur_outlier_power, _dyn, _att behind schur_power_call: k_pow_rows (in the place of k_rel_rows: one gather per
//                         row, vba_schur_rowpass.h), k_pow_stats, k_pow_totals (closed forms: vba_power_math.h, vba_schur_power_math.h)
//   vba_schur_snoop.hip   vba_schur_snoop, _dyn, _att behind schur_snoop_call, vba_schur_rejected, vba_schur_snoop_restore and their passes
//   vba_schur_robust.hip  vba_schur_reweight, vba_schur_get_weights, vba_schur_median and their passes
//   vba_schur_dyn.hip     vba_schur_enable_dynamics and the kernels of the factor
//   vba_schur_dyn_long.hip  vba_schur_enable_dynamics_long, vba_schur_long_edges and the kernels of the edges of more than 64 steps: parallel
//                         in time (bodies shared with the fixed-landmark path: vba_long_body.h; the host's plan: vba_schur_dyn_long.h)
//   vba_schur_att.hip     vba_schur_enable_attitude and the kernels of the Gauss-Newton attitude factor (bodies: vba_schur_att_math.h)
//   vba_schur_prior.hip   vba_schur_enable_state_prior and the kernels of the state prior factor; vba_schur_handoff and its kernel: the last
//                         pose's marginal across a gap into the prior of the next window (bodies: vba_schur_prior_math.h)
//
// Kernels (all reductions in a fixed order -- no float atomics):
//   k_lm_blocks     thread per landmark: C_l, w_l over its rows, C_l^-1, then E_k and Y_k = E_k C_l^-1 per row
//   k_pose_blocks   16 lanes per pose: B_i, v_i over its rows, g_i = v_i - sum Y_k w_l; diagonal block of S
//   k_pair_blocks   wave per (i, j) block of S: S_ij -= sum over the rows pairs sharing a landmark of Y_k E_k'^T
//   k_potrf64       64x64 diagonal block: Cholesky factor and its inverse (one workgroup, LDS)
//   k_gemm_abt      64x64x64 tiles on the matrix cores: panel = A inv(L)^T (MODE 0), trailing S_IJ -= L_I L_J^T (MODE 1)
//   k_trsv_step     one tile step of the forward / backward substitution (stored inverse diagonal factors), a launch per step
//   k_lm_update     dl, new landmarks, new poses (retraction as BA_filtering.py:56-60)
//   k_cost          sum w |r|^2 + prior, block partials
// Covariance query (vba_schur_covariance: build and factor into scratch of its own, then)
//   k_trinv_step    W = Lg^-1 on the matrix cores, a launch per tile distance from the diagonal, products beyond the band skipped
//   k_syrk_wtw      S^-1 = W^T W on the matrix cores, block per tile of the lower triangle
//   k_cov_gather    the listed 6x6 blocks of S^-1 (pair_cov) and its diagonal blocks (pose_cov)
//   k_lm_cov        thread per landmark: C_l^-1 + sum Y_k^T Sigma_{pose(k), pose(k')} Y_k'
// State covariances of a handle with the dynamics factor (vba_schur_covariance_dyn: build, factor, k_trinv_step as above, then)
//   k_syrk_wtw_sel  the tiles of S9^-1 = W^T W that an output reads, block per listed tile, the bits of k_syrk_wtw
//   k_state_gather  the 9x9 blocks [dp, dtheta, dv] of every pose and of every pair of consecutive poses
// Reliability query (vba_schur_reliability: the device part of the covariance query, then)
//   k_rel_rows      thread per row: pose-landmark cross-covariance Sigma_il from the gathered blocks and Y, leverage and w-test
//   k_rel_stats     thread per landmark / per pose: their rows' statistics; the catalogue prior of a landmark as an observation
//   k_rel_totals    one block: cost, redundancy, variance factor, largest tests (strided partial sums, one tree)
// Reliability of a handle with the dynamics factor (vba_schur_reliability_dyn: the device part of vba_schur_covariance_dyn,
// k_rel_rows and k_rel_stats as above, then)
//   k_rel_edges        eight lanes per dynamics edge, six at work: a diagonal entry of J Sigma12 J^T each, the edge's leverage
//   k_rel_edge_totals  one block behind k_rel_totals: the edges' leverages and cost shares folded into the fit
// Reliability of a handle with the attitude factor too (vba_schur_reliability_att: the launches above in their order, then)
//   k_rel_att_edges    thread per attitude edge: P_a from the attitude components of the 9x9 blocks, its leverage and w-test
//   k_rel_att_totals   one block behind k_rel_edge_totals: the attitude edges' leverages, cost shares and largest test folded into the fit
// Outlier power (vba_schur_outlier_power, _dyn, _att: the device part of the reliability query of the handle's kind with k_pow_rows
// as its row pass, then)
//   k_pow_rows      thread per row: the gather and P_k of k_rel_rows (lev, wt, om with its bits), then B_k = w Sigma_k J_k^T, detectable
//                   bias, external reliability in position, attitude and landmark, the row's influence, the pull of the prior
//   k_pow_stats     thread per landmark: detectable catalogue error, its effect on the landmark, the worst-hit pose; per pose: pose_fit
//   k_pow_totals    one block: the fit of the reliability query and four slots behind it (the tree of k_rel_totals)
// Data snooping (vba_schur_snoop, _dyn, _att: the device part of the reliability query of the handle's kind, then the passes of
// vba_schur_snoop.hip)
// Robust re-weighting (vba_schur_reweight, vba_schur_median: the passes of vba_schur_robust.hip)
// Orbit-dynamics factor with velocity unknowns (vba_schur_enable_dynamics: the kernels of vba_schur_dyn.hip; the reduced system
// becomes [6 n pose | 3 n velocity] unknowns, the build and factor kernels fill and factorise it unchanged)
// Long gaps of that factor (vba_schur_enable_dynamics_long: behind k_sdyn_edges, for the edges of more than 64 steps only)
//   k_sdyn_long_chain    wave per long edge: the parareal chain from the edge's start state into its pool slot, unless it is there
//   k_sdyn_long_tangent  eight workgroups of 128 per long edge: transition matrices of 16 sub-chunks each, their ordered product
//   k_sdyn_long_finish   wave per long edge: Phi from the partial products; A = D Phi, r, ecost at the edge's index
//   k_sdyn_long_cost     wave per long edge: sigma |r|^2 at the states given into a partial slot of its own; the chain stays in the pool
// Gauss-Newton attitude factor on such a handle (vba_schur_enable_attitude: the kernels of vba_schur_att.hip behind those of the orbit
// factor, in the build and in the cost; symmetric positive semidefinite blocks on the attitude unknowns, the same Cholesky)
// State prior factor on a dynamics handle (vba_schur_enable_state_prior: the kernels of vba_schur_prior.hip behind those of the other
// factors, in the build and in the cost; symmetric blocks on the 9x9 state blocks of the chosen poses, the same Cholesky)
//   k_sprior_terms    thread per prior: e, J, Lambda F, Lambda e and the cost share
//   k_sprior_scatter  block per prior, thread per target entry (45 of S, 9 of g): one owner per entry
//   k_sprior_cost     thread per prior: e^T Lambda e at the given states, block partials
// Window hand-off (vba_schur_handoff: the device part of vba_schur_covariance_dyn, then)
//   k_shandoff        one workgroup: (p, v) of the last pose over the gap with Phi (the six-tangent lanes up to 64 steps, the bodies of
//                     vba_long_body.h beyond), G Sigma G^T + noise, its inverse by a 9x9 Cholesky, the anchor
#include "vba_schur_context.h"
#include "vba_schur_dyn_long.h"

namespace {

// The shape of the factorisation where tests/schur_cases.py reads it (kernel_constants: its cases reach their branches for 64 x 4
// only).  The units take it from vba_schur_context.h; the two cannot drift apart.
namespace shape {
constexpr int kT = 64;
constexpr int kPanel = 4;
static_assert(kT == ::kT && kPanel == ::kPanel, "vba_schur_context.h and the shape on record in vba_schur.hip disagree");
}  // namespace shape

// One tile step of the forward (L y = g) / backward (L^T x = y) substitution, a launch per step (as the factorisation):
// block 0 forms the step's 64 solution entries from the stored inverse diagonal factor, every other block forms them too
// (a 64x64 product, cheaper than a hand-off) and updates ONE tile of the right-hand side with them.  Tiles further than bw
// from the diagonal are zero (the factor of a banded matrix keeps its band) and get no block.
//   forward:  y_kb = invL_kb g_kb (-> ybuf),  g_I    -= L_{I,kb}   y_kb   for kb < I <= kb + bw
//   backward: x_kb = invL_kb^T ybuf_kb (-> g), ybuf_J -= L_{kb,J}^T x_kb   for kb - bw <= J < kb
__global__ __launch_bounds__(256) void k_trsv_step(SchurView V, int kb, int backward) {
    __shared__ double xb[kT];
    __shared__ double gb[kT];
    __shared__ double part[4][kT];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const double* Li = V.invL + (size_t)kb * kT * kT;
    const double* rhs = backward ? V.ybuf : V.g;
    if (t < kT) gb[t] = rhs[kb * kT + t];
    __syncthreads();
    for (int e = wv; e < kT; e += 4) {      // entry e: a 64-term dot product by one wave
        double sdot = backward ? Li[(size_t)lane * kT + e] * gb[lane] : Li[(size_t)e * kT + lane] * gb[lane];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sdot += __shfl_xor(sdot, o, 64);
        if (lane == 0) xb[e] = sdot;
    }
    __syncthreads();
    if (blockIdx.x == 0) {
        if (t < kT) (backward ? V.g : V.ybuf)[kb * kT + t] = xb[t];
        return;
    }
    if (!backward) {
        const int I = kb + (int)blockIdx.x;
        // rows of the tile over the waves, lanes over its columns (64 consecutive doubles per load)
        for (int rr = wv; rr < kT; rr += 4) {
            const size_t row = (size_t)I * kT + rr;
            double sdot = V.S[row * V.Npad + kb * kT + lane] * xb[lane];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) sdot += __shfl_xor(sdot, o, 64);
            if (lane == 0) V.g[row] -= sdot;
        }
    } else {
        const int J = kb - (int)blockIdx.x;
        // lanes over the tile's columns (= entries of ybuf_J), the 64 rows split over the waves, partial sums through LDS
        double sdot = 0.0;
        for (int c = wv; c < kT; c += 4) sdot = fma(V.S[(size_t)(kb * kT + c) * V.Npad + J * kT + lane], xb[c], sdot);
        part[wv][lane] = sdot;
        __syncthreads();
        if (wv == 0) V.ybuf[J * kT + lane] -= ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
    }
}

// ------------------------------------------------------------------------------------------------ update / cost
__global__ __launch_bounds__(256) void k_lm_update(SchurView V) {
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id < V.L) {
        const int l = id;
        double s[3] = {V.wl[3 * l], V.wl[3 * l + 1], V.wl[3 * l + 2]};
        for (int k = V.lm_ptr[l]; k < V.lm_ptr[l + 1]; ++k) {
            const double* Ek = V.E + (size_t)k * 18;
            const double* dc = V.g + 6 * V.row_pose[k];
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int a = 0; a < 6; ++a) s[c] -= Ek[3 * a + c] * dc[a];
        }
        const double* Ci = V.Cinv + (size_t)l * 6;
        const double d0 = Ci[0] * s[0] + Ci[1] * s[1] + Ci[2] * s[2];
        const double d1 = Ci[1] * s[0] + Ci[3] * s[1] + Ci[4] * s[2];
        const double d2 = Ci[2] * s[0] + Ci[4] * s[1] + Ci[5] * s[2];
        V.dl[3 * l] = d0; V.dl[3 * l + 1] = d1; V.dl[3 * l + 2] = d2;
        V.X_new[3 * l] = V.X[3 * l] + d0;
        V.X_new[3 * l + 1] = V.X[3 * l + 1] + d1;
        V.X_new[3 * l + 2] = V.X[3 * l + 2] + d2;
    }
    if (id < V.n) {
        const double* dc = V.g + 6 * id;
        const double d9[9] = {dc[0], dc[1], dc[2], dc[3], dc[4], dc[5], 0.0, 0.0, 0.0};
        double o[10];
        retract(V.states + (size_t)id * 10, d9, o);
#pragma unroll
        for (int r = 0; r < 10; ++r) V.states_new[(size_t)id * 10 + r] = o[r];
    }
}

// cost at (states, X) given as arguments: sum w (ru^2 + rv^2) over rows + inv_sigma2 |X - X0|^2 over landmarks
__global__ __launch_bounds__(256) void k_cost(SchurView V, const double* states, const double* X) {
    __shared__ double red[4];
    const int id = blockIdx.x * 256 + threadIdx.x;
    double s = 0.0;
    if (id < V.m) {
        RowGeom q;
        row_geometry(V, states, X, id, q);
        s = V.row_w[id] * (q.ru * q.ru + q.rv * q.rv);
    }
    if (id < V.L) {
        const double dx = X[3 * id] - V.X0[3 * id], dy = X[3 * id + 1] - V.X0[3 * id + 1], dz = X[3 * id + 2] - V.X0[3 * id + 2];
        s += V.inv_sigma2 * (dx * dx + dy * dy + dz * dz);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) V.part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

thread_local std::string g_serr;

}  // namespace

int sfail(int code, const std::string& msg) { g_serr = msg; return code; }

// ------------------------------------------------------------------------------------------------ scratch of a feature
int schur_scratch_alloc(SchurScratch& Z, size_t bytes, const char* what) {
    char* A = nullptr;
    if (hipMalloc(&A, bytes) != hipSuccess) { (void)hipGetLastError(); return sfail(VBA_ENOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes of " + what + " failed"); }
    hipEvent_t ev[2] = {};
    if (hipMemset(A, 0, bytes) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess || hipEventCreate(&ev[0]) != hipSuccess ||
        hipEventCreate(&ev[1]) != hipSuccess) {
        if (ev[0]) hipEventDestroy(ev[0]);
        hipFree(A);
        return sfail(VBA_EHIP, std::string(what) + ": hipMemset / event creation failed");
    }
    Z.arena = A; Z.ev[0] = ev[0]; Z.ev[1] = ev[1];
    return VBA_OK;
}

void schur_scratch_release(SchurScratch& Z) {
    for (hipEvent_t e : Z.ev) if (e) hipEventDestroy(e);
    if (Z.arena) hipFree(Z.arena);
    Z = SchurScratch{};
}

// ------------------------------------------------------------------------------------------------ scaffold of the query entries
int schur_kind_check(SchurKind kind, vba_schur_handle h, const char* entry) {
    if (kind == kSchurPlain) return h->dyn.enabled ? sfail(VBA_ESTATE, std::string(entry) + kDynRefusal) : VBA_OK;
    if (!h->dyn.enabled) return sfail(VBA_ESTATE, "the dynamics factor is not enabled on this handle");
    if (kind == kSchurAtt && !h->att.enabled) return sfail(VBA_ESTATE, "the attitude factor is not enabled on this handle");
    if (kind == kSchurDyn && h->att.enabled && entry) return sfail(VBA_ESTATE, std::string(entry) + kAttRefusal);
    // (behind the checks above: their messages and their order are pinned)
    if (entry && h->prior.enabled) {
        std::string name(entry);
        if (kind == kSchurAtt) name.replace(name.size() - 3, 3, "att");    // (an _att entry passes the name of its _dyn counterpart)
        return sfail(VBA_ESTATE, name + kPriorRefusal);
    }
    return VBA_OK;
}

int schur_query_begin(vba_schur_handle h, SchurKind kind, const char* entry) {
    if (!h->uploaded || !h->have_state) return sfail(VBA_ESTATE, "upload the problem and set the state first");
    if (int rc = schur_kind_check(kind, h, entry)) return rc;
    SCHK(hipSetDevice(h->device));
    if (int rc = schur_query_alloc(h)) return rc;
    return schur_query_index(h);
}

int schur_outputs_finish(SchurScratch& Z, hipStream_t s, int bad, const Out* outs, size_t count) {
    if (bad != 0) {
        if (int rc = schur_scratch_finish(Z, s)) return rc;
        for (size_t k = 0; k < count; ++k)
            if (outs[k].host) std::fill(outs[k].host, outs[k].host + outs[k].count, std::nan(""));
        return VBA_OK;
    }
    return schur_scratch_finish(Z, s, [&]() -> int {
        SCHK(hipGetLastError());
        for (size_t k = 0; k < count; ++k)
            if (outs[k].host) SCHK(hipMemcpyAsync(outs[k].host, outs[k].dev, outs[k].count * 8, hipMemcpyDeviceToHost, s));
        return VBA_OK;
    });
}

// trial: the states are those of a trial (the chains of the long edges go where an accepted trial's next build finds them; the chains
// of the resident states where this call's build does)
static int schur_cost(vba_schur_handle h, const double* states, const double* X, double* cost, bool trial) {
    SchurView V = h->V;
    SchurDyn& D = h->dyn;
    SchurAtt& T = h->att;
    SchurPrior& P = h->prior;
    if (trial) SCHK(hipEventRecord(h->ev[0], h->stream));        // (the build's interval was read before the trial's cost began)
    hipLaunchKernelGGL(k_cost, dim3(V.npart), dim3(256), 0, h->stream, V, states, X);
    if (D.enabled) schur_dyn_cost_launch(schur_dyn_view(h, V), states, h->stream);
    if (D.nlong > 0) schur_dyn_long_cost_launch(schur_dyn_view(h, V), states, trial ? D.par ^ 1 : D.par, h->stream);
    if (T.enabled) schur_att_cost_launch(schur_att_view(h, V), states, h->stream);
    if (P.enabled) schur_prior_cost_launch(schur_prior_view(h, V), states, h->stream);
    SCHK(hipGetLastError());
    if (trial) SCHK(hipEventRecord(h->ev[4], h->stream));
    SCHK(hipMemcpyAsync(h->h_part.data(), V.part, (size_t)V.npart * 8, hipMemcpyDeviceToHost, h->stream));
    if (D.enabled) SCHK(hipMemcpyAsync(D.h_part.data(), D.part, (size_t)(D.npart + D.nlong) * 8, hipMemcpyDeviceToHost, h->stream));
    if (T.enabled) SCHK(hipMemcpyAsync(T.h_part.data(), T.part, (size_t)T.npart * 8, hipMemcpyDeviceToHost, h->stream));
    if (P.enabled) SCHK(hipMemcpyAsync(P.h_part.data(), P.part, (size_t)P.npart * 8, hipMemcpyDeviceToHost, h->stream));
    SCHK(hipStreamSynchronize(h->stream));
    if (trial) (void)hipEventElapsedTime(&h->ms[3], h->ev[0], h->ev[4]);
    double s = 0.0;
    for (int b = 0; b < V.npart; ++b) s += h->h_part[b];      // fixed order
    if (D.enabled) for (int b = 0; b < D.npart + D.nlong; ++b) s += D.h_part[b];   // ... the dynamics partials after the rows' and the prior's (the long edges' behind the blocks')
    if (T.enabled) for (int b = 0; b < T.npart; ++b) s += T.h_part[b];     // ... and the attitude partials after those
    if (P.enabled) for (int b = 0; b < P.npart; ++b) s += P.h_part[b];     // ... and the state prior's last
    *cost = s;
    return VBA_OK;
}

// Build the reduced camera system of the view's state and damping and factorise it, on stream s (the bulk of a panel's trailing
// update beside it on h->aux): S, g, Cinv, wl, E, Y, invL and *d_info are the view's and the caller's, so vba_schur_iterate runs it
// on the handle's arrays and vba_schur_covariance on scratch of its own.  ev_built (if given) is recorded between the two parts;
// dyn, att and prior (if given) stand for the handle's dynamics, attitude and state prior arrays in the build.
int schur_build_factor(vba_schur_handle h, const SchurView& V, hipStream_t s, int* d_info, hipEvent_t ev_built, const SchurDynView* dyn,
                       const SchurAttView* att, const SchurPriorView* prior) {
    SCHK(hipMemsetAsync(V.S, 0, (size_t)V.Npad * V.Npad * 8, s));
    SCHK(hipMemsetAsync(V.g, 0, (size_t)V.Npad * 8, s));
    SCHK(hipMemsetAsync(d_info, 0, 4, s));
    schur_build_launch(h, V, s, dyn, att, prior);
    if (ev_built) SCHK(hipEventRecord(ev_built, s));
    return schur_factor_launch(h, V, s, d_info);
}

extern "C" {

const char* vba_schur_last_error(void) { return g_serr.c_str(); }

int vba_schur_create(int device, int n, int64_t m, int L, int nblk, int64_t npairs, vba_schur_handle* out) {
    if (!out) return sfail(VBA_EINVAL, "null out");
    *out = nullptr;
    if (n < 1 || m < 1 || L < 1 || nblk < n || npairs < m) return sfail(VBA_EINVAL, "sizes out of range");
    if (m > INT32_MAX || npairs > INT32_MAX) return sfail(VBA_EINVAL, "m and npairs must fit 32-bit indices (CSR and pair lists are int32)");
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt == 0) return sfail(VBA_ENODEV, "no HIP device visible");
    if (device < 0 || device >= cnt) return sfail(VBA_EINVAL, "device index out of range");
    SCHK(hipSetDevice(device));
    vba_schur_context* h = new (std::nothrow) vba_schur_context();
    if (!h) return sfail(VBA_ENOMEM, "host allocation failed");
    h->device = device;
    SchurView& V = h->V;
    V.n = n; V.m = m; V.L = L; V.nblk = nblk;
    V.N = 6 * n;
    schur_padded_size(V.N, V.nb, V.Npad);
    V.npart = (int)((std::max<int64_t>(m, L) + 255) / 256);
    h->npairs = npairs;
    SchurLayout lay;
    const size_t o_lmptr = lay.need((size_t)(L + 1) * 4), o_rpose = lay.need(m * 4), o_rlm = lay.need(m * 4), o_u = lay.need(m * 8), o_v = lay.need(m * 8),
                 o_w = lay.need(m * 8);
    const size_t o_pptr = lay.need((size_t)(n + 1) * 4), o_prows = lay.need(m * 4);
    const size_t o_bi = lay.need((size_t)nblk * 4), o_bj = lay.need((size_t)nblk * 4), o_bptr = lay.need((size_t)(nblk + 1) * 4), o_pk = lay.need(npairs * 4),
                 o_pk2 = lay.need(npairs * 4);
    const size_t o_intr = lay.need((size_t)n * 32), o_X0 = lay.need((size_t)L * 24);
    const size_t o_s0 = lay.need((size_t)n * 80), o_s1 = lay.need((size_t)n * 80), o_x0 = lay.need((size_t)L * 24), o_x1 = lay.need((size_t)L * 24);
    const size_t o_ci = lay.need((size_t)L * 48), o_wl = lay.need((size_t)L * 24), o_E = lay.need(m * 144), o_Y = lay.need(m * 144);
    const size_t o_S = lay.need((size_t)V.Npad * V.Npad * 8), o_g = lay.need((size_t)V.Npad * 8), o_y = lay.need((size_t)V.Npad * 8),
                 o_iL = lay.need((size_t)V.nb * kT * kT * 8);
    const size_t o_dl = lay.need((size_t)L * 24), o_part = lay.need((size_t)V.npart * 8), o_info = lay.need(256);
    const size_t bytes = lay.bytes;
    if (hipMalloc(&h->arena, bytes) != hipSuccess) { delete h; return sfail(VBA_ENOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes failed"); }
    if (hipMemset(h->arena, 0, bytes) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess) { hipFree(h->arena); delete h; return sfail(VBA_EHIP, "hipMemset failed"); }
    char* A = h->arena;
    V.lm_ptr = (int*)(A + o_lmptr); V.row_pose = (int*)(A + o_rpose); V.row_lm = (int*)(A + o_rlm);
    V.row_u = (double*)(A + o_u); V.row_v = (double*)(A + o_v); V.row_w = (double*)(A + o_w);
    V.pose_ptr = (int*)(A + o_pptr); V.pose_rows = (int*)(A + o_prows);
    V.blk_i = (int*)(A + o_bi); V.blk_j = (int*)(A + o_bj); V.blk_ptr = (int*)(A + o_bptr); V.pair_k = (int*)(A + o_pk); V.pair_k2 = (int*)(A + o_pk2);
    V.intr = (double*)(A + o_intr); V.X0 = (double*)(A + o_X0);
    h->S0 = (double*)(A + o_s0); h->S1 = (double*)(A + o_s1); h->X0buf = (double*)(A + o_x0); h->X1buf = (double*)(A + o_x1);
    V.Cinv = (double*)(A + o_ci); V.wl = (double*)(A + o_wl); V.E = (double*)(A + o_E); V.Y = (double*)(A + o_Y);
    V.S = (double*)(A + o_S); V.g = (double*)(A + o_g); V.ybuf = (double*)(A + o_y); V.invL = (double*)(A + o_iL);
    V.dl = (double*)(A + o_dl); V.part = (double*)(A + o_part); h->d_info = (int*)(A + o_info);
    h->h_part.resize(V.npart);
    bool ok = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) == hipSuccess &&
              hipStreamCreateWithFlags(&h->aux, hipStreamNonBlocking) == hipSuccess &&
              hipEventCreateWithFlags(&h->ev_chain, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&h->ev_bulk, hipEventDisableTiming) == hipSuccess;
    if (const char* e = std::getenv("VBA_SCHUR_CLASSIC")) h->classic = std::atoi(e);
    if (const char* e = std::getenv("VBA_SCHUR_COV_FULL")) h->cov_full = std::atoi(e);
    for (int k = 0; k < 5 && ok; ++k) ok = hipEventCreate(&h->ev[k]) == hipSuccess;
    if (!ok) { vba_schur_destroy(h); return sfail(VBA_EHIP, "stream / event creation failed"); }
    *out = h;
    return VBA_OK;
}

int vba_schur_destroy(vba_schur_handle h) {
    if (!h) return VBA_OK;
    hipSetDevice(h->device);
    if (h->stream) { hipStreamSynchronize(h->stream); hipStreamDestroy(h->stream); }
    if (h->aux) { hipStreamSynchronize(h->aux); hipStreamDestroy(h->aux); }
    if (h->ev_chain) hipEventDestroy(h->ev_chain);
    if (h->ev_bulk) hipEventDestroy(h->ev_bulk);
    for (hipEvent_t e : h->ev) if (e) hipEventDestroy(e);
    if (h->dyn.arena) hipFree(h->dyn.arena);
    if (h->att.arena) hipFree(h->att.arena);
    if (h->prior.arena) hipFree(h->prior.arena);
    for (SchurScratch* z : {&h->handoff.sc, &h->robust.sc, &h->snoop.sc, &h->pow.sc, &h->rel.sc, &h->q.sc}) schur_scratch_release(*z);
    if (h->arena) hipFree(h->arena);
    delete h;
    return VBA_OK;
}

int vba_schur_upload(vba_schur_handle h, const int* lm_ptr, const int* row_pose, const int* row_lm, const double* row_u,
                     const double* row_v, const double* row_w, const int* pose_ptr, const int* pose_rows, const int* blk_i,
                     const int* blk_j, const int* blk_ptr, const int* pair_k, const int* pair_k2, const double* intrinsics,
                     const double* X0, double sigma_prior) {
    if (!h) return sfail(VBA_EINVAL, "null handle");
    if (!lm_ptr || !row_pose || !row_lm || !row_u || !row_v || !row_w || !pose_ptr || !pose_rows || !blk_i || !blk_j || !blk_ptr ||
        !pair_k || !pair_k2 || !intrinsics || !X0)
        return sfail(VBA_EINVAL, "null array");
    if (!(sigma_prior > 0.0)) return sfail(VBA_EINVAL, "sigma_prior must be positive");
    const SchurView& V = h->V;
    // the structure arrays index each other: check them on the host before a kernel trusts them
    if (lm_ptr[0] != 0 || lm_ptr[V.L] != V.m || pose_ptr[0] != 0 || pose_ptr[V.n] != V.m || blk_ptr[0] != 0 || blk_ptr[V.nblk] != h->npairs)
        return sfail(VBA_EINVAL, "CSR pointers do not span their arrays");
    for (int l = 0; l < V.L; ++l) if (lm_ptr[l + 1] < lm_ptr[l]) return sfail(VBA_EINVAL, "lm_ptr not monotone");
    for (int i = 0; i < V.n; ++i) if (pose_ptr[i + 1] < pose_ptr[i]) return sfail(VBA_EINVAL, "pose_ptr not monotone");
    for (int b = 0; b < V.nblk; ++b) {
        if (blk_ptr[b + 1] < blk_ptr[b]) return sfail(VBA_EINVAL, "blk_ptr not monotone");
        if (blk_i[b] < 0 || blk_i[b] >= V.n || blk_j[b] < 0 || blk_j[b] > blk_i[b]) return sfail(VBA_EINVAL, "block index outside the lower triangle");
    }
    for (int64_t k = 0; k < V.m; ++k) {
        if (row_pose[k] < 0 || row_pose[k] >= V.n || row_lm[k] < 0 || row_lm[k] >= V.L || pose_rows[k] < 0 || pose_rows[k] >= V.m)
            return sfail(VBA_EINVAL, "row index out of range");
    }
    for (int64_t p = 0; p < h->npairs; ++p)
        if (pair_k[p] < 0 || pair_k[p] >= V.m || pair_k2[p] < 0 || pair_k2[p] >= V.m) return sfail(VBA_EINVAL, "pair index out of range");
    SCHK(hipSetDevice(h->device));
    auto up = [&](const void* dst, const void* src, size_t bytes) { return hipMemcpy(const_cast<void*>(dst), src, bytes, hipMemcpyHostToDevice); };
    SCHK(up(V.lm_ptr, lm_ptr, (size_t)(V.L + 1) * 4)); SCHK(up(V.row_pose, row_pose, V.m * 4)); SCHK(up(V.row_lm, row_lm, V.m * 4));
    SCHK(up(V.row_u, row_u, V.m * 8)); SCHK(up(V.row_v, row_v, V.m * 8)); SCHK(up(V.row_w, row_w, V.m * 8));
    SCHK(up(V.pose_ptr, pose_ptr, (size_t)(V.n + 1) * 4)); SCHK(up(V.pose_rows, pose_rows, V.m * 4));
    SCHK(up(V.blk_i, blk_i, (size_t)V.nblk * 4)); SCHK(up(V.blk_j, blk_j, (size_t)V.nblk * 4)); SCHK(up(V.blk_ptr, blk_ptr, (size_t)(V.nblk + 1) * 4));
    SCHK(up(V.pair_k, pair_k, h->npairs * 4)); SCHK(up(V.pair_k2, pair_k2, h->npairs * 4));
    SCHK(up(V.intr, intrinsics, (size_t)V.n * 32)); SCHK(up(V.X0, X0, (size_t)V.L * 24));
    h->V.inv_sigma2 = 1.0 / (sigma_prior * sigma_prior);
    h->bw = 0;
    for (int b = 0; b < V.nblk; ++b) h->bw = std::max(h->bw, (6 * blk_i[b] + 5) / kT - (6 * blk_j[b]) / kT);
    if (h->dyn.enabled) h->bw = V.nb - 1;       // velocity rows reach every pose column
    h->q.indexed = false;
    if (h->snoop.sc.arena) {    // new weights: nothing is rejected
        SCHK(hipMemset(h->snoop.row_mask, 0, (size_t)V.m));
        SCHK(hipMemset(h->snoop.lm_mask, 0, (size_t)V.L));
        SCHK(hipStreamSynchronize(nullptr));
        std::fill(h->snoop.totals, h->snoop.totals + 3, 0);
    }
    h->robust.captured = h->robust.have_keys = false;       // new weights: they are the base of the next re-weighting
    h->uploaded = true;
    return VBA_OK;
}

int vba_schur_set_state(vba_schur_handle h, const double* states, const double* landmarks) {
    if (!h || !states || !landmarks) return sfail(VBA_EINVAL, "null argument");
    SCHK(hipSetDevice(h->device));
    SCHK(hipStreamSynchronize(h->stream));
    SCHK(hipMemcpy(h->S0, states, (size_t)h->V.n * 80, hipMemcpyHostToDevice));
    SCHK(hipMemcpy(h->X0buf, landmarks, (size_t)h->V.L * 24, hipMemcpyHostToDevice));
    h->have_state = true;
    return VBA_OK;
}

int vba_schur_get_state(vba_schur_handle h, double* states, double* landmarks) {
    if (!h) return sfail(VBA_EINVAL, "null handle");
    if (!h->have_state) return sfail(VBA_ESTATE, "no state set");
    SCHK(hipSetDevice(h->device));
    SCHK(hipStreamSynchronize(h->stream));
    if (states) SCHK(hipMemcpy(states, h->S0, (size_t)h->V.n * 80, hipMemcpyDeviceToHost));
    if (landmarks) SCHK(hipMemcpy(landmarks, h->X0buf, (size_t)h->V.L * 24, hipMemcpyDeviceToHost));
    return VBA_OK;
}

int vba_schur_iterate(vba_schur_handle h, double lamda, double* cost_before, double* cost_after, int* accepted) {
    if (!h || !cost_before || !cost_after || !accepted) return sfail(VBA_EINVAL, "null argument");
    if (!h->uploaded || !h->have_state) return sfail(VBA_ESTATE, "upload the problem and set the state first");
    if (!(lamda >= 0.0)) return sfail(VBA_EINVAL, "lamda must be >= 0");
    SCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    SchurView V = h->V;
    V.lamda = lamda;
    V.states = h->S0; V.X = h->X0buf; V.states_new = h->S1; V.X_new = h->X1buf;
    if (int rc = schur_cost(h, V.states, V.X, cost_before, false)) return rc;
    SCHK(hipEventRecord(h->ev[0], s));
    if (int rc = schur_build_factor(h, V, s, h->d_info, h->ev[1])) return rc;
    SCHK(hipEventRecord(h->ev[2], s));
    for (int kb = 0; kb < V.nb; ++kb)
        hipLaunchKernelGGL(k_trsv_step, dim3(1 + std::min(h->bw, V.nb - 1 - kb)), dim3(256), 0, s, V, kb, 0);
    for (int kb = V.nb - 1; kb >= 0; --kb)
        hipLaunchKernelGGL(k_trsv_step, dim3(1 + std::min(h->bw, kb)), dim3(256), 0, s, V, kb, 1);
    hipLaunchKernelGGL(k_lm_update, dim3((std::max(V.L, V.n) + 255) / 256), dim3(256), 0, s, V);
    if (h->dyn.enabled) schur_dyn_update_launch(schur_dyn_view(h, V), V.states, V.states_new, s);
    SCHK(hipEventRecord(h->ev[3], s));
    SCHK(hipGetLastError());
    int info = 0;
    SCHK(hipMemcpyAsync(&info, h->d_info, 4, hipMemcpyDeviceToHost, s));
    SCHK(hipStreamSynchronize(s));
    for (int k = 0; k < 3; ++k) (void)hipEventElapsedTime(&h->ms[k], h->ev[k], h->ev[k + 1]);
    h->last_info = info;
    if (info != 0) {
        // Not positive definite at this damping: the ordinary LM answer to a failed factorisation is a rejected trial (the
        // caller raises lamda), not an error.  The state is untouched; vba_schur_last_info reports the failing row.
        *cost_after = *cost_before;
        *accepted = 0;
        return VBA_OK;
    }
    if (int rc = schur_cost(h, V.states_new, V.X_new, cost_after, true)) return rc;
    *accepted = (*cost_after < *cost_before) ? 1 : 0;
    if (*accepted) { std::swap(h->S0, h->S1); std::swap(h->X0buf, h->X1buf); h->dyn.par ^= 1; }   // (the trial's chains are the next build's)
    return VBA_OK;
}

int vba_schur_last_info(vba_schur_handle h, int* info) {
    if (!h || !info) return sfail(VBA_EINVAL, "null argument");
    *info = h->last_info;
    return VBA_OK;
}

int vba_schur_last_ms(vba_schur_handle h, float* build_ms, float* factor_ms, float* solve_ms) {
    if (!h) return sfail(VBA_EINVAL, "null handle");
    if (build_ms) *build_ms = h->ms[0];
    if (factor_ms) *factor_ms = h->ms[1];
    if (solve_ms) *solve_ms = h->ms[2];
    return VBA_OK;
}

int vba_schur_last_trial_cost_ms(vba_schur_handle h, float* ms) {
    if (!h || !ms) return sfail(VBA_EINVAL, "null argument");
    *ms = h->ms[3];
    return VBA_OK;
}

// what: 0 = step of the last iteration [6 n + 3 L] (dc then dl), 1 = lower triangle of the Cholesky factor as a dense
// [N][N] row-major matrix (upper part zero; N = 6 n, or 9 n with the dynamics factor), 2 = the 2 m keys |r| of the last
// re-weighting; with the dynamics factor 3 = dv [n][3] of the last iteration, 4 = r [n - 1][6], 5 = D Phi [n - 1][6][6] and
// 6 = sigma_dyn |r_e|^2 [n - 1] of its build; with the attitude factor 7 = a [n - 1][3], 8 = the Jacobian pairs [n - 1][2][3][3] and
// 9 = sigma_att |a_e|^2 [n - 1] of its build; with the state prior 10 = e [count][9], 11 = J [count][3][3] and 12 = e^T Lambda e [count]
// of its build
int vba_schur_debug_fetch(vba_schur_handle h, int what, double* out, int64_t capacity) {
    if (!h || !out) return sfail(VBA_EINVAL, "null argument");
    SCHK(hipSetDevice(h->device));
    SCHK(hipStreamSynchronize(h->stream));
    const SchurView& V = h->V;
    if (what == 0) {
        const int64_t n6 = 6 * (int64_t)V.n;      // (the pose unknowns come first, with or without the velocities behind them)
        if (capacity < n6 + 3 * (int64_t)V.L) return sfail(VBA_EINVAL, "buffer too small");
        SCHK(hipMemcpy(out, V.g, (size_t)n6 * 8, hipMemcpyDeviceToHost));
        SCHK(hipMemcpy(out + n6, V.dl, (size_t)V.L * 24, hipMemcpyDeviceToHost));
        return VBA_OK;
    }
    if (what >= 3 && what <= 6) {
        const SchurDyn& D = h->dyn;
        if (!D.enabled) return sfail(VBA_ESTATE, "the dynamics factor is not enabled on this handle");
        const int64_t n = V.n;
        const double* src[4] = {V.g + 6 * n, D.r, D.A, D.ecost};
        const int64_t count[4] = {3 * n, 6 * (n - 1), 36 * (n - 1), n - 1};
        if (capacity < count[what - 3]) return sfail(VBA_EINVAL, "buffer too small");
        SCHK(hipMemcpy(out, src[what - 3], (size_t)count[what - 3] * 8, hipMemcpyDeviceToHost));
        return VBA_OK;
    }
    if (what >= 7 && what <= 9) {
        const SchurAtt& T = h->att;
        if (!T.enabled) return sfail(VBA_ESTATE, "the attitude factor is not enabled on this handle");
        const int64_t ne = (int64_t)V.n - 1;
        const double* src[3] = {T.a, T.J, T.ecost};
        const int64_t count[3] = {3 * ne, 18 * ne, ne};
        if (capacity < count[what - 7]) return sfail(VBA_EINVAL, "buffer too small");
        SCHK(hipMemcpy(out, src[what - 7], (size_t)count[what - 7] * 8, hipMemcpyDeviceToHost));
        return VBA_OK;
    }
    if (what >= 10 && what <= 12) {
        const SchurPrior& P = h->prior;
        if (!P.enabled) return sfail(VBA_ESTATE, "the state prior is not enabled on this handle");
        const double* src[3] = {P.e, P.J, P.share};
        const int64_t count[3] = {9 * (int64_t)P.count, 9 * (int64_t)P.count, P.count};
        if (capacity < count[what - 10]) return sfail(VBA_EINVAL, "buffer too small");
        SCHK(hipMemcpy(out, src[what - 10], (size_t)count[what - 10] * 8, hipMemcpyDeviceToHost));
        return VBA_OK;
    }
    if (what == 1) {
        if (capacity < (int64_t)V.N * V.N) return sfail(VBA_EINVAL, "buffer too small");
        std::vector<double> tmp((size_t)V.Npad * V.Npad);
        SCHK(hipMemcpy(tmp.data(), V.S, tmp.size() * 8, hipMemcpyDeviceToHost));
        for (int r = 0; r < V.N; ++r)
            for (int c = 0; c < V.N; ++c) out[(size_t)r * V.N + c] = c <= r ? tmp[(size_t)r * V.Npad + c] : 0.0;
        return VBA_OK;
    }
    if (what == 2) {
        if (!h->robust.sc.arena || !h->robust.have_keys) return sfail(VBA_ESTATE, "no re-weighting since the upload");
        if (capacity < 2 * V.m) return sfail(VBA_EINVAL, "buffer too small");
        SCHK(hipMemcpy(out, h->robust.keys, (size_t)V.m * 16, hipMemcpyDeviceToHost));
        return VBA_OK;
    }
    return sfail(VBA_EINVAL, "unknown selector");
}

}  // extern "C"
