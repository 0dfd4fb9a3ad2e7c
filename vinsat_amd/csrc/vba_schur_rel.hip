// vba_schur_rel.hip -- the reliability query of the free-landmark mode (vba_schur_reliability, vba_schur_reliability_dyn on a handle
// with the dynamics factor, vba_schur_reliability_att on one with the attitude factor too; include/vinsat_ba.h carries the contracts):
// the device part of the covariance query (vba_schur_cov.hip), then leverage and w-test of every row and of every catalogue prior, the
// statistics per landmark and per pose, the totals of the fit; with the dynamics factor the leverage of every dynamics edge and the
// edges' share of the fit (vba_schur_dyn_rel.h); with the attitude factor leverage and w-test of every attitude edge and their share
// (vba_schur_att_rel.h).  One body (schur_rel_call) and one device part (schur_rel_device) serve the three kinds of handle; the device
// part is what the snoop and the outlier power queries start with (the row pass of the latter, vba_schur_power.hip, takes the place of
// k_rel_rows there).  vba_schur.hip carries the map of the units; the closed forms of the rows are vba_schur_rel_math.h, the gather of
// a row is vba_schur_rowpass.h.
#include "vba_schur_context.h"
#include "vba_schur_att_rel.h"
#include "vba_schur_dyn_rel.h"
#include "vba_schur_rel_math.h"
#include "vba_schur_rowpass.h"

namespace {

// ------------------------------------------------------------------------------------------------ reliability query
// vba_schur_reliability, after the device part of the covariance query (gathered blocks, Y, Cinv, landmark marginals resident).
//
// Row pass, THREAD PER ROW k (pose i, landmark l, position a in the track of l):
//   Sigma_il = -sum_{k' in rows(l)} (S^-1)_{i, pose(k')} Y_k'   (6x3, k' upwards; the block of the pair from lp_blk, which lists
//                                                               k >= k' only: for k' > k the block of (k', k) is read transposed)
//   P_k = w [A Al] [[Sigma_ii, Sigma_il], [Sigma_il^T, Sigma_ll]] [A Al]^T   (symmetric part), leverage = tr P_k, w-test by
//   rel_wtest2.  A row costs t products of 6x6 by 6x3 for a track of t rows, so the rows of a landmark together cost the t^2 of
//   k_lm_cov -- spread over t threads that sit side by side in a wave and read the same Y and the same blocks.  The gather and
//   P_k are schur_row_blocks (vba_schur_rowpass.h).
// om[k] = w |r|^2 is kept for the totals.
__global__ __launch_bounds__(256) void k_rel_rows(SchurView V, const double* pair, const int* lp_ptr, const int* lp_blk, const double* lm,
                                                  double* lev, double* wt, double* om) {
    const int64_t k64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k64 >= V.m) return;
    const int k = (int)k64;
    const double w = V.row_w[k];
    RowGeom q;
    row_geometry(V, V.states, V.X, k, q);
    om[k] = w * (q.ru * q.ru + q.rv * q.rv);
    if (w == 0.0) { lev[k] = 0.0; wt[k] = 0.0; return; }
    SchurRowBlocks b;
    schur_row_blocks(V, pair, lp_ptr, lp_blk, lm, k, q, w, b);
    lev[k] = b.p00 + b.p11;
    wt[k] = rel_wtest2(b.p00, b.p01, b.p11, q.ru, q.rv, w);
}

// sum of leverage, largest finite w-test, count of rows with w > 0 over a list of rows in list order (idx == nullptr: beg .. end)
__device__ __forceinline__ void rel_row_stats(const SchurView& V, const int* idx, int beg, int end, const double* lev, const double* wt, double* out) {
    double s = 0.0, mx = 0.0, cnt = 0.0;
    for (int r = beg; r < end; ++r) {
        const int k = idx ? idx[r] : r;
        s += lev[k];
        const double t = wt[k];
        if (t <= 1.79e308 && t > mx) mx = t;    // (NaN fails both)
        cnt += V.row_w[k] > 0.0 ? 1.0 : 0.0;
    }
    out[0] = s; out[1] = mx; out[2] = cnt;
}

// Thread id < L: the statistics of landmark id over its rows and the test of its catalogue prior as an observation,
// e = X - X0, P_l = Sigma_ll / sigma^2; lmom = |e|^2 / sigma^2 is kept for the totals.  Thread id < n: the statistics of pose id.
__global__ __launch_bounds__(256) void k_rel_stats(SchurView V, const double* lm, const double* lev, const double* wt, double* lmlev, double* lmwt,
                                                   double* lmom, double* lm_stats, double* pose_stats) {
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id < V.L) {
        const int l = id, beg = V.lm_ptr[l], end = V.lm_ptr[l + 1];
        rel_row_stats(V, nullptr, beg, end, lev, wt, lm_stats + (size_t)l * 3);
        const double e[3] = {V.X[3 * l] - V.X0[3 * l], V.X[3 * l + 1] - V.X0[3 * l + 1], V.X[3 * l + 2] - V.X0[3 * l + 2]};
        lmom[l] = V.inv_sigma2 * (e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
        if (beg == end) {           // tested by nothing: the closed form of k_lm_cov's d
            const double d = 1.0 / (V.inv_sigma2 + V.lamda);
            lmlev[l] = (3.0 * d) * V.inv_sigma2;
            lmwt[l] = 0.0;
        } else {
            const double* Sl = lm + (size_t)l * 9;
            const double is2 = V.inv_sigma2;
            const double p[6] = {Sl[0] * is2, Sl[1] * is2, Sl[2] * is2, Sl[4] * is2, Sl[5] * is2, Sl[8] * is2};
            lmlev[l] = (p[0] + p[3]) + p[5];
            const double mI[6] = {1.0 - p[0], -p[1], -p[2], 1.0 - p[3], -p[4], 1.0 - p[5]};
            lmwt[l] = rel_wtest3(mI, e, is2);
        }
    }
    if (id < V.n) rel_row_stats(V, V.pose_rows, V.pose_ptr[id], V.pose_ptr[id + 1], lev, wt, pose_stats + (size_t)id * 3);
}

// Totals, ONE block: thread t sums the rows t, t + 256, ... and the landmarks likewise, then a tree over the 256 partials -- one
// shape for every problem.  fit[8] = Omega, m_eff, t_rows, t_prior, rho, s0sq, largest finite row / landmark w-test.
__global__ __launch_bounds__(256) void k_rel_totals(SchurView V, const double* lev, const double* wt, const double* om, const double* lmlev,
                                                    const double* lmwt, const double* lmom, double* fit) {
    __shared__ double red[7][256];
    const int t = threadIdx.x;
    double a[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};     // om rows, m_eff, t_rows, max row, om prior, t_prior, max landmark
    for (int64_t k = t; k < V.m; k += 256) {
        a[0] += om[k];
        a[1] += V.row_w[k] > 0.0 ? 1.0 : 0.0;
        a[2] += lev[k];
        const double x = wt[k];
        if (x <= 1.79e308 && x > a[3]) a[3] = x;
    }
    for (int l = t; l < V.L; l += 256) {
        a[4] += lmom[l];
        a[5] += lmlev[l];
        const double x = lmwt[l];
        if (x <= 1.79e308 && x > a[6]) a[6] = x;
    }
#pragma unroll
    for (int e = 0; e < 7; ++e) red[e][t] = a[e];
    for (int o = 128; o > 0; o >>= 1) {
        __syncthreads();
        if (t < o) {
#pragma unroll
            for (int e = 0; e < 7; ++e) {
                const double x = red[e][t], y = red[e][t + o];
                red[e][t] = (e == 3 || e == 6) ? (y > x ? y : x) : x + y;
            }
        }
    }
    if (t == 0) {
        const double Omega = red[0][0] + red[4][0], meff = red[1][0], trows = red[2][0], tprior = red[5][0];
        const double rho = ((2.0 * meff + 3.0 * (double)V.L) - trows) - tprior;
        fit[0] = Omega; fit[1] = meff; fit[2] = trows; fit[3] = tprior; fit[4] = rho;
        fit[5] = rho > 0.0 ? Omega / rho : __builtin_nan("");
        fit[6] = red[3][0]; fit[7] = red[6][0];
    }
}

// ------------------------------------------------------------------------------------------------ with the dynamics factor
// vba_schur_reliability_dyn, after the device part of vba_schur_covariance_dyn (state and edge blocks, D Phi of the query's own
// build resident) and the row and statistics passes above, which run unchanged.
//
// Edge leverage, EIGHT LANES PER EDGE, six at work (the shape of k_sdyn_edges): lane c forms diagonal entry c of J Sigma12 J^T
// (vba_schur_dyn_rel.h: row c of J against the seven columns of Sigma12 it is non-zero at, then against itself; the -D half of J
// is a constant per lane), the six entries meet in lane 0 of the group, which sums them in lane order.  There are n - 1 edges:
// the kernel is a chain of dependent loads and fma, not a bandwidth matter.
constexpr int kEdgeLanes = 8;

__global__ __launch_bounds__(256) void k_rel_edges(int n, double sigma, const double* A, const double* state, const double* edge, double* elev) {
    const int gid = blockIdx.x * 256 + threadIdx.x;
    const int e = gid / kEdgeLanes, c = gid % kEdgeLanes;
    double d = 0.0;
    if (e < n - 1 && c < 6)
        d = schur_dyn_rel_edge_diag(A + (size_t)e * 36, state + (size_t)e * 81, edge + (size_t)e * 81, state + (size_t)(e + 1) * 81, c);
    double diag[6];             // (every lane of the wave takes part in the exchange; the lanes past the edges carry zeros)
#pragma unroll
    for (int k = 0; k < 6; ++k) diag[k] = __shfl(d, k, kEdgeLanes);
    if (e < n - 1 && c == 0) elev[e] = schur_dyn_rel_edge_leverage(sigma, diag);
}

// Behind k_rel_totals, ONE block: the edges' leverages and cost shares summed as k_rel_totals sums the rows (thread t takes the
// edges t, t + 256, ..., then the tree), folded into the fit k_rel_totals left: Omega and the redundancy gain the edges, s0sq
// follows, fit[8] = t_edges, fit[9] = Omega_edges.
__global__ __launch_bounds__(256) void k_rel_edge_totals(int n, int L, const double* elev, const double* eom, double* fit) {
    __shared__ double red[2][256];
    const int t = threadIdx.x;
    double a0 = 0.0, a1 = 0.0;
    for (int e = t; e < n - 1; e += 256) { a0 += elev[e]; a1 += eom[e]; }
    red[0][t] = a0; red[1][t] = a1;
    for (int o = 128; o > 0; o >>= 1) {
        __syncthreads();
        if (t < o) { red[0][t] += red[0][t + o]; red[1][t] += red[1][t + o]; }
    }
    if (t == 0) {
        const double tedges = red[0][0], omedges = red[1][0];
        const double Omega = fit[0] + omedges, meff = fit[1], trows = fit[2], tprior = fit[3];
        const double rho = ((((2.0 * meff + 3.0 * (double)L) + 6.0 * (double)(n - 1)) - trows) - tprior) - tedges;
        fit[0] = Omega; fit[4] = rho;
        fit[5] = rho > 0.0 ? Omega / rho : __builtin_nan("");
        fit[8] = tedges; fit[9] = omedges;
    }
}

// ------------------------------------------------------------------------------------------------ with the attitude factor
// vba_schur_reliability_att, after the device part of vba_schur_reliability_dyn on a handle with both factors (state and edge blocks
// of the Sigma that includes the attitude factor, a and J of the query's own build resident).
//
// Attitude edge, THREAD PER EDGE (vba_schur_att_rel.h): Sigma6 out of the attitude components of the three 9x9 blocks, P_a, its
// trace, the w-test.  Not the lane group of k_rel_edges: an edge is 36 + 18 + 3 independent loads and 162 fma, which one lane holds
// in registers without scratch (DESIGN 9.10 has the compiler's figures), and the w-test needs all of P_a in one lane -- a group of
// three lanes would exchange nine entries by __shfl to save a chain of fma a fraction of a microsecond long.  There are n - 1 edges:
// the kernel is a chain of dependent loads and fma, not a bandwidth matter.
__global__ __launch_bounds__(256) void k_rel_att_edges(int n, double sigma, const double* J, const double* a, const double* state, const double* edge,
                                                       double* alev, double* awt) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n - 1) return;
    double P[9];
    schur_att_rel_P(J + (size_t)e * 18, state + (size_t)e * 81, edge + (size_t)e * 81, state + (size_t)(e + 1) * 81, sigma, P);
    const double av[3] = {a[(size_t)e * 3], a[(size_t)e * 3 + 1], a[(size_t)e * 3 + 2]};
    alev[e] = schur_att_rel_leverage(P);
    awt[e] = schur_att_rel_wtest(P, av, sigma);
}

// Behind k_rel_edge_totals, ONE block with its strided sum and tree (thread t takes the edges t, t + 256, ...): the attitude edges'
// leverages, cost shares and largest finite w-test, folded into the fit k_rel_edge_totals left: Omega and the redundancy gain the
// attitude edges, s0sq follows, fit[10] = t_att, fit[11] = Omega_att, fit[12] = largest finite att_wtest.
__global__ __launch_bounds__(256) void k_rel_att_totals(int n, int L, const double* alev, const double* aom, const double* awt, double* fit) {
    __shared__ double red[3][256];
    const int t = threadIdx.x;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int e = t; e < n - 1; e += 256) {
        a0 += alev[e];
        a1 += aom[e];
        const double x = awt[e];
        if (x <= 1.79e308 && x > a2) a2 = x;    // (NaN fails both)
    }
    red[0][t] = a0; red[1][t] = a1; red[2][t] = a2;
    for (int o = 128; o > 0; o >>= 1) {
        __syncthreads();
        if (t < o) {
            red[0][t] += red[0][t + o];
            red[1][t] += red[1][t + o];
            const double x = red[2][t], y = red[2][t + o];
            red[2][t] = y > x ? y : x;
        }
    }
    if (t == 0) {
        const double tatt = red[0][0], omatt = red[1][0];
        const double Omega = fit[0] + omatt, meff = fit[1], trows = fit[2], tprior = fit[3], tedges = fit[8];
        const double rho = ((((((2.0 * meff + 3.0 * (double)L) + 6.0 * (double)(n - 1)) + 3.0 * (double)(n - 1)) - trows) - tprior) - tedges) - tatt;
        fit[0] = Omega; fit[4] = rho;
        fit[5] = rho > 0.0 ? Omega / rho : __builtin_nan("");
        fit[10] = tatt; fit[11] = omatt; fit[12] = red[2][0];
    }
}

}  // namespace

// first reliability query of a handle: its scratch and its two timing events
int schur_rel_alloc(vba_schur_handle h) {
    SchurRel& R = h->rel;
    if (R.sc.arena) return VBA_OK;
    const SchurView& V = h->V;
    const size_t m = (size_t)V.m, L = (size_t)V.L;
    SchurLayout lay;
    const size_t o_lev = lay.need(m * 8), o_wt = lay.need(m * 8), o_om = lay.need(m * 8), o_ll = lay.need(L * 8), o_lw = lay.need(L * 8),
                 o_lo = lay.need(L * 8), o_ls = lay.need(L * 24), o_ps = lay.need((size_t)V.n * 24), o_fit = lay.need(13 * 8),
                 o_el = lay.need(h->dyn.enabled ? ((size_t)V.n - 1) * 8 : 0), o_al = lay.need(h->att.enabled ? ((size_t)V.n - 1) * 8 : 0),
                 o_aw = lay.need(h->att.enabled ? ((size_t)V.n - 1) * 8 : 0);
    if (int rc = schur_scratch_alloc(R.sc, lay.bytes, "reliability scratch")) return rc;
    char* A = R.sc.arena;
    R.lev = (double*)(A + o_lev); R.wt = (double*)(A + o_wt); R.om = (double*)(A + o_om); R.lmlev = (double*)(A + o_ll); R.lmwt = (double*)(A + o_lw);
    R.lmom = (double*)(A + o_lo); R.lm_stats = (double*)(A + o_ls); R.pose_stats = (double*)(A + o_ps); R.fit = (double*)(A + o_fit);
    if (h->dyn.enabled) R.elev = (double*)(A + o_el);
    if (h->att.enabled) { R.alev = (double*)(A + o_al); R.awt = (double*)(A + o_aw); }
    return VBA_OK;
}

// The device part of the reliability query of a handle of this kind, shared with the snoop and the outlier power queries:
// schur_query_device with the landmark marginals from ev_begin on, and unless the factorisation failed (*bad != 0: nothing more is
// launched) the passes into the reliability scratch -- rows, statistics, totals; with the dynamics factor the edge pass in front of
// the totals and the edges folded into them behind (their cost shares are the ecost of the query's own build); with the attitude
// factor then the attitude edge pass and those edges folded in (on such a handle the covariance query's build fills att.q_a, att.q_J,
// att.q_ecost).  The launches and their order are those the three queries have always issued.  pow_ncp > 0
// (vba_schur_outlier_power): the row pass is k_pow_rows, which leaves lev, wt, om as k_rel_rows does and that query's row figures.
int schur_rel_device(vba_schur_handle h, SchurKind kind, double lamda, hipEvent_t ev_begin, SchurView& V, int* bad, double pow_ncp) {
    SchurQuery& Q = h->q;
    SchurRel& R = h->rel;
    hipStream_t s = h->stream;
    if (int rc = schur_query_device(h, lamda, true, ev_begin, V, bad)) return rc;
    if (*bad != 0) return VBA_OK;
    // every output is formed whatever is asked for: what is asked for decides the copies only
    if (pow_ncp > 0.0) schur_pow_rows_launch(h, V, pow_ncp);
    else hipLaunchKernelGGL(k_rel_rows, dim3((unsigned)(((size_t)V.m + 255) / 256)), dim3(256), 0, s, V, Q.pair, Q.lp_ptr, Q.lp_blk, Q.lm, R.lev, R.wt, R.om);
    hipLaunchKernelGGL(k_rel_stats, dim3((std::max(V.L, V.n) + 255) / 256), dim3(256), 0, s, V, Q.lm, R.lev, R.wt, R.lmlev, R.lmwt, R.lmom, R.lm_stats,
                       R.pose_stats);
    if (kind >= kSchurDyn)
        hipLaunchKernelGGL(k_rel_edges, dim3(((V.n - 1) * kEdgeLanes + 255) / 256), dim3(256), 0, s, V.n, h->dyn.sigma, Q.dyn_A, Q.state, Q.edge, R.elev);
    hipLaunchKernelGGL(k_rel_totals, dim3(1), dim3(256), 0, s, V, R.lev, R.wt, R.om, R.lmlev, R.lmwt, R.lmom, R.fit);
    if (kind >= kSchurDyn) hipLaunchKernelGGL(k_rel_edge_totals, dim3(1), dim3(256), 0, s, V.n, V.L, R.elev, Q.dyn_ecost, R.fit);
    if (kind == kSchurAtt) {
        hipLaunchKernelGGL(k_rel_att_edges, dim3((V.n - 1 + 255) / 256), dim3(256), 0, s, V.n, h->att.sigma, h->att.q_J, h->att.q_a, Q.state, Q.edge,
                           R.alev, R.awt);
        hipLaunchKernelGGL(k_rel_att_totals, dim3(1), dim3(256), 0, s, V.n, V.L, R.alev, h->att.q_ecost, R.awt, R.fit);
    }
    return VBA_OK;
}

// The body of the three entries behind their null check (and the kind check of the plain one): the six outputs of every kind, the
// edges' two with the dynamics factor, the attitude edges' three with the attitude factor, the fit of 8, 10 or 13 slots.
static int schur_rel_call(vba_schur_handle h, SchurKind kind, double lamda, double* leverage, double* wtest, double* lm_leverage, double* lm_wtest,
                          double* lm_stats, double* pose_stats, double* edge_leverage, double* edge_omega, double* att_leverage, double* att_wtest,
                          double* att_omega, double* fit, int* info) {
    if (!(lamda >= 0.0)) return sfail(VBA_EINVAL, "lamda must be >= 0");
    if (int rc = schur_query_begin(h, kind, kind == kSchurPlain ? "vba_schur_reliability" : "vba_schur_reliability_dyn")) return rc;
    if (int rc = schur_rel_alloc(h)) return rc;
    SchurRel& R = h->rel;
    SchurView V;
    int bad = 0;
    if (int rc = schur_rel_device(h, kind, lamda, R.sc.ev[0], V, &bad)) return rc;
    *info = bad;
    const size_t m = (size_t)V.m, L = (size_t)V.L, n = (size_t)V.n;
    Out outs[12] = {{leverage, R.lev, m}, {wtest, R.wt, m}, {lm_leverage, R.lmlev, L}, {lm_wtest, R.lmwt, L}, {lm_stats, R.lm_stats, 3 * L},
                    {pose_stats, R.pose_stats, 3 * n}};
    size_t count = 6;
    if (kind >= kSchurDyn) { outs[count++] = {edge_leverage, R.elev, n - 1}; outs[count++] = {edge_omega, h->q.dyn_ecost, n - 1}; }
    if (kind == kSchurAtt) {
        outs[count++] = {att_leverage, R.alev, n - 1}; outs[count++] = {att_wtest, R.awt, n - 1}; outs[count++] = {att_omega, h->att.q_ecost, n - 1};
    }
    outs[count++] = {fit, R.fit, kind == kSchurAtt ? (size_t)13 : kind == kSchurDyn ? (size_t)10 : (size_t)8};
    return schur_outputs_finish(R.sc, h->stream, bad, outs, count);
}

extern "C" {

int vba_schur_reliability_att(vba_schur_handle h, double lamda, double* leverage, double* wtest, double* lm_leverage, double* lm_wtest,
                              double* lm_stats, double* pose_stats, double* edge_leverage, double* edge_omega, double* att_leverage,
                              double* att_wtest, double* att_omega, double* fit, int* info) {
    if (!h || !info) return sfail(VBA_EINVAL, "null argument");
    return schur_rel_call(h, kSchurAtt, lamda, leverage, wtest, lm_leverage, lm_wtest, lm_stats, pose_stats, edge_leverage, edge_omega, att_leverage,
                          att_wtest, att_omega, fit, info);
}

int vba_schur_last_reliability_att_ms(vba_schur_handle h, float* ms) { return schur_last_ms(h, &vba_schur_context::rel, ms); }

int vba_schur_reliability_dyn(vba_schur_handle h, double lamda, double* leverage, double* wtest, double* lm_leverage, double* lm_wtest,
                              double* lm_stats, double* pose_stats, double* edge_leverage, double* edge_omega, double* fit, int* info) {
    if (!h || !info) return sfail(VBA_EINVAL, "null argument");
    return schur_rel_call(h, kSchurDyn, lamda, leverage, wtest, lm_leverage, lm_wtest, lm_stats, pose_stats, edge_leverage, edge_omega, nullptr, nullptr,
                          nullptr, fit, info);
}

int vba_schur_last_reliability_dyn_ms(vba_schur_handle h, float* ms) { return schur_last_ms(h, &vba_schur_context::rel, ms); }

int vba_schur_reliability(vba_schur_handle h, double lamda, double* leverage, double* wtest, double* lm_leverage, double* lm_wtest,
                          double* lm_stats, double* pose_stats, double* fit, int* info) {
    if (!h || !info) return sfail(VBA_EINVAL, "null argument");
    if (int rc = schur_kind_check(kSchurPlain, h, "vba_schur_reliability")) return rc;
    return schur_rel_call(h, kSchurPlain, lamda, leverage, wtest, lm_leverage, lm_wtest, lm_stats, pose_stats, nullptr, nullptr, nullptr, nullptr, nullptr,
                          fit, info);
}

int vba_schur_last_reliability_ms(vba_schur_handle h, float* ms) { return schur_last_ms(h, &vba_schur_context::rel, ms); }

}  // extern "C"
