// vba_schur_power.hip -- the outlier power query of the free-landmark mode (vba_schur_outlier_power, _dyn, _att;
// include/vinsat_ba.h carries the contract, vba_schur.hip the map of the units): the device part of the reliability query of the
// handle (vba_schur_rel.hip) with k_pow_rows in the place of k_rel_rows, so that the gather of Sigma_il -- the expensive part of a
// row -- is formed once per row in this query, then the figures per landmark and per pose and the totals.  The row's gather and P_k
// are vba_schur_rowpass.h, the closed forms vba_power_math.h and vba_schur_power_math.h.  No float atomics, every sum in one order.
#include "vba_schur_context.h"
#include "vba_schur_power_math.h"
#include "vba_schur_rel_math.h"
#include "vba_schur_rowpass.h"

namespace {

struct PowRowsOut {
    double *lev, *wt, *om;                              // the reliability scratch, as k_rel_rows leaves it
    double *mdb, *epos, *eatt, *elm, *dpos, *dlm, *pull;
};

// Row pass, THREAD PER ROW: the statements of k_rel_rows up to lev and wt (same arithmetic, same order: same bits), then from the
// registers of the gather
//   T = Sigma_k J_k^T (9x2):  rows 0..5 = Sigma_ii A^T + Sigma_il Al^T,  rows 6..8 = Sigma_il^T A^T + Sigma_ll Al^T   (Sigma_il = -G)
//   the six figures by schur_pow_row, and pull = |Sigma_il[0:3,:] z_l| with z_l = (I - P_l)^-1 e_l / sigma^2 formed per row from
//   lm[l] (a 3x3 adjugate: cheaper than a pass per landmark in front of this one).
// A row of weight 0: mdb = +inf, everything else 0.
__global__ __launch_bounds__(256) void k_pow_rows(SchurView V, const double* pair, const int* lp_ptr, const int* lp_blk, const double* lm, double ncp,
                                                  PowRowsOut O) {
    const int64_t k64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k64 >= V.m) return;
    const int k = (int)k64;
    const double w = V.row_w[k];
    RowGeom q;
    row_geometry(V, V.states, V.X, k, q);
    O.om[k] = w * (q.ru * q.ru + q.rv * q.rv);
    if (w == 0.0) {
        O.lev[k] = 0.0; O.wt[k] = 0.0;
        O.mdb[k] = __builtin_inf();
        O.epos[k] = 0.0; O.eatt[k] = 0.0; O.elm[k] = 0.0; O.dpos[k] = 0.0; O.dlm[k] = 0.0; O.pull[k] = 0.0;
        return;
    }
    SchurRowBlocks b;
    schur_row_blocks(V, pair, lp_ptr, lp_blk, lm, k, q, w, b);
    O.lev[k] = b.p00 + b.p11;
    O.wt[k] = rel_wtest2(b.p00, b.p01, b.p11, q.ru, q.rv, w);
    double tu[9], tv[9];
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        double su = 0.0, sv = 0.0, gu = 0.0, gv = 0.0;
#pragma unroll
        for (int qq = 0; qq < 6; ++qq) { su = fma(b.Sii[6 * p + qq], b.jc[qq], su); sv = fma(b.Sii[6 * p + qq], b.jc[6 + qq], sv); }
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) { gu = fma(b.G[3 * p + cc], b.jl[cc], gu); gv = fma(b.G[3 * p + cc], b.jl[3 + cc], gv); }
        tu[p] = su - gu;
        tv[p] = sv - gv;
    }
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) {
        double su = 0.0, sv = 0.0, gu = 0.0, gv = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) { su = fma(b.Sl[3 * cc + r], b.jl[r], su); sv = fma(b.Sl[3 * cc + r], b.jl[3 + r], sv); }
#pragma unroll
        for (int p = 0; p < 6; ++p) { gu = fma(b.G[3 * p + cc], b.jc[p], gu); gv = fma(b.G[3 * p + cc], b.jc[6 + p], gv); }
        tu[6 + cc] = su - gu;
        tv[6 + cc] = sv - gv;
    }
    double out[6];
    schur_pow_row(w, b.p00, b.p01, b.p11, q.ru, q.rv, tu, tv, ncp, out);
    O.mdb[k] = out[0]; O.epos[k] = out[1]; O.eatt[k] = out[2]; O.elm[k] = out[3]; O.dpos[k] = out[4]; O.dlm[k] = out[5];
    const int l = V.row_lm[k];
    const double is2 = V.inv_sigma2;
    const double P[6] = {b.Sl[0] * is2, b.Sl[1] * is2, b.Sl[2] * is2, b.Sl[4] * is2, b.Sl[5] * is2, b.Sl[8] * is2};
    const double e[3] = {V.X[3 * l] - V.X0[3 * l], V.X[3 * l + 1] - V.X0[3 * l + 1], V.X[3 * l + 2] - V.X0[3 * l + 2]};
    O.pull[k] = schur_pow_pull(b.G, P, e, is2);
}

// Thread id < L: the catalogue prior of landmark id as an observation -- detectable error, its effect on the landmark's own
// estimate, and the largest finite pull over its rows of non-zero weight in row order.  Thread id < n: pose_fit of pose id over
// pose_rows in list order; its second slot is the sum rel_row_stats forms, in its order.
__global__ __launch_bounds__(256) void k_pow_stats(SchurView V, const double* lm, const double* lev, const double* wt, const double* om,
                                                   const double* epos, const double* pull, double ncp, double crit, double* lm_mdb, double* lm_ext,
                                                   double* lm_del, double* pose_fit) {
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id < V.L) {
        const int l = id, beg = V.lm_ptr[l], end = V.lm_ptr[l + 1];
        if (beg == end) {           // tested by nothing
            lm_mdb[l] = __builtin_inf();
            lm_ext[l] = 0.0;
            lm_del[l] = 0.0;
        } else {
            const double* Sl = lm + (size_t)l * 9;
            const double is2 = V.inv_sigma2;
            const double P[6] = {Sl[0] * is2, Sl[1] * is2, Sl[2] * is2, Sl[4] * is2, Sl[5] * is2, Sl[8] * is2};
            double a, x;
            schur_pow_prior(P, sqrt(1.0 / is2), ncp, a, x);
            lm_mdb[l] = a;
            lm_ext[l] = x;
            double mx = 0.0;
            for (int k = beg; k < end; ++k) {
                const double t = pull[k];
                if (V.row_w[k] > 0.0 && t <= 1.79e308 && t > mx) mx = t;
            }
            lm_del[l] = schur_pow_prior_det(P) > 0.0 ? mx : __builtin_nan("");
        }
    }
    if (id < V.n) {
        double s_om = 0.0, s_lev = 0.0, mx = 0.0, cnt = 0.0;
        for (int r = V.pose_ptr[id]; r < V.pose_ptr[id + 1]; ++r) {
            const int k = V.pose_rows[r];
            s_om += om[k];
            s_lev += lev[k];
            const double t = epos[k];
            if (t <= 1.79e308 && t > mx) mx = t;    // (NaN fails both)
            cnt += wt[k] > crit ? 1.0 : 0.0;
        }
        double* pf = pose_fit + (size_t)id * 4;
        pf[0] = s_om; pf[1] = s_lev; pf[2] = mx; pf[3] = cnt;
    }
}

// Totals, ONE block with the tree of k_rel_totals: thread t takes the rows t, t + 256, ... and the landmarks likewise.  fit = the
// `lead` slots of the reliability fit as they are, then rows with wtest > crit, largest finite ext_pos, landmarks with
// lm_wtest > crit, largest finite lm_del_pos.
__global__ __launch_bounds__(256) void k_pow_totals(SchurView V, const double* wt, const double* epos, const double* lmwt, const double* lm_del,
                                                    const double* rel_fit, int lead, double crit, double* fit) {
    __shared__ double red[4][256];
    const int t = threadIdx.x;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t k = t; k < V.m; k += 256) {
        a[0] += wt[k] > crit ? 1.0 : 0.0;
        const double x = epos[k];
        if (x <= 1.79e308 && x > a[1]) a[1] = x;
    }
    for (int l = t; l < V.L; l += 256) {
        a[2] += lmwt[l] > crit ? 1.0 : 0.0;
        const double x = lm_del[l];
        if (x <= 1.79e308 && x > a[3]) a[3] = x;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) red[e][t] = a[e];
    for (int o = 128; o > 0; o >>= 1) {
        __syncthreads();
        if (t < o) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double x = red[e][t], y = red[e][t + o];
                red[e][t] = (e & 1) ? (y > x ? y : x) : x + y;
            }
        }
    }
    if (t < lead) fit[t] = rel_fit[t];
    if (t == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) fit[lead + e] = red[e][0];
    }
}

// first power query of a handle: its scratch and its two timing events
int schur_pow_alloc(vba_schur_handle h) {
    SchurPow& P = h->pow;
    if (P.sc.arena) return VBA_OK;
    const size_t m = (size_t)h->V.m, L = (size_t)h->V.L, n = (size_t)h->V.n;
    SchurLayout lay;
    size_t o_row[7], o_lm[3];
    for (size_t& o : o_row) o = lay.need(m * 8);
    for (size_t& o : o_lm) o = lay.need(L * 8);
    const size_t o_pf = lay.need(n * 32), o_fit = lay.need(17 * 8);
    if (int rc = schur_scratch_alloc(P.sc, lay.bytes, "outlier power scratch")) return rc;
    char* A = P.sc.arena;
    double** row[7] = {&P.mdb, &P.epos, &P.eatt, &P.elm, &P.dpos, &P.dlm, &P.pull};
    for (int e = 0; e < 7; ++e) *row[e] = (double*)(A + o_row[e]);
    P.lm_mdb = (double*)(A + o_lm[0]); P.lm_ext = (double*)(A + o_lm[1]); P.lm_del = (double*)(A + o_lm[2]);
    P.pose_fit = (double*)(A + o_pf); P.fit = (double*)(A + o_fit);
    return VBA_OK;
}

// The body of the three entries (kind: the handle has the dynamics factor, or the attitude factor too, and everything comes from
// the device part of vba_schur_reliability_dyn / vba_schur_reliability_att; the three kernels are the same, the fit leads with that
// query's ten / thirteen slots).
int schur_power_call(vba_schur_handle h, SchurKind kind, double lamda, double ncp, double crit, double* mdb, double* ext_pos, double* ext_att,
                     double* ext_lm, double* del_pos, double* del_lm, double* lm_mdb, double* lm_ext, double* lm_del_pos, double* pose_fit,
                     double* fit, int* info) {
    if (!(lamda >= 0.0)) return sfail(VBA_EINVAL, "lamda must be >= 0");
    if (!(ncp > 0.0 && ncp <= 1.79e308)) return sfail(VBA_EINVAL, "ncp must be positive and finite");
    if (!(crit > 0.0)) return sfail(VBA_EINVAL, "crit must be > 0 (+inf counts nothing)");
    if (int rc = schur_query_begin(h, kind, kind == kSchurPlain ? "vba_schur_outlier_power" : "vba_schur_outlier_power_dyn")) return rc;
    if (int rc = schur_rel_alloc(h)) return rc;
    if (int rc = schur_pow_alloc(h)) return rc;
    SchurRel& R = h->rel;
    SchurPow& P = h->pow;
    hipStream_t s = h->stream;
    SchurView V;
    int bad = 0;
    if (int rc = schur_rel_device(h, kind, lamda, P.sc.ev[0], V, &bad, ncp)) return rc;
    *info = bad;
    const size_t m = (size_t)V.m, L = (size_t)V.L, n = (size_t)V.n;
    const int lead = kind == kSchurAtt ? 13 : kind == kSchurDyn ? 10 : 8;
    const Out outs[11] = {{mdb, P.mdb, m}, {ext_pos, P.epos, m}, {ext_att, P.eatt, m}, {ext_lm, P.elm, m}, {del_pos, P.dpos, m}, {del_lm, P.dlm, m},
                          {lm_mdb, P.lm_mdb, L}, {lm_ext, P.lm_ext, L}, {lm_del_pos, P.lm_del, L}, {pose_fit, P.pose_fit, 4 * n},
                          {fit, P.fit, (size_t)lead + 4}};
    if (bad == 0) {                 // (else no factor, no covariance, no figure: NaN, and the row in *info)
        // every output is formed whatever is asked for: what is asked for decides the copies only
        hipLaunchKernelGGL(k_pow_stats, dim3((std::max(V.L, V.n) + 255) / 256), dim3(256), 0, s, V, h->q.lm, R.lev, R.wt, R.om, P.epos, P.pull, ncp, crit,
                           P.lm_mdb, P.lm_ext, P.lm_del, P.pose_fit);
        hipLaunchKernelGGL(k_pow_totals, dim3(1), dim3(256), 0, s, V, R.wt, P.epos, R.lmwt, P.lm_del, R.fit, lead, crit, P.fit);
    }
    return schur_outputs_finish(P.sc, s, bad, outs, 11);
}

}  // namespace

void schur_pow_rows_launch(vba_schur_handle h, const SchurView& V, double ncp) {
    const SchurQuery& Q = h->q;
    const SchurRel& R = h->rel;
    const SchurPow& P = h->pow;
    const PowRowsOut O{R.lev, R.wt, R.om, P.mdb, P.epos, P.eatt, P.elm, P.dpos, P.dlm, P.pull};
    hipLaunchKernelGGL(k_pow_rows, dim3((unsigned)(((size_t)V.m + 255) / 256)), dim3(256), 0, h->stream, V, Q.pair, Q.lp_ptr, Q.lp_blk, Q.lm, ncp, O);
}

extern "C" {

int vba_schur_outlier_power(vba_schur_handle h, double lamda, double ncp, double crit, double* mdb, double* ext_pos, double* ext_att, double* ext_lm,
                            double* del_pos, double* del_lm, double* lm_mdb, double* lm_ext, double* lm_del_pos, double* pose_fit, double* fit,
                            int* info) {
    if (!h || !info) return sfail(VBA_EINVAL, "null argument");
    if (int rc = schur_kind_check(kSchurPlain, h, "vba_schur_outlier_power")) return rc;
    return schur_power_call(h, kSchurPlain, lamda, ncp, crit, mdb, ext_pos, ext_att, ext_lm, del_pos, del_lm, lm_mdb, lm_ext, lm_del_pos, pose_fit, fit, info);
}

int vba_schur_last_outlier_power_ms(vba_schur_handle h, float* ms) { return schur_last_ms(h, &vba_schur_context::pow, ms); }

int vba_schur_outlier_power_dyn(vba_schur_handle h, double lamda, double ncp, double crit, double* mdb, double* ext_pos, double* ext_att,
                                double* ext_lm, double* del_pos, double* del_lm, double* lm_mdb, double* lm_ext, double* lm_del_pos, double* pose_fit,
                                double* fit, int* info) {
    if (!h || !info) return sfail(VBA_EINVAL, "null argument");
    return schur_power_call(h, kSchurDyn, lamda, ncp, crit, mdb, ext_pos, ext_att, ext_lm, del_pos, del_lm, lm_mdb, lm_ext, lm_del_pos, pose_fit, fit, info);
}

int vba_schur_last_outlier_power_dyn_ms(vba_schur_handle h, float* ms) { return schur_last_ms(h, &vba_schur_context::pow, ms); }

int vba_schur_outlier_power_att(vba_schur_handle h, double lamda, double ncp, double crit, double* mdb, double* ext_pos, double* ext_att,
                                double* ext_lm, double* del_pos, double* del_lm, double* lm_mdb, double* lm_ext, double* lm_del_pos, double* pose_fit,
                                double* fit, int* info) {
    if (!h || !info) return sfail(VBA_EINVAL, "null argument");
    return schur_power_call(h, kSchurAtt, lamda, ncp, crit, mdb, ext_pos, ext_att, ext_lm, del_pos, del_lm, lm_mdb, lm_ext, lm_del_pos, pose_fit, fit, info);
}

int vba_schur_last_outlier_power_att_ms(vba_schur_handle h, float* ms) { return schur_last_ms(h, &vba_schur_context::pow, ms); }

}  // extern "C"
