// vba_power.hip -- outlier power (vba_outlier_power): per observation row the minimal detectable bias, the external reliability
// in position and attitude and the deletion influence; per pose and per window the weighted residual sum, the redundancy and the
// a-posteriori variance factor of the observation class.  At the resident states, behind the covariance step.
//
// Definitions (include/vinsat_ba.h carries the contract).  J_k, r_k, w_k, S_i and P_k as in vba_rel.hip, for row k of pose i:
//   R_k     = I - P_k                  2x2, its symmetric part; R_k / w_k is the covariance of the row's residual
//   B_k     = w_k S_i J_k^T            6x2: change of the pose's [dp, dtheta] per pixel of error in the row; B_p rows 0..2, B_t rows 3..5
//   mdb     = sqrt(ncp / (w_k mu_min(R_k)))                pixels: the bias the w-test finds with the power ncp stands for, along
//                                                          the direction it sees worst
//   ext_pos = sqrt(ncp / w_k  mu_max(B_p^T B_p, R_k))      km: the largest |dp| a bias at the detection limit causes
//   ext_att = 2 sqrt(ncp / w_k  mu_max(B_t^T B_t, R_k))    rad (the header's 2 |dtheta| convention)
//   del_pos = | B_p R_k^-1 r_k |                           km: how far the position moves if the row is removed
// mu_min, mu_max of a pair and R^-1 r: the closed forms of vba_power_math.h.  w_k == 0: mdb = +inf, the others 0.  det R_k <= 0 or
// mu_min <= 0: NaN in all four.  A window without Sigma (VBA_FLAG_ZERO_PIVOT / VBA_FLAG_NONFINITE): NaN in every row.
//
// k_outlier_power: the row pass of vba_rowpass.h (mapping, prefetch, projector, pose butterfly).  The leverage and the w-test come
// from the function k_reliability calls (row_lev_wtest): the pose sums of the leverage and the largest w-test have that kernel's bits.
// It keeps T = S J^T, which k_reliability drops, and writes four doubles per row.  Per pose six numbers go through the butterfly,
// a lane adding its rows in row order: four are pose_fit, two (rows of non-zero weight, largest finite wtest) only feed the
// window totals.
// k_power_window: one wavefront per window; lane l adds poses l, l + 64, ... in order, then a butterfly in a fixed order.
// No atomics; nothing depends on W or a setting of the handle: a window has the same bits alone and in any batch.
#include "vba_context.h"
#include "vba_power_math.h"
#include "vba_rowpass.h"

namespace vba {

// diag, flags, perm: RowGroup (vba_rowpass.h); mdb / epos / eatt / dpos [W][m_max] in input order; pfit [W][n_max][4]: sum w |r|^2,
// sum of leverages, largest finite ext_pos, rows with wtest > crit; paux [W][n_max][2]: rows of non-zero weight, largest finite wtest.
__global__ __launch_bounds__(256) void k_outlier_power(DevView V, const double* __restrict__ diag, const unsigned* __restrict__ flags,
                                                       const int* __restrict__ perm, double ncp, double crit, double* __restrict__ mdb,
                                                       double* __restrict__ epos, double* __restrict__ eatt, double* __restrict__ dpos,
                                                       double* __restrict__ pfit, double* __restrict__ paux) {
    RowGroup g;
    Row nxt;
    if (!rowpass_begin(V, diag, flags, perm, g, nxt)) return;
    const double nan = __builtin_nan("");
    double osum = 0.0, lsum = 0.0, emax = 0.0, ccnt = 0.0, cnt = 0.0, tmax = 0.0;
    for (int k = g.beg + g.sub; k < g.end; k += kRowLanes) {
        const Row o = row_take(V, g, k, nxt);
        double ru, rv, wk, t0[6], t1[6], p00, p01, p11;
        row_projector<true>(g, o, ru, rv, wk, t0, t1, p00, p01, p11);
        double lv, ts, o_mdb, o_ep, o_ea, o_dp;
        if (wk == 0.0) {
            lv = 0.0;
            ts = g.no_sigma ? nan : 0.0;
            o_mdb = g.no_sigma ? nan : __builtin_inf();
            o_ep = o_ea = o_dp = g.no_sigma ? nan : 0.0;
        } else {
            double m00, m11, pw01, det;
            row_lev_wtest(wk, p00, p01, p11, ru, rv, g.no_sigma, lv, ts, m00, m11, pw01, det);
            cnt += 1.0;
            // R = [m00, -p01; -p01, m11]; B = w T
            const double rb = -pw01;
            const double mu = sym2_mu_min(m00, rb, m11);
            double mp00 = 0.0, mp01 = 0.0, mp11 = 0.0, mt00 = 0.0, mt01 = 0.0, mt11 = 0.0;
            double z0, z1, dp2 = 0.0;
            sym2_solve(m00, rb, m11, ru, rv, z0, z1);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double b0 = wk * t0[a], b1 = wk * t1[a], c0 = wk * t0[3 + a], c1 = wk * t1[3 + a];
                mp00 = fma(b0, b0, mp00); mp01 = fma(b0, b1, mp01); mp11 = fma(b1, b1, mp11);
                mt00 = fma(c0, c0, mt00); mt01 = fma(c0, c1, mt01); mt11 = fma(c1, c1, mt11);
                const double e = fma(b0, z0, b1 * z1);
                dp2 = fma(e, e, dp2);
            }
            const bool ok = !g.no_sigma && det > 0.0 && mu > 0.0;   // (false for NaN)
            const double scale = ncp / wk;
            o_mdb = ok ? sqrt(ncp / (wk * mu)) : nan;
            o_ep = ok ? sqrt(scale * pair_mu_max(mp00, mp01, mp11, m00, rb, m11)) : nan;
            o_ea = ok ? 2.0 * sqrt(scale * pair_mu_max(mt00, mt01, mt11, m00, rb, m11)) : nan;
            o_dp = ok ? sqrt(dp2) : nan;
        }
        if ((unsigned)o.p < (unsigned)g.m) {
            mdb[g.mb + o.p] = o_mdb;
            epos[g.mb + o.p] = o_ep;
            eatt[g.mb + o.p] = o_ea;
            dpos[g.mb + o.p] = o_dp;
        }
        osum = fma(wk, ru * ru + rv * rv, osum);
        lsum += lv;
        if (ts <= 1.79e308) tmax = fmax(tmax, ts);          // (false for NaN: the largest FINITE value)
        if (o_ep <= 1.79e308) emax = fmax(emax, o_ep);
        if (ts > crit) ccnt += 1.0;
    }
    osum = group16_sum(osum); lsum = group16_sum(lsum); cnt = group16_sum(cnt); ccnt = group16_sum(ccnt);
    tmax = group16_max(tmax); emax = group16_max(emax);
    if (g.live && g.sub == 0) {
        double* pf = pfit + g.pb * 4;
        pf[0] = osum;
        pf[1] = lsum;
        pf[2] = emax;
        pf[3] = ccnt;
        paux[g.pb * 2] = cnt;
        paux[g.pb * 2 + 1] = tmax;
    }
}

// fit [W][8]: Omega, m_eff, t, rho = 2 m_eff - t, s0sq = Omega / rho (NaN if rho <= 0), largest finite wtest, rows with
// wtest > crit, largest finite ext_pos.  One wavefront per window.
__global__ __launch_bounds__(64) void k_power_window(const int* __restrict__ n_of, int n_max, const double* __restrict__ pfit,
                                                     const double* __restrict__ paux, double* __restrict__ fit) {
    const int w = blockIdx.x, lane = threadIdx.x;
    const int n = min(n_of[w], n_max);
    const size_t pb = (size_t)w * n_max;
    double osum = 0.0, lsum = 0.0, emax = 0.0, ccnt = 0.0, cnt = 0.0, tmax = 0.0;
    for (int i = lane; i < n; i += kWave) {
        const double* pf = pfit + (pb + i) * 4;
        osum += pf[0];
        lsum += pf[1];
        emax = fmax(emax, pf[2]);
        ccnt += pf[3];
        cnt += paux[(pb + i) * 2];
        tmax = fmax(tmax, paux[(pb + i) * 2 + 1]);
    }
    osum = wave_sum(osum); lsum = wave_sum(lsum); ccnt = wave_sum(ccnt); cnt = wave_sum(cnt);
    emax = wave_max(emax); tmax = wave_max(tmax);
    if (lane == 0) {
        const double rho = 2.0 * cnt - lsum;
        double* f = fit + (size_t)w * 8;
        f[0] = osum;
        f[1] = cnt;
        f[2] = lsum;
        f[3] = rho;
        f[4] = rho > 0.0 ? osum / rho : __builtin_nan("");
        f[5] = tmax;
        f[6] = ccnt;
        f[7] = emax;
    }
}

}  // namespace vba

// ---------------------------------------------------------------------------------------------------------- host side

int vba_outlier_power(vba_handle h, int iter, int damped, double ncp, double crit, double* mdb, double* ext_pos, double* ext_att,
                      double* del_pos, double* pose_fit, double* fit, unsigned* flags) {
    if (!(ncp > 0.0) || !(ncp <= 1.79e308)) return fail(VBA_EINVAL, "ncp must be positive and finite");
    if (!(crit > 0.0)) return fail(VBA_EINVAL, "crit must be positive (+inf counts nothing)");
    if (int rc = cov_begin(h, iter, "vba_outlier_power")) return rc;
    const int* d_perm = nullptr;
    if (int rc = rel_device_perm(h, &d_perm)) return rc;
    const size_t W = h->W, N = h->n_max, M = h->m_max;
    Carver count;
    pow_layout(count, W, N, M);
    if (int rc = query_reserve(h, h->q_pow, count.total(), "outlier power scratch failed (four doubles per "
                                                           "observation row of every window)")) return rc;
    Carver place{static_cast<char*>(h->q_pow.d)};
    const PowBufs b = pow_layout(place, W, N, M);
    hipStream_t s = h->stream;
    CovQuery q;
    if (int rc = cov_build_invert(h, iter, damped, q)) return rc;
    hipLaunchKernelGGL(k_outlier_power, rowpass_grid(h->n_max, h->W), dim3(256), 0, s, q.V, q.diag, q.flags, d_perm, ncp, crit, b.row[0],
                       b.row[1], b.row[2], b.row[3], b.pfit, b.paux);
    hipLaunchKernelGGL(k_power_window, dim3(h->W), dim3(64), 0, s, q.V.n, h->n_max, b.pfit, b.paux, b.fit);
    HIPCHK(hipGetLastError());
    if (int rc = query_finish(h, h->q_pow)) return rc;
    double* const out[4] = {mdb, ext_pos, ext_att, del_pos};
    for (int a = 0; a < 4; ++a)
        if (out[a]) if (int rc = query_copy_out(out[a], b.row[a], W, M, h->m, 1)) return rc;
    if (pose_fit) if (int rc = query_copy_out(pose_fit, b.pfit, W, N * 4, h->n, 4)) return rc;
    if (fit) HIPCHK(hipMemcpy(fit, b.fit, W * 8 * 8, hipMemcpyDeviceToHost));
    if (flags) HIPCHK(hipMemcpy(flags, q.flags, W * 4, hipMemcpyDeviceToHost));
    return VBA_OK;
}

int vba_last_outlier_power_ms(vba_handle h, float* ms) {
    return query_last_ms(h, &vba_context::q_pow, ms, "no outlier power query has run");
}
