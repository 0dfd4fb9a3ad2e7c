// vba_rel.hip -- observation reliability (vba_reliability): the leverage and the standardised residual (Baarda's w-test) of every
// observation row, and a per-pose summary, at the resident states.
//
// Definitions (include/vinsat_ba.h carries the contract).  Sigma is the inverse of the system vba_covariance inverts -- the same
// shadow front, the same selected inversion, the same damping and symmetrisation rules (vba_query.hip: cov_build_invert).  For row k
// of pose i = ii[k], with J_k [2,6] the reprojection Jacobian over [dp, dtheta] (VBA_DBG_JG), r_k = uv - est, w_k the final robust
// weight (w_raw / w_max) conf (VBA_DBG_WEIGHT) and S_i = Sigma_ii[:6, :6]:
//   P_k      = w_k J_k S_i J_k^T          2x2; only its symmetric part is formed (S_i enters through its upper triangle)
//   leverage = tr(P_k)                    in [0, 2); the redundancy of the row is 2 - leverage
//   wtest    = sqrt(w_k r_k^T (I - P_k)^-1 r_k)       the 2x2 inverse in closed form; (I - P_k) / w_k is the covariance of the
//                                                     row's residual under the linearised model
// w_k == 0: leverage = 0, wtest = 0.  det(I - P_k) <= 0, a negative or non-finite quadratic form: wtest = NaN.  A window the covariance
// step flagged VBA_FLAG_ZERO_PIVOT / VBA_FLAG_NONFINITE has no Sigma: wtest = NaN for every row of it (rows of weight zero included),
// leverage = NaN for its rows of non-zero weight.
//
// Precision: the row pass evaluates J_k in fp64 with the closed forms of vba_math.h (pose_camera, project, project_jacobian: the bits
// of VBA_DBG_JG in fp64 mode) whatever VBA_OPT_JACOBIAN_F32 says -- the query is a diagnostic, not the hot loop.  Sigma comes from
// the system the handle builds in its mode (fp32 Jacobian terms in the accumulation if the option is on), as in vba_covariance.
//
// k_reliability: the row pass of vba_rowpass.h (mapping, prefetch, projector, leverage and w-test, pose butterfly) with two doubles
// per row scattered to the input order of the rows and three numbers per pose.
#include "vba_context.h"
#include "vba_rowpass.h"

namespace vba {

// diag, flags, perm: RowGroup (vba_rowpass.h); lev / wt [W][m_max] in input order; pstat [W][n_max][3]: sum of leverages, largest
// finite wtest, rows of non-zero weight.
__global__ __launch_bounds__(256) void k_reliability(DevView V, const double* __restrict__ diag, const unsigned* __restrict__ flags,
                                                     const int* __restrict__ perm, double* __restrict__ lev, double* __restrict__ wt,
                                                     double* __restrict__ pstat) {
    RowGroup g;
    Row nxt;
    if (!rowpass_begin(V, diag, flags, perm, g, nxt)) return;
    double lsum = 0.0, tmax = 0.0, cnt = 0.0;
    for (int k = g.beg + g.sub; k < g.end; k += kRowLanes) {
        const Row o = row_take(V, g, k, nxt);
        double ru, rv, wk, q00, q01, q11;
        row_projector<false>(g, o, ru, rv, wk, nullptr, nullptr, q00, q01, q11);
        double lv, ts;
        if (wk == 0.0) {
            lv = 0.0;
            ts = g.no_sigma ? __builtin_nan("") : 0.0;
        } else {
            double m00, m11, p01, det;
            row_lev_wtest(wk, q00, q01, q11, ru, rv, g.no_sigma, lv, ts, m00, m11, p01, det);
            cnt += 1.0;
        }
        if ((unsigned)o.p < (unsigned)g.m) {
            lev[g.mb + o.p] = lv;
            wt[g.mb + o.p] = ts;
        }
        lsum += lv;
        if (ts <= 1.79e308) tmax = fmax(tmax, ts);      // (false for NaN: the largest FINITE wtest)
    }
    lsum = group16_sum(lsum); cnt = group16_sum(cnt); tmax = group16_max(tmax);
    if (g.live && g.sub == 0) {
        double* ps = pstat + g.pb * 3;
        ps[0] = lsum;
        ps[1] = tmax;
        ps[2] = cnt;
    }
}

}  // namespace vba

// ---------------------------------------------------------------------------------------------------------- host side

// The scratch of the row pass (rel_layout), kept or grown.  A new allocation holds no permutation: every window's copy is stale.
static int rel_reserve(vba_handle h, RelBufs& b) {
    const size_t W = h->W, N = h->n_max, M = h->m_max;
    if ((int)h->perm_stale.size() != h->W) h->perm_stale.assign(W, 1);
    Carver count;
    rel_layout(count, W, N, M);
    const size_t had = h->q_rel.cap;
    const int rc = query_reserve(h, h->q_rel, count.total(), "reliability scratch failed (two doubles and an index per "
                                                              "observation row of every window)");
    if (h->q_rel.cap != had) std::fill(h->perm_stale.begin(), h->perm_stale.end(), 1);
    if (rc) return rc;
    Carver place{static_cast<char*>(h->q_rel.d)};
    b = rel_layout(place, W, N, M);
    return VBA_OK;
}

// the input position of every sorted row, for the windows whose rows were uploaded since the last query of either row pass
// (one copy over the range of windows that holds them)
static int rel_upload_perm(vba_handle h, int* d_perm) {
    const size_t W = h->W, M = h->m_max;
    size_t lo = W, hi = 0;
    for (size_t w = 0; w < W; ++w)
        if (h->perm_stale[w]) { lo = std::min(lo, w); hi = w + 1; }
    if (lo < hi) {
        std::vector<int> tmp((hi - lo) * M, 0);
        for (size_t w = lo; w < hi; ++w) std::copy(h->perm[w].begin(), h->perm[w].end(), tmp.begin() + (w - lo) * M);
        HIPCHK(hipMemcpy(d_perm + lo * M, tmp.data(), tmp.size() * 4, hipMemcpyHostToDevice));
        std::fill(h->perm_stale.begin(), h->perm_stale.end(), 0);
    }
    return VBA_OK;
}

// The device copy of the permutation, brought up to date: what vba_outlier_power (vba_power.hip) takes from this scratch.
int rel_device_perm(vba_handle h, const int** d_perm) {
    RelBufs b;
    if (int rc = rel_reserve(h, b)) return rc;
    if (int rc = rel_upload_perm(h, b.perm)) return rc;
    *d_perm = b.perm;
    return VBA_OK;
}

// ... and the whole scratch with it: what vba_snoop (vba_snoop.hip) takes -- it stores its w-tests where k_reliability does.
int rel_device_bufs(vba_handle h, RelBufs& b) {
    if (int rc = rel_reserve(h, b)) return rc;
    return rel_upload_perm(h, b.perm);
}

int vba_reliability(vba_handle h, int iter, int damped, double* leverage, double* wtest, double* pose_stats, unsigned* flags) {
    if (int rc = cov_begin(h, iter, "vba_reliability")) return rc;
    RelBufs b;
    if (int rc = rel_reserve(h, b)) return rc;
    const size_t W = h->W, N = h->n_max, M = h->m_max;
    hipStream_t s = h->stream;
    if (int rc = rel_upload_perm(h, b.perm)) return rc;
    CovQuery q;
    if (int rc = cov_build_invert(h, iter, damped, q)) return rc;
    HIPCHK(hipMemsetAsync(b.pstat, 0, W * N * 3 * 8, s));       // (blocks beyond a window's poses do not run)
    hipLaunchKernelGGL(k_reliability, rowpass_grid(h->n_max, h->W), dim3(256), 0, s, q.V, q.diag, q.flags, b.perm, b.lev, b.wt, b.pstat);
    HIPCHK(hipGetLastError());
    if (int rc = query_finish(h, h->q_rel)) return rc;
    if (leverage) if (int rc = query_copy_out(leverage, b.lev, W, M, h->m, 1)) return rc;
    if (wtest) if (int rc = query_copy_out(wtest, b.wt, W, M, h->m, 1)) return rc;
    if (pose_stats) if (int rc = query_copy_out(pose_stats, b.pstat, W, N * 3, h->n, 3)) return rc;
    if (flags) HIPCHK(hipMemcpy(flags, q.flags, W * 4, hipMemcpyDeviceToHost));
    return VBA_OK;
}

int vba_last_reliability_ms(vba_handle h, float* ms) { return query_last_ms(h, &vba_context::q_rel, ms, "no reliability query has run"); }
