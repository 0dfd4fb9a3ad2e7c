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
// k_outlier_power: the row pass, with the mapping of k_reliability (16 lanes -- one DPP row -- per pose, lane `sub` takes rows
// beg + sub, + 16, ...; the next row prefetched; stores scattered to the input order through the device copy of the permutation)
// and its arithmetic for the leverage and the w-test (restated below, operation for operation).  It keeps T = S J^T, which
// k_reliability drops, and writes four doubles per row.  Per pose six numbers go through the four-step butterfly inside the DPP
// row, a lane adding its rows in row order: four are pose_fit, two (rows of non-zero weight, largest finite wtest) only feed the
// window totals.
// k_power_window: one wavefront per window; lane l adds poses l, l + 64, ... in order, then a butterfly in a fixed order.
// No atomics; nothing depends on W or a setting of the handle: a window has the same bits alone and in any batch.
#include "vba_context.h"
#include "vba_power_math.h"

namespace vba {

constexpr int kPowLanes = 16;           // lanes per pose: one DPP row (the mapping of k_reliability)

// The projector, the leverage and the w-test restate k_reliability (vba_rel.hip), which stays as it is.  vba_outlier_power
// promises that kernel's bits for the pose sums of the leverage and for the largest w-test, and under the build's
// -ffp-contract=fast the compiler chooses per kernel which products it folds into an fma.  So the operations k_reliability
// compiles to are written out here one by one -- fma where its ISA has one, a product or sum rounded on its own elsewhere
// (contraction off) -- and tests/test_gpu_outlier_power.py holds the two kernels to equal bits.
// T = S J^T (6x2, columns t0 / t1; S the packed upper triangle of S_i) and J T (2x2, its symmetric part; P = w J T)
__device__ __forceinline__ void pow_projector(const double* S /*[21]*/, const double* J /*[12]*/, double* t0 /*[6]*/,
                                              double* t1 /*[6]*/, double& p00, double& p01, double& p11) {
    p00 = 0.0; p01 = 0.0; p11 = 0.0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        t0[a] = 0.0; t1[a] = 0.0;
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            const double s = S[sym6(a, b)];
            t0[a] = fma(s, J[b], t0[a]);
            t1[a] = fma(s, J[6 + b], t1[a]);
        }
        p00 = fma(J[a], t0[a], p00);
        p01 = fma(J[a], t1[a], p01);
        p11 = fma(J[6 + a], t1[a], p11);
    }
}

// A row of non-zero weight, from q = J T: leverage, w-test, and I - P = [m00, -p01; -p01, m11] with its determinant
__device__ __forceinline__ void pow_lev_wtest(double wk, double q00, double q01, double q11, double ru, double rv, bool no_sigma,
                                              double& lv, double& ts, double& m00, double& m11, double& p01, double& det) {
#pragma clang fp contract(off)
    lv = fma(wk, q00, wk * q11);
    m00 = fma(-wk, q00, 1.0);
    m11 = fma(-wk, q11, 1.0);
    p01 = wk * q01;
    det = fma(m00, m11, -(p01 * p01));
    // r^T (I - P)^-1 r with (I - P)^-1 = [m11, p01; p01, m00] / det
    const double ruv = ru * rv;
    const double qf = fma(rv * rv, m00, fma(ruv + ruv, p01, (ru * ru) * m11)) / det;
    const double t2 = wk * qf;
    ts = (!no_sigma && det > 0.0 && t2 >= 0.0 && t2 <= 1.79e308) ? sqrt(t2) : __builtin_nan("");
}

// diag, flags, perm as k_reliability; mdb / epos / eatt / dpos [W][m_max] in input order; pfit [W][n_max][4]: sum w |r|^2, sum of
// leverages, largest finite ext_pos, rows with wtest > crit; paux [W][n_max][2]: rows of non-zero weight, largest finite wtest.
__global__ __launch_bounds__(256) void k_outlier_power(DevView V, const double* __restrict__ diag, const unsigned* __restrict__ flags,
                                                       const int* __restrict__ perm, double ncp, double crit, double* __restrict__ mdb,
                                                       double* __restrict__ epos, double* __restrict__ eatt, double* __restrict__ dpos,
                                                       double* __restrict__ pfit, double* __restrict__ paux) {
    constexpr int G = kPowLanes, PPB = 256 / G;
    const int w = blockIdx.y;
    const int n = V.n[w], m = V.m[w];
    if (blockIdx.x * PPB >= n) return;      // (block uniform)
    const int i = blockIdx.x * PPB + threadIdx.x / G, sub = threadIdx.x % G;
    const bool live = i < n;                // (uniform over the 16 lanes of a group: the exchanges below stay inside one)
    const size_t ob = (size_t)w * V.obs_stride, mb = (size_t)w * V.m_max;
    const size_t pb = (size_t)w * V.n_max + (live ? i : 0);
    const int* ptr = V.pose_ptr + 2 * ob;
    const int beg = live ? ptr[i] : 0, end = live ? min(ptr[i + 1], m) : 0;
    const bool no_sigma = (flags[w] & (VBA_FLAG_ZERO_PIVOT | VBA_FLAG_NONFINITE)) != 0u;
    const double inv_wmax = 1.0 / bits_f64(V.sc[w].wmax_bits[V.par]);
    const int* pw = perm + mb;
    const double nan = __builtin_nan("");

    struct Row { double x, y, z, u, v, c, wr; int p; };
    auto load = [&](int k) {
        Row o;
        o.x = V.ox[ob + k]; o.y = V.oy[ob + k]; o.z = V.oz[ob + k];
        o.u = V.ou[ob + k]; o.v = V.ov[ob + k]; o.c = V.oconf[ob + k];
        o.wr = V.wraw[mb + k];
        o.p = pw[k];
        return o;
    };
    Row nxt{};
    if (beg + sub < end) nxt = load(beg + sub);
    PoseCam pc{};
    double S[21];           // upper triangle of S_i, packed as sym6
#pragma unroll
    for (int q = 0; q < 21; ++q) S[q] = 0.0;
    if (live) {
        pose_camera(V.states + pb * 10, V.intr + pb * 4, pc);
        const double* Sp = diag + pb * 81;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b) S[sym6(a, b)] = Sp[a * 9 + b];
    }
    double osum = 0.0, lsum = 0.0, emax = 0.0, ccnt = 0.0, cnt = 0.0, tmax = 0.0;
    for (int k = beg + sub; k < end; k += G) {
        const Row o = nxt;
        if (k + G < end) nxt = load(k + G);
        double u, v, cam[3], d, J[12];
        project(pc, o.x, o.y, o.z, u, v, cam, d);
        project_jacobian(pc, cam, d, J);
        const double ru = o.u - u, rv = o.v - v;
        const double wk = (o.wr * inv_wmax) * o.c;
        double t0[6], t1[6], p00, p01, p11;
        pow_projector(S, J, t0, t1, p00, p01, p11);
        double lv, ts, o_mdb, o_ep, o_ea, o_dp;
        if (wk == 0.0) {
            lv = 0.0;
            ts = no_sigma ? nan : 0.0;
            o_mdb = no_sigma ? nan : __builtin_inf();
            o_ep = o_ea = o_dp = no_sigma ? nan : 0.0;
        } else {
            double m00, m11, pw01, det;
            pow_lev_wtest(wk, p00, p01, p11, ru, rv, no_sigma, lv, ts, m00, m11, pw01, det);
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
            const bool ok = !no_sigma && det > 0.0 && mu > 0.0;     // (false for NaN)
            const double scale = ncp / wk;
            o_mdb = ok ? sqrt(ncp / (wk * mu)) : nan;
            o_ep = ok ? sqrt(scale * pair_mu_max(mp00, mp01, mp11, m00, rb, m11)) : nan;
            o_ea = ok ? 2.0 * sqrt(scale * pair_mu_max(mt00, mt01, mt11, m00, rb, m11)) : nan;
            o_dp = ok ? sqrt(dp2) : nan;
        }
        if ((unsigned)o.p < (unsigned)m) {
            mdb[mb + o.p] = o_mdb;
            epos[mb + o.p] = o_ep;
            eatt[mb + o.p] = o_ea;
            dpos[mb + o.p] = o_dp;
        }
        osum = fma(wk, ru * ru + rv * rv, osum);
        lsum += lv;
        if (ts <= 1.79e308) tmax = fmax(tmax, ts);          // (false for NaN: the largest FINITE value)
        if (o_ep <= 1.79e308) emax = fmax(emax, o_ep);
        if (ts > crit) ccnt += 1.0;
    }
    // the 16 partial results of the pose: a butterfly inside the DPP row, the same shape for every pose
    osum += shfl_xor_f64_c<1>(osum); osum += shfl_xor_f64_c<2>(osum); osum += shfl_xor_f64_c<4>(osum); osum += shfl_xor_f64_c<8>(osum);
    lsum += shfl_xor_f64_c<1>(lsum); lsum += shfl_xor_f64_c<2>(lsum); lsum += shfl_xor_f64_c<4>(lsum); lsum += shfl_xor_f64_c<8>(lsum);
    cnt += shfl_xor_f64_c<1>(cnt); cnt += shfl_xor_f64_c<2>(cnt); cnt += shfl_xor_f64_c<4>(cnt); cnt += shfl_xor_f64_c<8>(cnt);
    ccnt += shfl_xor_f64_c<1>(ccnt); ccnt += shfl_xor_f64_c<2>(ccnt); ccnt += shfl_xor_f64_c<4>(ccnt); ccnt += shfl_xor_f64_c<8>(ccnt);
    tmax = fmax(tmax, shfl_xor_f64_c<1>(tmax)); tmax = fmax(tmax, shfl_xor_f64_c<2>(tmax));
    tmax = fmax(tmax, shfl_xor_f64_c<4>(tmax)); tmax = fmax(tmax, shfl_xor_f64_c<8>(tmax));
    emax = fmax(emax, shfl_xor_f64_c<1>(emax)); emax = fmax(emax, shfl_xor_f64_c<2>(emax));
    emax = fmax(emax, shfl_xor_f64_c<4>(emax)); emax = fmax(emax, shfl_xor_f64_c<8>(emax));
    if (live && sub == 0) {
        double* pf = pfit + pb * 4;
        pf[0] = osum;
        pf[1] = lsum;
        pf[2] = emax;
        pf[3] = ccnt;
        paux[pb * 2] = cnt;
        paux[pb * 2 + 1] = tmax;
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

// scratch of the query beyond the reliability scratch (whose device copy of the permutation it reads): four row arrays
// [W][m_max], pose_fit [W][n_max][4], the two pose numbers behind the window totals, fit [W][8]
static int pow_scratch(vba_handle h) {
    const size_t W = h->W, N = h->n_max, M = h->m_max;
    const size_t need = 4 * rel_round(W * M * 8) + rel_round(W * N * 4 * 8) + rel_round(W * N * 2 * 8) + rel_round(W * 8 * 8);
    if (h->pow_cap >= need) return VBA_OK;
    if (h->d_pow) (void)hipFree(h->d_pow);
    h->d_pow = nullptr;
    h->pow_cap = 0;
    if (hipMalloc(&h->d_pow, need) != hipSuccess) {
        (void)hipGetLastError();
        return fail(VBA_ENOMEM, "hipMalloc of " + std::to_string(need) + " bytes of outlier power scratch failed (four doubles per "
                                "observation row of every window)");
    }
    h->pow_cap = need;
    return VBA_OK;
}

int vba_outlier_power(vba_handle h, int iter, int damped, double ncp, double crit, double* mdb, double* ext_pos, double* ext_att,
                      double* del_pos, double* pose_fit, double* fit, unsigned* flags) {
    if (!(ncp > 0.0) || !(ncp <= 1.79e308)) return fail(VBA_EINVAL, "ncp must be positive and finite");
    if (!(crit > 0.0)) return fail(VBA_EINVAL, "crit must be positive (+inf counts nothing)");
    if (int rc = cov_begin(h, iter, "vba_outlier_power")) return rc;
    const int* d_perm = nullptr;
    if (int rc = rel_device_perm(h, &d_perm)) return rc;
    if (int rc = pow_scratch(h)) return rc;
    if (!h->pow_ev) HIPCHK(hipEventCreate(&h->pow_ev));
    const size_t W = h->W, N = h->n_max, M = h->m_max;
    char* p = reinterpret_cast<char*>(h->d_pow);
    double* d_row[4];
    for (auto& r : d_row) { r = reinterpret_cast<double*>(p); p += rel_round(W * M * 8); }
    double* d_pfit = reinterpret_cast<double*>(p); p += rel_round(W * N * 4 * 8);
    double* d_paux = reinterpret_cast<double*>(p); p += rel_round(W * N * 2 * 8);
    double* d_fit = reinterpret_cast<double*>(p);
    hipStream_t s = h->stream;
    CovQuery q;
    if (int rc = cov_build_invert(h, iter, damped, q)) return rc;
    hipLaunchKernelGGL(k_outlier_power, dim3((h->n_max + 256 / kPowLanes - 1) / (256 / kPowLanes), h->W), dim3(256), 0, s, q.V, q.diag,
                       q.flags, d_perm, ncp, crit, d_row[0], d_row[1], d_row[2], d_row[3], d_pfit, d_paux);
    hipLaunchKernelGGL(k_power_window, dim3(h->W), dim3(64), 0, s, q.V.n, h->n_max, d_pfit, d_paux, d_fit);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->pow_ev, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipEventElapsedTime(&h->pow_ms, h->cov_ev[0], h->pow_ev));
    h->pow_ran = true;
    double* const out[4] = {mdb, ext_pos, ext_att, del_pos};
    for (int a = 0; a < 4; ++a)
        if (out[a]) if (int rc = rel_copy_out(out[a], d_row[a], W, M, h->m, 1)) return rc;
    if (pose_fit) if (int rc = rel_copy_out(pose_fit, d_pfit, W, N * 4, h->n, 4)) return rc;
    if (fit) HIPCHK(hipMemcpy(fit, d_fit, W * 8 * 8, hipMemcpyDeviceToHost));
    if (flags) HIPCHK(hipMemcpy(flags, q.flags, W * 4, hipMemcpyDeviceToHost));
    return VBA_OK;
}

int vba_last_outlier_power_ms(vba_handle h, float* ms) {
    if (!h || !ms) return fail(VBA_EINVAL, "null argument");
    if (!h->pow_ran) return fail(VBA_ESTATE, "no outlier power query has run");
    *ms = h->pow_ms;
    return VBA_OK;
}
