// vba_rel.hip -- observation reliability (vba_reliability): the leverage and the standardised residual (Baarda's w-test) of every
// observation row, and a per-pose summary, at the resident states.
//
// Definitions (include/vinsat_ba.h carries the contract).  Sigma is the inverse of the system vba_covariance inverts -- the same
// shadow front, the same selected inversion, the same damping and symmetrisation rules (vba_cov.hip: cov_build_invert).  For row k
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
// k_reliability: one pass over the pose-sorted SoA observation block of every window.  The row-to-lane mapping is the accumulation's
// (k_obs_accumulate<16>): 16 lanes -- one DPP row -- per pose, 16 poses per block of 256, lane `sub` takes rows beg + sub, + 16, ... of
// the pose's CSR segment, so a group reads 128 contiguous bytes of each stream per step.  S_i (21 unique doubles) is loaded once per
// lane into registers: the 16 lanes of a group read the same addresses (one request, broadcast) and keep the block for all their
// rows.  Reads per row: six observation doubles, wraw, the 4-byte input position; writes: two doubles scattered to the input order
// of the rows.  The pose summary is a fixed-order reduction: a lane sums its rows in row order, the 16 partial results meet in a
// butterfly of four DPP exchanges whose shape does not depend on anything -- no atomics, equal settings give equal bits (and no
// setting of the handle changes the mapping: a window has the same bits alone and in any batch).
#include "vba_context.h"

namespace vba {

constexpr int kRelLanes = 16;           // lanes per pose: one DPP row

// diag [W][n_max][81] Sigma_ii, flags [W] of the covariance step; perm [W][m_max] sorted position -> input row;
// lev / wt [W][m_max] in input order; pstat [W][n_max][3]: sum of leverages, largest finite wtest, rows of non-zero weight.
__global__ __launch_bounds__(256) void k_reliability(DevView V, const double* __restrict__ diag, const unsigned* __restrict__ flags,
                                                     const int* __restrict__ perm, double* __restrict__ lev, double* __restrict__ wt,
                                                     double* __restrict__ pstat) {
    constexpr int G = kRelLanes, PPB = 256 / G;
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

    struct Row { double x, y, z, u, v, c, wr; int p; };
    auto load = [&](int k) {
        Row o;
        o.x = V.ox[ob + k]; o.y = V.oy[ob + k]; o.z = V.oz[ob + k];
        o.u = V.ou[ob + k]; o.v = V.ov[ob + k]; o.c = V.oconf[ob + k];
        o.wr = V.wraw[mb + k];
        o.p = pw[k];
        return o;
    };
    // the first row is requested before the pose's camera and covariance block: independent round trips side by side
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
    double lsum = 0.0, tmax = 0.0, cnt = 0.0;
    for (int k = beg + sub; k < end; k += G) {
        const Row o = nxt;
        if (k + G < end) nxt = load(k + G);
        double u, v, cam[3], d, J[12];
        project(pc, o.x, o.y, o.z, u, v, cam, d);
        project_jacobian(pc, cam, d, J);
        const double ru = o.u - u, rv = o.v - v;
        const double wk = (o.wr * inv_wmax) * o.c;
        // T = S J^T (6x2), P = w J T
        double p00 = 0.0, p01 = 0.0, p11 = 0.0;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            double t0 = 0.0, t1 = 0.0;
#pragma unroll
            for (int b = 0; b < 6; ++b) {
                const double s = S[sym6(a, b)];
                t0 = fma(s, J[b], t0);
                t1 = fma(s, J[6 + b], t1);
            }
            p00 = fma(J[a], t0, p00);
            p01 = fma(J[a], t1, p01);
            p11 = fma(J[6 + a], t1, p11);
        }
        p00 *= wk; p01 *= wk; p11 *= wk;
        double lv, ts;
        if (wk == 0.0) {
            lv = 0.0;
            ts = no_sigma ? __builtin_nan("") : 0.0;
        } else {
            lv = p00 + p11;
            const double m00 = 1.0 - p00, m11 = 1.0 - p11;
            const double det = m00 * m11 - p01 * p01;
            // r^T (I - P)^-1 r with (I - P)^-1 = [m11, p01; p01, m00] / det
            const double qf = (ru * ru * m11 + 2.0 * (ru * rv) * p01 + rv * rv * m00) / det;
            const double t2 = wk * qf;
            ts = (!no_sigma && det > 0.0 && t2 >= 0.0 && t2 <= 1.79e308) ? sqrt(t2) : __builtin_nan("");
            cnt += 1.0;
        }
        if ((unsigned)o.p < (unsigned)m) {
            lev[mb + o.p] = lv;
            wt[mb + o.p] = ts;
        }
        lsum += lv;
        if (ts <= 1.79e308) tmax = fmax(tmax, ts);      // (false for NaN: the largest FINITE wtest)
    }
    // the 16 partial results of the pose: a butterfly inside the DPP row, the same shape for every pose
    lsum += shfl_xor_f64_c<1>(lsum); lsum += shfl_xor_f64_c<2>(lsum); lsum += shfl_xor_f64_c<4>(lsum); lsum += shfl_xor_f64_c<8>(lsum);
    cnt += shfl_xor_f64_c<1>(cnt); cnt += shfl_xor_f64_c<2>(cnt); cnt += shfl_xor_f64_c<4>(cnt); cnt += shfl_xor_f64_c<8>(cnt);
    tmax = fmax(tmax, shfl_xor_f64_c<1>(tmax)); tmax = fmax(tmax, shfl_xor_f64_c<2>(tmax));
    tmax = fmax(tmax, shfl_xor_f64_c<4>(tmax)); tmax = fmax(tmax, shfl_xor_f64_c<8>(tmax));
    if (live && sub == 0) {
        double* ps = pstat + pb * 3;
        ps[0] = lsum;
        ps[1] = tmax;
        ps[2] = cnt;
    }
}

}  // namespace vba

// ---------------------------------------------------------------------------------------------------------- host side

// scratch of the row pass: lev, wt [W][m_max] doubles, perm [W][m_max] ints, pstat [W][n_max][3] doubles -- 20 bytes per row and
// window (W = 4096 windows of 50 000 rows: 1.6 GB per row array, 4.1 GB in all)
size_t rel_round(size_t b) { return (b + 255) & ~size_t(255); }

static int rel_scratch(vba_handle h) {
    const size_t W = h->W, N = h->n_max, M = h->m_max;
    const size_t need = 2 * rel_round(W * M * 8) + rel_round(W * M * 4) + rel_round(W * N * 3 * 8);
    if ((int)h->perm_stale.size() != h->W) h->perm_stale.assign(W, 1);
    if (h->rel_cap >= need) return VBA_OK;
    if (h->d_rel) (void)hipFree(h->d_rel);
    h->d_rel = nullptr;
    h->rel_cap = 0;
    std::fill(h->perm_stale.begin(), h->perm_stale.end(), 1);
    if (hipMalloc(&h->d_rel, need) != hipSuccess) {
        (void)hipGetLastError();
        return fail(VBA_ENOMEM, "hipMalloc of " + std::to_string(need) + " bytes of reliability scratch failed (two doubles and an index per "
                                "observation row of every window)");
    }
    h->rel_cap = need;
    return VBA_OK;
}

// per-window results: rows beyond a window's count stay as the caller left them
int rel_copy_out(double* out, const double* dev, size_t W, size_t stride, const std::vector<int>& used, size_t per) {
    bool full = true;
    for (size_t w = 0; w < W; ++w) full = full && (size_t)used[w] * per == stride;
    if (full) {
        HIPCHK(hipMemcpy(out, dev, W * stride * 8, hipMemcpyDeviceToHost));
        return VBA_OK;
    }
    if (W <= 8) {
        for (size_t w = 0; w < W; ++w)
            HIPCHK(hipMemcpy(out + w * stride, dev + w * stride, (size_t)used[w] * per * 8, hipMemcpyDeviceToHost));
        return VBA_OK;
    }
    std::vector<double> tmp;        // many ragged windows: one copy, then the used part of every window
    try {
        tmp.resize(W * stride);
    } catch (const std::bad_alloc&) {
        return fail(VBA_ENOMEM, "host staging for the ragged copy of a reliability output failed");
    }
    HIPCHK(hipMemcpy(tmp.data(), dev, W * stride * 8, hipMemcpyDeviceToHost));
    for (size_t w = 0; w < W; ++w) std::memcpy(out + w * stride, tmp.data() + w * stride, (size_t)used[w] * per * 8);
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
    if (int rc = rel_scratch(h)) return rc;
    int* p = reinterpret_cast<int*>(reinterpret_cast<char*>(h->d_rel) + 2 * rel_round((size_t)h->W * h->m_max * 8));
    if (int rc = rel_upload_perm(h, p)) return rc;
    *d_perm = p;
    return VBA_OK;
}

int vba_reliability(vba_handle h, int iter, int damped, double* leverage, double* wtest, double* pose_stats, unsigned* flags) {
    if (int rc = cov_begin(h, iter, "vba_reliability")) return rc;
    if (int rc = rel_scratch(h)) return rc;
    if (!h->rel_ev) HIPCHK(hipEventCreate(&h->rel_ev));
    const size_t W = h->W, N = h->n_max, M = h->m_max;
    char* p = reinterpret_cast<char*>(h->d_rel);
    double* d_lev = reinterpret_cast<double*>(p); p += rel_round(W * M * 8);
    double* d_wt = reinterpret_cast<double*>(p); p += rel_round(W * M * 8);
    int* d_perm = reinterpret_cast<int*>(p); p += rel_round(W * M * 4);
    double* d_pstat = reinterpret_cast<double*>(p);
    hipStream_t s = h->stream;
    if (int rc = rel_upload_perm(h, d_perm)) return rc;
    CovQuery q;
    if (int rc = cov_build_invert(h, iter, damped, q)) return rc;
    HIPCHK(hipMemsetAsync(d_pstat, 0, W * N * 3 * 8, s));       // (blocks beyond a window's poses do not run)
    hipLaunchKernelGGL(k_reliability, dim3((h->n_max + 256 / kRelLanes - 1) / (256 / kRelLanes), h->W), dim3(256), 0, s, q.V, q.diag,
                       q.flags, d_perm, d_lev, d_wt, d_pstat);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->rel_ev, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipEventElapsedTime(&h->rel_ms, h->cov_ev[0], h->rel_ev));
    h->rel_ran = true;
    if (leverage) if (int rc = rel_copy_out(leverage, d_lev, W, M, h->m, 1)) return rc;
    if (wtest) if (int rc = rel_copy_out(wtest, d_wt, W, M, h->m, 1)) return rc;
    if (pose_stats) if (int rc = rel_copy_out(pose_stats, d_pstat, W, N * 3, h->n, 3)) return rc;
    if (flags) HIPCHK(hipMemcpy(flags, q.flags, W * 4, hipMemcpyDeviceToHost));
    return VBA_OK;
}

int vba_last_reliability_ms(vba_handle h, float* ms) {
    if (!h || !ms) return fail(VBA_EINVAL, "null argument");
    if (!h->rel_ran) return fail(VBA_ESTATE, "no reliability query has run");
    *ms = h->rel_ms;
    return VBA_OK;
}
