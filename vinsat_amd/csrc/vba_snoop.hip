// vba_snoop.hip -- data snooping (vba_snoop): per pose, the observation row whose w-test exceeds a critical value by most is
// rejected on the device -- its confidence in the observation block becomes 0, its original value and a mask byte are kept.
//
// Definitions (include/vinsat_ba.h carries the contract).  The system, the row quantities and the w-test are those of
// vba_reliability at the resident states (vba_rel.hip): the same shadow front, the same selected inversion, row_projector and
// row_lev_wtest of vba_rowpass.h with the same mapping -- wtest of every row has the bits vba_reliability would return, and is
// stored where k_reliability stores it (the reliability scratch, input order).  For pose i:
//   candidates   its rows with w_k > 0, wtest finite and wtest > crit;
//   cnt_i        its rows of non-zero weight;
//   mode 0       the best candidate (largest wtest; ties: the smaller sorted position, which inside a pose is the smaller input
//                row index -- vba_snoop_pick.h) is rejected if cnt_i - 1 >= min_rows;
//   mode 1       every candidate is rejected if cnt_i - #candidates >= min_rows; else the rule of mode 0.
// A window the covariance step flagged VBA_FLAG_ZERO_PIVOT / NONFINITE / INDEFINITE rejects nothing.
//
// k_snoop: one launch.  First loop: the row pass of k_reliability; each lane keeps its best (wtest, sorted position), its count
// of candidates and of weighted rows.  Then the 16 partial results of a pose meet in a butterfly of four DPP exchanges inside the
// row whose shape depends on nothing; the combine rule is a strict total order, so every lane of the pose ends with the same
// winner.  Second loop: the lanes that own rejected rows (a lane owns rows beg + sub, + 16, ...) save the confidence, write 0.0
// and set the mask byte at the row's input position; a lane reads and writes its own rows only.  No atomics, plain vector
// stores, equal settings give equal bits, a window has the same result alone and in any batch.
//
// vba_snoop_scaled: the same rule with one critical value per window, quantile * s0 of the window's own fit, formed on the device
// behind one covariance step: k_snoop_fit (the row pass, and per pose the sums k_outlier_power forms), k_snoop_crit (one wavefront
// per window: s0sq and the critical value), k_snoop_pick (k_snoop's butterfly, decision and stores over the stored w-tests).
#include "vba_context.h"
#include "vba_rowpass.h"
#include "vba_snoop_pick.h"

namespace vba {

// One step of the pose butterfly: the partner's (wtest, position, candidate count); position and count travel as one 64-bit word
template <int MASK>
__device__ __forceinline__ void snoop_exchange(double& best, int& bpos, int& cand) {
    const double o_val = shfl_xor_f64_c<MASK>(best);
    const unsigned long long mine = ((unsigned long long)(unsigned)cand << 32) | (unsigned)bpos;
    const unsigned long long theirs = (unsigned long long)__double_as_longlong(shfl_xor_f64_c<MASK>(__longlong_as_double((long long)mine)));
    cand += (int)(unsigned)(theirs >> 32);
    pick(best, bpos, o_val, (int)(unsigned)theirs);
}

__device__ __forceinline__ bool snoop_candidate(double wk, double ts, double crit) {
    return wk > 0.0 && ts <= 1.79e308 && ts > crit;         // (false for a NaN in any of them)
}

// The decision of a pose (uniform over its 16 lanes) from what the butterfly left: `left` rows of non-zero weight, `cand` candidates
enum SnoopDecision { kSnoopNone = 0, kSnoopOne, kSnoopAll };
__device__ __forceinline__ SnoopDecision snoop_decide(bool barred, int left, int cand, int mode, int min_rows) {
    if (barred || cand <= 0) return kSnoopNone;
    if (mode == 1 && left - cand >= min_rows) return kSnoopAll;
    return left - 1 >= min_rows ? kSnoopOne : kSnoopNone;
}

// ... and its stores, by the lanes that own the rejected rows: the confidence saved, 0.0 in its place, the mask byte at the row's
// input position, the pose's count
__device__ __forceinline__ void snoop_apply(const DevView& V, const RowGroup& g, SnoopDecision d, int bpos, int cand, double crit,
                                            const double* wt, double* conf, double* __restrict__ orig,
                                            unsigned char* __restrict__ mask, int* __restrict__ prej) {
    if (d == kSnoopAll) {
        for (int k = g.beg + g.sub; k < g.end; k += kRowLanes) {
            const int p = g.pw[k];
            if ((unsigned)p >= (unsigned)g.m) continue;
            const double c = conf[g.ob + k];
            const double wk = (V.wraw[g.mb + k] * g.inv_wmax) * c;
            if (snoop_candidate(wk, wt[g.mb + p], crit)) {
                orig[g.mb + p] = c;
                conf[g.ob + k] = 0.0;
                mask[g.mb + p] = 1;
            }
        }
    } else if (d == kSnoopOne && bpos >= g.beg && bpos < g.end && (bpos - g.beg) % kRowLanes == g.sub) {
        const int p = g.pw[bpos];
        if ((unsigned)p < (unsigned)g.m) {
            orig[g.mb + p] = conf[g.ob + bpos];
            conf[g.ob + bpos] = 0.0;
            mask[g.mb + p] = 1;
        }
    }
    if (g.live && g.sub == 0) prej[g.pb] = d == kSnoopAll ? cand : (d == kSnoopOne ? 1 : 0);
}

__device__ __forceinline__ bool snoop_barred(const unsigned* __restrict__ flags) {
    return (flags[blockIdx.y] & (VBA_FLAG_ZERO_PIVOT | VBA_FLAG_NONFINITE | VBA_FLAG_INDEFINITE)) != 0u;
}

// diag, flags, perm: RowGroup (vba_rowpass.h); wt [W][m_max] in input order (the reliability scratch); conf: the confidences of
// window 0 inside the observation block (DevView::oconf, writable); orig, mask [W][m_max] in input order; prej [W][n_max] rows the
// pose lost in this call.
__global__ __launch_bounds__(256) void k_snoop(DevView V, const double* __restrict__ diag, const unsigned* __restrict__ flags,
                                               const int* __restrict__ perm, double crit, int mode, int min_rows, double* wt,
                                               double* conf, double* __restrict__ orig, unsigned char* __restrict__ mask,
                                               int* __restrict__ prej) {
    RowGroup g;
    Row nxt;
    if (!rowpass_begin(V, diag, flags, perm, g, nxt)) return;
    const bool barred = snoop_barred(flags);
    double best = __builtin_nan(""), cnt = 0.0;
    int bpos = kSnoopNoPos, cand = 0;
    for (int k = g.beg + g.sub; k < g.end; k += kRowLanes) {
        const Row o = row_take(V, g, k, nxt);
        double ru, rv, wk, q00, q01, q11;
        row_projector<false>(g, o, ru, rv, wk, nullptr, nullptr, q00, q01, q11);
        double ts;
        if (wk == 0.0) {
            ts = g.no_sigma ? __builtin_nan("") : 0.0;
        } else {
            double lv, m00, m11, p01, det;
            row_lev_wtest(wk, q00, q01, q11, ru, rv, g.no_sigma, lv, ts, m00, m11, p01, det);
            cnt += 1.0;
        }
        if ((unsigned)o.p < (unsigned)g.m) wt[g.mb + o.p] = ts;
        if (snoop_candidate(wk, ts, crit)) {
            cand += 1;
            pick(best, bpos, ts, k);
        }
    }
    cnt = group16_sum(cnt);
    snoop_exchange<1>(best, bpos, cand); snoop_exchange<2>(best, bpos, cand);
    snoop_exchange<4>(best, bpos, cand); snoop_exchange<8>(best, bpos, cand);
    snoop_apply(V, g, snoop_decide(barred, (int)cnt, cand, mode, min_rows), bpos, cand, crit, wt, conf, orig, mask, prej);
}

// ---- vba_snoop_scaled: the critical value of a window is quantile * s0 of its own fit, formed on the device.  Three launches.
//
// k_snoop_fit: the row pass of k_snoop's first loop without a critical value -- wtest of every row into wt -- and per pose what
// k_outlier_power accumulates for the window's variance factor, with that kernel's bits: pose [W][n_max][3] = Omega_i, the sum of
// the leverages, the rows of non-zero weight.  A lane adds its rows in row order, then group16_sum.
// Omega_i: k_outlier_power writes fma(wk, ru * ru + rv * rv, osum) under -ffp-contract=fast, and the compiler forms the inner sum
// as fma(ru, ru, rv * rv) (its gfx950 assembly: v_mul rv rv; v_fmac ru ru; v_fmac wk . osum).  Here that choice is spelled out
// with contraction off, so the bits are that kernel's whatever a compiler would fold in this one.
__global__ __launch_bounds__(256) void k_snoop_fit(DevView V, const double* __restrict__ diag, const unsigned* __restrict__ flags,
                                                   const int* __restrict__ perm, double* __restrict__ wt, double* __restrict__ pose) {
#pragma clang fp contract(off)
    RowGroup g;
    Row nxt;
    if (!rowpass_begin(V, diag, flags, perm, g, nxt)) return;
    double osum = 0.0, lsum = 0.0, cnt = 0.0;
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
        if ((unsigned)o.p < (unsigned)g.m) wt[g.mb + o.p] = ts;
        osum = fma(wk, fma(ru, ru, rv * rv), osum);
        lsum += lv;
    }
    osum = group16_sum(osum); lsum = group16_sum(lsum); cnt = group16_sum(cnt);
    if (g.live && g.sub == 0) {
        double* pf = pose + g.pb * 3;
        pf[0] = osum;
        pf[1] = lsum;
        pf[2] = cnt;
    }
}

// k_snoop_crit: one wavefront per window; lane l adds poses l, l + 64, ... in order, then wave_sum -- the order of k_power_window,
// so rho and s0sq have the bits of its fit[3] and fit[4].  win [W][2] = s0sq, crit_used = quantile * sqrt(s0sq) as the IEEE
// product of the correctly rounded root (NaN unless s0sq > 0).
__global__ __launch_bounds__(64) void k_snoop_crit(const int* __restrict__ n_of, int n_max, const double* __restrict__ pose,
                                                   double quantile, double* __restrict__ win) {
    const int w = blockIdx.x, lane = threadIdx.x;
    const int n = min(n_of[w], n_max);
    const size_t pb = (size_t)w * n_max;
    double osum = 0.0, lsum = 0.0, cnt = 0.0;
    for (int i = lane; i < n; i += kWave) {
        const double* pf = pose + (pb + i) * 3;
        osum += pf[0];
        lsum += pf[1];
        cnt += pf[2];
    }
    osum = wave_sum(osum); lsum = wave_sum(lsum); cnt = wave_sum(cnt);
    if (lane == 0) {
        const double rho = 2.0 * cnt - lsum;            // (2 cnt is exact: an fma gives the same bits)
        const double s0sq = rho > 0.0 ? osum / rho : __builtin_nan("");
        win[2 * w] = s0sq;
        win[2 * w + 1] = s0sq > 0.0 ? __dmul_rn(quantile, __dsqrt_rn(s0sq)) : __builtin_nan("");
    }
}

// k_snoop_pick: k_snoop behind the stored results -- no projector, no S_i.  A lane walks the rows it owns in row order, reads the
// wtest k_snoop_fit stored, the confidence and the raw weight, tests against the window's own critical value (win, read from
// device memory), and the pose butterfly, the decision and the stores are k_snoop's.  cnt_i is k_snoop_fit's (pose[..][2]).
__global__ __launch_bounds__(256) void k_snoop_pick(DevView V, const unsigned* __restrict__ flags, const int* __restrict__ perm,
                                                    const double* __restrict__ pose, const double* __restrict__ win, int mode,
                                                    int min_rows, const double* wt, double* conf, double* __restrict__ orig,
                                                    unsigned char* __restrict__ mask, int* __restrict__ prej) {
    RowGroup g;
    if (!rowpass_rows(V, flags, perm, g)) return;
    const bool barred = snoop_barred(flags);
    const double crit = win[2 * blockIdx.y + 1];        // (NaN: no row is a candidate)
    double best = __builtin_nan("");
    int bpos = kSnoopNoPos, cand = 0;
    for (int k = g.beg + g.sub; k < g.end; k += kRowLanes) {
        const int p = g.pw[k];
        if ((unsigned)p >= (unsigned)g.m) continue;
        const double wk = (V.wraw[g.mb + k] * g.inv_wmax) * conf[g.ob + k];
        const double ts = wt[g.mb + p];
        if (snoop_candidate(wk, ts, crit)) {
            cand += 1;
            pick(best, bpos, ts, k);
        }
    }
    snoop_exchange<1>(best, bpos, cand); snoop_exchange<2>(best, bpos, cand);
    snoop_exchange<4>(best, bpos, cand); snoop_exchange<8>(best, bpos, cand);
    const int left = g.live ? (int)pose[g.pb * 3 + 2] : 0;
    snoop_apply(V, g, snoop_decide(barred, left, cand, mode, min_rows), bpos, cand, crit, wt, conf, orig, mask, prej);
}

// The rejected rows of windows w0 + blockIdx.y get their confidences back; one thread per sorted row (perm is a bijection)
__global__ __launch_bounds__(256) void k_snoop_restore(const int* __restrict__ m_of, int w0, size_t obs_stride, size_t m_max,
                                                       const int* __restrict__ perm, double* __restrict__ conf,
                                                       const double* __restrict__ orig, unsigned char* __restrict__ mask) {
    const int w = w0 + blockIdx.y;
    const int m = min(m_of[w], (int)m_max);
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= m) return;
    const size_t mb = (size_t)w * m_max;
    const int p = perm[mb + s];
    if ((unsigned)p >= (unsigned)m || !mask[mb + p]) return;
    conf[(size_t)w * obs_stride + s] = orig[mb + p];
    mask[mb + p] = 0;
}

}  // namespace vba

// ---------------------------------------------------------------------------------------------------------- host side

static SnoopBufs snoop_bufs(vba_handle h) {
    Carver place{static_cast<char*>(h->q_snoop.d)};
    return snoop_layout(place, h->W, h->n_max, h->m_max);
}

// The scratch of the feature, allocated by the first vba_snoop with an empty mask
static int snoop_reserve(vba_handle h, SnoopBufs& b) {
    const size_t W = h->W, M = h->m_max;
    Carver count;
    snoop_layout(count, W, h->n_max, M);
    const bool fresh = h->q_snoop.d == nullptr;
    if (int rc = query_reserve(h, h->q_snoop, count.total(), "snooping scratch failed (a double and a byte per observation row of "
                                                             "every window)")) return rc;
    b = snoop_bufs(h);
    if (fresh) {
        HIPCHK(hipMemsetAsync(b.mask, 0, W * M, h->stream));
        h->snoop_total.assign(W, 0);
    }
    return VBA_OK;
}

static double* conf_of(vba_handle h) { return h->d_obs + 5 * (size_t)h->m_pad; }

// What an upload of observation rows does to the handle's bookkeeping, for a call that changes confidences in place
static int snoop_boundary(vba_handle h) {
    if (int rc = settle(h, true)) return rc;
    h->touch();
    h->carry_ok = false;
    return VBA_OK;
}

int snoop_forget_window(vba_handle h, int window) {
    if (h->snoop_total[window] == 0) return VBA_OK;
    HIPCHK(hipMemsetAsync(snoop_bufs(h).mask + (size_t)window * h->m_max, 0, (size_t)h->m_max, h->stream));
    h->snoop_total[window] = 0;
    return VBA_OK;
}

// What the two snooping calls check and reserve before the covariance step; `who` names the entry point in the messages
static int snoop_enter(vba_handle h, int iter, int mode, int min_rows, const char* who, RelBufs& rb, SnoopBufs& sb) {
    if (mode != 0 && mode != 1) return fail(VBA_EINVAL, "mode must be 0 (the largest w-test of a pose) or 1 (every flagged row)");
    if (min_rows < 0) return fail(VBA_EINVAL, "min_rows must be >= 0");
    if (h->sharded) return fail(VBA_ESTATE, std::string(who) + " does not serve observation-sharded handles");
    if (int rc = snoop_boundary(h)) return rc;
    if (int rc = cov_begin(h, iter, who)) return rc;
    if (int rc = rel_device_bufs(h, rb)) return rc;
    return snoop_reserve(h, sb);
}

// What a finished snooping call hands back: the per-pose counts summed into the totals, the cumulative mask, the flags
static int snoop_collect(vba_handle h, const SnoopBufs& sb, const CovQuery& q, unsigned char* rejected, int* counts, unsigned* flags) {
    const size_t W = h->W, N = h->n_max, M = h->m_max;
    std::vector<int> prej;
    try {
        prej.resize(W * N);
    } catch (const std::bad_alloc&) {
        return fail(VBA_ENOMEM, "host staging for the per-pose counts of vba_snoop failed");
    }
    HIPCHK(hipMemcpy(prej.data(), sb.prej, W * N * 4, hipMemcpyDeviceToHost));
    for (size_t w = 0; w < W; ++w) {
        int now = 0;
        for (int i = 0; i < h->n[w]; ++i) now += prej[w * N + i];
        h->snoop_total[w] += now;
        if (counts) { counts[2 * w] = now; counts[2 * w + 1] = h->snoop_total[w]; }
    }
    if (rejected) HIPCHK(hipMemcpy(rejected, sb.mask, W * M, hipMemcpyDeviceToHost));
    if (flags) HIPCHK(hipMemcpy(flags, q.flags, W * 4, hipMemcpyDeviceToHost));
    return VBA_OK;
}

int vba_snoop(vba_handle h, int iter, int damped, double crit, int mode, int min_rows, unsigned char* rejected, int* counts,
              unsigned* flags) {
    if (!h) return fail(VBA_EINVAL, "null handle");
    if (!(crit > 0.0)) return fail(VBA_EINVAL, "crit must be positive (+inf rejects nothing)");
    RelBufs rb;
    SnoopBufs sb;
    if (int rc = snoop_enter(h, iter, mode, min_rows, "vba_snoop", rb, sb)) return rc;
    hipStream_t s = h->stream;
    CovQuery q;
    if (int rc = cov_build_invert(h, iter, damped, q)) return rc;
    HIPCHK(hipMemsetAsync(sb.prej, 0, (size_t)h->W * h->n_max * 4, s));     // (blocks beyond a window's poses do not run)
    hipLaunchKernelGGL(k_snoop, rowpass_grid(h->n_max, h->W), dim3(256), 0, s, q.V, q.diag, q.flags, rb.perm, crit, mode, min_rows,
                       rb.wt, conf_of(h), sb.orig, sb.mask, sb.prej);
    HIPCHK(hipGetLastError());
    if (int rc = query_finish(h, h->q_snoop)) return rc;
    return snoop_collect(h, sb, q, rejected, counts, flags);
}

int vba_snoop_scaled(vba_handle h, int iter, int damped, double quantile, int mode, int min_rows, unsigned char* rejected, int* counts,
                     double* crit_used, double* s0sq, unsigned* flags) {
    if (!h) return fail(VBA_EINVAL, "null handle");
    if (!(quantile > 0.0)) return fail(VBA_EINVAL, "quantile must be positive (+inf rejects nothing)");
    RelBufs rb;
    SnoopBufs sb;
    if (int rc = snoop_enter(h, iter, mode, min_rows, "vba_snoop_scaled", rb, sb)) return rc;
    const size_t W = h->W, N = h->n_max;
    Carver count;
    snoop_fit_layout(count, W, N);
    if (int rc = query_reserve(h, h->q_snoop_fit, count.total(), "scaled snooping scratch failed (three doubles per pose of every "
                                                                 "window)")) return rc;
    Carver place{static_cast<char*>(h->q_snoop_fit.d)};
    const SnoopFitBufs fb = snoop_fit_layout(place, W, N);
    hipStream_t s = h->stream;
    CovQuery q;
    if (int rc = cov_build_invert(h, iter, damped, q)) return rc;
    HIPCHK(hipMemsetAsync(sb.prej, 0, W * N * 4, s));           // (blocks beyond a window's poses do not run)
    hipLaunchKernelGGL(k_snoop_fit, rowpass_grid(h->n_max, h->W), dim3(256), 0, s, q.V, q.diag, q.flags, rb.perm, rb.wt, fb.pose);
    hipLaunchKernelGGL(k_snoop_crit, dim3(h->W), dim3(64), 0, s, q.V.n, h->n_max, fb.pose, quantile, fb.win);
    hipLaunchKernelGGL(k_snoop_pick, rowpass_grid(h->n_max, h->W), dim3(256), 0, s, q.V, q.flags, rb.perm, fb.pose, fb.win, mode,
                       min_rows, rb.wt, conf_of(h), sb.orig, sb.mask, sb.prej);
    HIPCHK(hipGetLastError());
    if (int rc = query_finish(h, h->q_snoop)) return rc;
    if (crit_used || s0sq) {
        std::vector<double> win;
        try {
            win.resize(W * 2);
        } catch (const std::bad_alloc&) {
            return fail(VBA_ENOMEM, "host staging for the critical values of vba_snoop_scaled failed");
        }
        HIPCHK(hipMemcpy(win.data(), fb.win, W * 2 * 8, hipMemcpyDeviceToHost));
        for (size_t w = 0; w < W; ++w) {
            if (s0sq) s0sq[w] = win[2 * w];
            if (crit_used) crit_used[w] = win[2 * w + 1];
        }
    }
    return snoop_collect(h, sb, q, rejected, counts, flags);
}

int vba_snoop_restore(vba_handle h, int window) {
    if (!h) return fail(VBA_EINVAL, "null handle");
    if (window != -1) if (int rc = check_window(h, window)) return rc;
    if (int rc = snoop_boundary(h)) return rc;
    if (h->snoop_total.empty()) return VBA_OK;
    const int w0 = window < 0 ? 0 : window, w1 = window < 0 ? h->W : window + 1;
    bool any = false;
    for (int w = w0; w < w1; ++w) any = any || h->snoop_total[w] > 0;
    if (!any) return VBA_OK;
    HIPCHK(hipSetDevice(h->device));
    const int* d_perm = nullptr;
    if (int rc = rel_device_perm(h, &d_perm)) return rc;
    const SnoopBufs sb = snoop_bufs(h);
    hipLaunchKernelGGL(k_snoop_restore, dim3((unsigned)((h->m_max + 255) / 256), w1 - w0), dim3(256), 0, h->stream, h->V.m, w0,
                       (size_t)h->V.obs_stride, (size_t)h->m_max, d_perm, conf_of(h), sb.orig, sb.mask);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int w = w0; w < w1; ++w) h->snoop_total[w] = 0;
    return VBA_OK;
}

int vba_get_rejected(vba_handle h, unsigned char* rejected, int* totals) {
    if (!h) return fail(VBA_EINVAL, "null handle");
    const size_t W = h->W, M = h->m_max;
    if (totals)
        for (size_t w = 0; w < W; ++w) totals[w] = h->snoop_total.empty() ? 0 : h->snoop_total[w];
    if (!rejected) return VBA_OK;
    if (h->snoop_total.empty()) {
        std::memset(rejected, 0, W * M);
        return VBA_OK;
    }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(rejected, snoop_bufs(h).mask, W * M, hipMemcpyDeviceToHost));
    return VBA_OK;
}

int vba_last_snoop_ms(vba_handle h, float* ms) { return query_last_ms(h, &vba_context::q_snoop, ms, "no vba_snoop or vba_snoop_scaled has run"); }
