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
    const bool barred = (flags[blockIdx.y] & (VBA_FLAG_ZERO_PIVOT | VBA_FLAG_NONFINITE | VBA_FLAG_INDEFINITE)) != 0u;
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
    // the decision of the pose (uniform over its 16 lanes)
    const int left = (int)cnt;
    bool all = false, one = false;
    if (!barred && cand > 0) {
        if (mode == 1 && left - cand >= min_rows) all = true;
        else if (left - 1 >= min_rows) one = true;
    }
    if (all) {
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
    } else if (one && bpos >= g.beg && bpos < g.end && (bpos - g.beg) % kRowLanes == g.sub) {
        const int p = g.pw[bpos];
        if ((unsigned)p < (unsigned)g.m) {
            orig[g.mb + p] = conf[g.ob + bpos];
            conf[g.ob + bpos] = 0.0;
            mask[g.mb + p] = 1;
        }
    }
    if (g.live && g.sub == 0) prej[g.pb] = all ? cand : (one ? 1 : 0);
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

int vba_snoop(vba_handle h, int iter, int damped, double crit, int mode, int min_rows, unsigned char* rejected, int* counts,
              unsigned* flags) {
    if (!h) return fail(VBA_EINVAL, "null handle");
    if (!(crit > 0.0)) return fail(VBA_EINVAL, "crit must be positive (+inf rejects nothing)");
    if (mode != 0 && mode != 1) return fail(VBA_EINVAL, "mode must be 0 (the largest w-test of a pose) or 1 (every flagged row)");
    if (min_rows < 0) return fail(VBA_EINVAL, "min_rows must be >= 0");
    if (h->sharded) return fail(VBA_ESTATE, "vba_snoop does not serve observation-sharded handles");
    if (int rc = snoop_boundary(h)) return rc;
    if (int rc = cov_begin(h, iter, "vba_snoop")) return rc;
    RelBufs rb;
    if (int rc = rel_device_bufs(h, rb)) return rc;
    SnoopBufs sb;
    if (int rc = snoop_reserve(h, sb)) return rc;
    const size_t W = h->W, N = h->n_max, M = h->m_max;
    hipStream_t s = h->stream;
    CovQuery q;
    if (int rc = cov_build_invert(h, iter, damped, q)) return rc;
    HIPCHK(hipMemsetAsync(sb.prej, 0, W * N * 4, s));           // (blocks beyond a window's poses do not run)
    hipLaunchKernelGGL(k_snoop, rowpass_grid(h->n_max, h->W), dim3(256), 0, s, q.V, q.diag, q.flags, rb.perm, crit, mode, min_rows,
                       rb.wt, conf_of(h), sb.orig, sb.mask, sb.prej);
    HIPCHK(hipGetLastError());
    if (int rc = query_finish(h, h->q_snoop)) return rc;
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

int vba_last_snoop_ms(vba_handle h, float* ms) { return query_last_ms(h, &vba_context::q_snoop, ms, "no vba_snoop has run"); }
