// vba_query.hip -- the host scaffold of the queries at the resident states (vba_covariance, vba_reliability, vba_outlier_power,
// vba_snoop, vba_snoop_scaled): the checks they start with, their scratch and timing, and the step they share -- the front of a full
// -phase call on a SHADOW view (see vba_cov.hip) followed by the selected inversion (launch_cov_invert, vba_cov.hip).
#include "vba_context.h"

// The scratch of the covariance step (CovBufs): the shadow of every array the front of a call writes (into V), and what the selected
// inversion writes.  Sizes come from V alone, so the counting and the placing run agree by construction.
static CovBufs cov_layout(Carver& c, DevView& V, size_t W) {
    const size_t N = V.n_max, M = V.m_max, PR = (size_t)V.p_max;
    CovBufs b;
    b.sc = c.take<WinScalars>(W);
    V.sc = b.sc;
    V.absr = c.take<double>(W * 2 * M);
    V.wraw = c.take<double>(W * M);
    V.ckeys = c.take<double>(W * 2 * M);
    V.part_init = c.take<double>(W * V.nblk_obs);
    V.part_trial = c.take<double>(W * V.trial_stride);
    V.part_next = c.take<double>(W * V.nblk_obs);
    V.part_pred = c.take<double>(W * 2 * V.pred_stride);
    V.part_prior = c.take<double>(W * 2 * V.pred_stride);
    V.lastD = c.take<double>(W * 81);
    V.hist = c.take<unsigned>(W * kHistStride);
    V.Hraw = c.take<double>(W * N * 21);
    V.braw = c.take<double>(W * N * 6);
    {
        double* d = c.take<double>(W * N * (6 + 36 + 6 + 1 + 3 + 9 + 9 + 9));
        V.xhat = d; d += W * N * 6; V.Phi = d; d += W * N * 36; V.rorb = d; d += W * N * 6; V.fatt = d; d += W * N;
        V.qgrad = d; d += W * N * 3; V.Hd = d; d += W * N * 9; V.Hu = d; d += W * N * 9; V.Hl = d;
    }
    V.bands = c.take<double>(W * N * 243);
    V.rhs = c.take<double>(W * N * 9);
    V.states_new = c.take<double>(W * N * 10);
    b.pool = c.take<double>(W * 2 * (size_t)V.long_pool_cap * 6);
    b.diag = c.take<double>(W * N * 81);
    b.sup = c.take<double>(W * N * 81);
    b.flags = c.take<unsigned>(W);
    b.X = c.take<double>(W * N * 162);
    b.contrib = c.take<double>(W * PR * 243);
    b.sepb = c.take<double>(W * PR * 243);
    b.SSd = c.take<double>(W * PR * 81);
    b.SSs = c.take<double>(W * PR * 81);
    return b;
}

int query_reserve(vba_handle h, QueryScratch& q, size_t bytes, const char* what) {
    if (q.cap >= bytes) return VBA_OK;
    if (q.d) (void)hipFree(q.d);
    q.d = nullptr;
    q.cap = 0;
    if (hipMalloc(&q.d, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(VBA_ENOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes of " + what);
    }
    q.cap = bytes;
    return VBA_OK;
}

int query_finish(vba_handle h, QueryScratch& q) {
    if (!q.ev) HIPCHK(hipEventCreate(&q.ev));
    HIPCHK(hipEventRecord(q.ev, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipEventElapsedTime(&q.ms, h->cov_ev0, q.ev));
    q.ran = true;
    return VBA_OK;
}

int query_last_ms(vba_handle h, QueryScratch vba_context::*q, float* ms, const char* none_ran) {
    if (!h || !ms) return fail(VBA_EINVAL, "null argument");
    if (!(h->*q).ran) return fail(VBA_ESTATE, none_ran);
    *ms = (h->*q).ms;
    return VBA_OK;
}

// per-window results: rows beyond a window's count stay as the caller left them
int query_copy_out(double* out, const double* dev, size_t W, size_t stride, const std::vector<int>& used, size_t per) {
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

// What every query checks first: the arguments, the handle's mode, a speculated call (dropped as a mismatched resident call drops
// it), states in every window.  `who` names the entry point in the messages.
int cov_begin(vba_handle h, int iter, const char* who) {
    if (!h) return fail(VBA_EINVAL, "null handle");
    if (iter < 0) return fail(VBA_EINVAL, "iter must be >= 0");
    if (h->sharded) return fail(VBA_ESTATE, std::string(who) + " does not serve observation-sharded handles");
    if (int rc_settle = settle(h)) return rc_settle;        // a speculated call is dropped as a mismatched resident call drops it
    if (int rc = ready(h)) return rc;
    HIPCHK(hipSetDevice(h->device));
    return VBA_OK;
}

// The shadow front and the selected inversion, enqueued on the handle's stream into the scratch of the query: the step
// vba_covariance (vba_cov.hip), vba_reliability (vba_rel.hip), vba_outlier_power (vba_power.hip) and the snoops (vba_snoop.hip)
// share.  cov_ev0 is recorded in front of it; the caller ends with query_finish.  q: the shadow view (its wraw, its window scalars
// with the maximum raw weight and its bands stay valid until the next query) and the device results.
int cov_build_invert(vba_handle h, int iter, int damped, CovQuery& q) {
    hipStream_t s = h->stream;
    const size_t W = h->W;
    // the shadow view: the view of the next call (parity h->par, full phase, nothing carried, nothing emitted) with every array
    // the front writes redirected into the scratch
    CallSpec c;
    c.iter = iter; c.initialize = 0; c.call = -1; c.par = h->par; c.emit = 0; c.carry = 0;
    DevView& V = q.V;
    view_for_call(h, V, c);
    Carver count;
    cov_layout(count, V, W);
    if (int rc = query_reserve(h, h->q_cov, count.total(), "covariance scratch failed")) return rc;
    if (!h->cov_ev0) HIPCHK(hipEventCreate(&h->cov_ev0));
    Carver place{static_cast<char*>(h->q_cov.d)};
    const CovBufs b = cov_layout(place, V, W);
    V.wbucket = nullptr;            // nothing carried: the bin buckets are neither read nor written
    V.wmax_ext = nullptr;
    V.hist0_ext[0] = V.hist0_ext[1] = nullptr;
    V.sel_slots = nullptr;
    V.host_states = nullptr;
    V.sel_inline = 0;
    V.dyn_in_acc = 0;
    // the window scalars as the next call would find them, without a pending repeat
    std::vector<WinScalars> hsc(W);
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipMemcpy(hsc.data(), h->V.sc, W * sizeof(WinScalars), hipMemcpyDeviceToHost));
    for (auto& x : hsc) { x.miss = 0; x.call_idx = 0; x.pending = -1; }
    HIPCHK(hipMemcpyAsync(b.sc, hsc.data(), W * sizeof(WinScalars), hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(h->cov_ev0, s));
    if (V.nblk_long > 0)
        HIPCHK(hipMemcpyAsync(b.pool, h->V.long_pool, W * 2 * (size_t)V.long_pool_cap * 6 * 8, hipMemcpyDeviceToDevice, s));
    V.long_pool = b.pool;
    HIPCHK(hipMemsetAsync(V.hist, 0, W * kHistStride * 4, s));
    // the front of a full-phase call with nothing carried (enqueue_front, the profiled order), then the assembly
    launch_obs_residual(V, nullptr, s);
    launch_select(V, false, s);
    V.median_ready = V.lat ? 0 : 1;
    if (V.median_ready) launch_select_finish(V, s);
    launch_obs_accumulate(V, s);
    launch_dynamics(V, s);
    launch_assemble(V, 0, s);
    if (int rc = launch_cov_invert(h, V, b, damped, s)) return rc;
    q.diag = b.diag;
    q.sup = b.sup;
    q.flags = b.flags;
    return VBA_OK;
}
