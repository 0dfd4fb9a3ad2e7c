// vba_debug.hip -- vba_debug_fetch: the intermediates of the last call, for tests and diagnostics.
#include "vba_context.h"

namespace {
// Where a fetch goes.  room(cnt): the caller's buffer holds cnt doubles, and *count says so; copy: ... filled from the device.
struct DebugOut {
    double* out;
    int64_t capacity;
    int64_t* count;
    int room(int64_t cnt) const {
        if (cnt > capacity) return fail(VBA_EINVAL, "debug buffer too small");
        *count = cnt;
        return VBA_OK;
    }
    int copy(const double* src, int64_t cnt) const {
        if (int rc = room(cnt)) return rc;
        HIPCHK(hipMemcpy(out, src, cnt * 8, hipMemcpyDeviceToHost));
        return VBA_OK;
    }
};

// d_dbg holds the 15 doubles per row that k_debug_project writes
int ensure_dbg(vba_handle h, size_t need) {
    if (h->dbg_cap >= need) return VBA_OK;
    if (h->d_dbg) hipFree(h->d_dbg);
    h->d_dbg = nullptr;
    h->dbg_cap = 0;
    HIPCHK(hipMalloc(&h->d_dbg, need));
    h->dbg_cap = need;
    return VBA_OK;
}

// VBA_DBG_EST / WEIGHT / JG: `per` doubles per row, re-projected now and scattered from the sorted order back to the caller's
int fetch_rows(vba_handle h, const DevView& V, int window, int what, const DebugOut& o) {
    const int64_t m = h->m[window];
    const int64_t per = what == VBA_DBG_EST ? 2 : (what == VBA_DBG_JG ? 12 : 1);
    if (int rc = o.room(m * per)) return rc;
    if (int rc = ensure_dbg(h, (size_t)m * 15 * 8)) return rc;
    double* est = h->d_dbg;
    double* J = est + 2 * m;
    double* wt = J + 12 * m;
    launch_debug_project(V, window, (int)m, est, J, wt, h->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    std::vector<double> tmp((size_t)m * per);
    const double* src = what == VBA_DBG_EST ? est : (what == VBA_DBG_JG ? J : wt);
    HIPCHK(hipMemcpy(tmp.data(), src, (size_t)m * per * 8, hipMemcpyDeviceToHost));
    const std::vector<int64_t>& perm = h->perm[window];
    for (int64_t s = 0; s < m; ++s) std::memcpy(o.out + perm[s] * per, tmp.data() + s * per, per * 8);
    return VBA_OK;
}

// VBA_DBG_NEXT_*: what the trial kernel of the last call left for the next one (k_trial EMIT), as that call will read it -- the slots
// of the parity V.par ^ 1.  Read-only.  A call that emitted nothing (key carry off), or whose carried data the host has dropped since
// (vba_set_states, an abandoned call), has nothing to show.
int fetch_next(vba_handle h, const DevView& V, const WinScalars& sc, int window, int what, const DebugOut& o) {
    const int kind = h->carry_enabled ? h->carry_ok : 0;
    if (!kind)
        return fail(VBA_ESTATE, "the last call carried nothing into the next one (key carry is off, or the states were replaced behind it)");
    const int64_t m = h->m[window];
    const int np = V.par ^ 1;       // parity of the call that reads
    switch (what) {
        case VBA_DBG_NEXT_KEYS: {
            if (int rc = o.room(2 * m)) return rc;
            std::vector<double> tmp((size_t)m * 2);
            HIPCHK(hipMemcpy(tmp.data(), V.absr + 2 * (size_t)window * V.m_max, (size_t)m * 16, hipMemcpyDeviceToHost));
            const std::vector<int64_t>& perm = h->perm[window];
            for (int64_t s = 0; s < m; ++s) std::memcpy(o.out + perm[s] * 2, tmp.data() + s * 2, 16);
            return VBA_OK;
        }
        case VBA_DBG_NEXT_HIST: {
            const int bins = kind == 2 ? kSelBins : 1024;
            if (int rc = o.room(4 + bins)) return rc;
            std::vector<unsigned> hist(bins);
            HIPCHK(hipMemcpy(hist.data(), V.hist + (size_t)window * kHistStride + (size_t)np * kSelBins, (size_t)bins * 4, hipMemcpyDeviceToHost));
            o.out[0] = kind;
            std::memcpy(o.out + 1, &sc.warm_lo[np], 8);      // (raw bits)
            o.out[2] = V.warm_shift;
            o.out[3] = (double)sc.sel_rank[0];
            for (int b = 0; b < bins; ++b) o.out[4 + b] = hist[b];
            return VBA_OK;
        }
        case VBA_DBG_NEXT_BUCKETS: {
            if (!V.wbucket) return fail(VBA_ESTATE, "this handle has no bin buckets (it runs the bandwidth-mode kernels)");
            if (kind != 2) return fail(VBA_ESTATE, "the last call left the exponent histogram: only a warm histogram comes with bin buckets");
            const int64_t cnt = (int64_t)kSelBins * V.bucket_cap;
            if (int rc = o.room(1 + cnt)) return rc;
            o.out[0] = V.bucket_cap;
            HIPCHK(hipMemcpy(o.out + 1, V.wbucket + ((size_t)window * 2 + np) * kSelBins * (size_t)V.bucket_cap, (size_t)cnt * 8, hipMemcpyDeviceToHost));
            return VBA_OK;
        }
        default: return o.copy(V.part_next + (size_t)window * V.nblk_obs, V.nblk_obs);
    }
}
}  // namespace

int vba_debug_fetch(vba_handle h, int window, int what, double* out, int64_t capacity, int64_t* count) {
    if (int rc = check_window(h, window)) return rc;
    if (int rc_settle = settle(h)) return rc_settle;
    if (!out || !count) return fail(VBA_EINVAL, "null output");
    if (!h->stepped) return fail(VBA_ESTATE, "no step has run");
    if (h->last_pipelined)
        return fail(VBA_ESTATE, "the last call was a pipelined vba_iterate_resident: the call speculated behind it has reused its scratch "
                                "(maximum weight, step, trial states); switch the pipeline off (vba_set_pipeline(h, 0)) to inspect intermediates");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int n = h->n[window];
    const size_t pb = (size_t)window * h->n_max;
    // the view of the call that ran last: its input states are in the buffer of the other parity by now
    DevView V;
    {
        CallSpec c;
        c.iter = h->last_iter; c.initialize = h->last_init; c.call = -1; c.par = h->par ^ 1;
        view_for_call(h, V, c);
    }
    const DebugOut o{out, capacity, count};
    WinScalars sc;
    HIPCHK(hipMemcpy(&sc, V.sc + window, sizeof(sc), hipMemcpyDeviceToHost));
    double wmax;
    std::memcpy(&wmax, &sc.wmax_bits[V.par], 8);
    switch (what) {
#ifdef VBA_ENTRY_STAMPS
        case 103: {         // diagnostic build: the host stamps around the entry of a chained schedule (vba_context.h): count, ns per interval
            if (int rc = o.room(12)) return rc;
            for (int k = 0; k < 6; ++k) { out[2 * k] = g_estamps.cnt[k]; out[2 * k + 1] = g_estamps.sum[k]; }
            g_estamps = EntryStamps();
            return VBA_OK;
        }
#endif
#ifdef VBA_RESIDENT_STAMPS
        case 100:           // diagnostic build: the wall-clock stamps of the last k_solve_resident launch (raw 64-bit words)
            return o.copy(V.cR2 + (size_t)window * V.res_stride * 4, (int64_t)V.res_stride * 4);
        case 102: {         // ... and along k_trial and k_obs_accumulate (fetch_ostamps, vba_trial.hip): 64 raw words
            if (int rc = o.room(64)) return rc;
            fetch_ostamps(reinterpret_cast<unsigned long long*>(out));
            return VBA_OK;
        }
        case 101: {         // ... and of one thread along the solve kernels (g_kstamps, vba_solve_step.h): 128 raw words
            if (int rc = o.room(128)) return rc;
            fetch_kstamps(reinterpret_cast<unsigned long long*>(out));
            return VBA_OK;
        }
#endif
        case VBA_DBG_EST:
        case VBA_DBG_WEIGHT:
        case VBA_DBG_JG: return fetch_rows(h, V, window, what, o);
        case VBA_DBG_H: {
            if (int rc = o.room((int64_t)n * 36)) return rc;
            std::vector<double> tmp((size_t)n * 21);
            HIPCHK(hipMemcpy(tmp.data(), V.Hraw + pb * 21, (size_t)n * 21 * 8, hipMemcpyDeviceToHost));
            for (int i = 0; i < n; ++i)
                for (int a = 0; a < 6; ++a)
                    for (int b = 0; b < 6; ++b) out[(size_t)i * 36 + a * 6 + b] = tmp[(size_t)i * 21 + sym6(a, b)] / wmax;
            return VBA_OK;
        }
        case VBA_DBG_B: {
            if (int rc = o.copy(V.braw + pb * 6, (int64_t)n * 6)) return rc;
            for (int64_t k = 0; k < (int64_t)n * 6; ++k) out[k] /= wmax;
            return VBA_OK;
        }
        case VBA_DBG_PHI: return o.copy(V.Phi + pb * 36, (int64_t)n * 36);
        case VBA_DBG_RPRED: {
            if (int rc = o.room((int64_t)(n - 1) * 7)) return rc;
            std::vector<double> ro((size_t)n * 6), fa(n);
            HIPCHK(hipMemcpy(ro.data(), V.rorb + pb * 6, (size_t)n * 48, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(fa.data(), V.fatt + pb, (size_t)n * 8, hipMemcpyDeviceToHost));
            for (int i = 0; i < n - 1; ++i) {
                for (int r = 0; r < 6; ++r) out[(size_t)i * 7 + r] = ro[(size_t)i * 6 + r];
                out[(size_t)i * 7 + 6] = fa[i];
            }
            return VBA_OK;
        }
        case VBA_DBG_QGRAD: return o.copy(V.qgrad + pb * 3, (int64_t)n * 3);
        case VBA_DBG_HQ: {
            if (int rc = o.room((int64_t)n * 27)) return rc;
            std::vector<double> d((size_t)n * 9), u((size_t)n * 9), l((size_t)n * 9);
            HIPCHK(hipMemcpy(d.data(), V.Hd + pb * 9, (size_t)n * 72, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(u.data(), V.Hu + pb * 9, (size_t)n * 72, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(l.data(), V.Hl + pb * 9, (size_t)n * 72, hipMemcpyDeviceToHost));
            for (int i = 0; i < n; ++i)
                for (int k = 0; k < 9; ++k) {
                    out[(size_t)i * 27 + k] = l[(size_t)i * 9 + k];
                    out[(size_t)i * 27 + 9 + k] = d[(size_t)i * 9 + k];
                    out[(size_t)i * 27 + 18 + k] = u[(size_t)i * 9 + k];
                }
            return VBA_OK;
        }
        case VBA_DBG_BANDS: {
            // latency mode never writes the bands to memory (the chunk kernel forms its blocks in LDS): form them now
            // (VBA_DBG_RAW_BANDS: diagnostic -- fetch what is in memory instead)
            if (!std::getenv("VBA_DBG_RAW_BANDS")) launch_assemble(V, 0, h->stream);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(h->stream));
            if (int rc = o.copy(V.bands + pb * 243, (int64_t)n * 243)) return rc;
            if (h->last_init) {     // landmark-only phase: the off-diagonal blocks are zero and are not written
                for (int i = 0; i < n; ++i) {
                    std::memset(out + (size_t)i * 243, 0, 81 * 8);
                    std::memset(out + (size_t)i * 243 + 162, 0, 81 * 8);
                }
            }
            return VBA_OK;
        }
        case VBA_DBG_RHS: {
            if (!std::getenv("VBA_DBG_RAW_BANDS")) launch_assemble(V, 0, h->stream);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(h->stream));
            return o.copy(V.rhs + pb * 9, (int64_t)n * 9);
        }
        case VBA_DBG_DPOSE: return o.copy(V.dpose + pb * 9, (int64_t)n * 9);
        case VBA_DBG_SCALARS: {
            if (int rc = o.room(8)) return rc;
            StepParams p;
            fill_params(p, h->last_iter, h->last_init);
            out[0] = sc.c_obs; out[1] = wmax; out[2] = sc.init_residual; out[3] = sc.trial_residual;
            out[4] = sc.lam32; out[5] = p.sigma; out[6] = p.alpha; out[7] = (double)sc.n_trials;
            return VBA_OK;
        }
        case VBA_DBG_NEXT_KEYS:
        case VBA_DBG_NEXT_HIST:
        case VBA_DBG_NEXT_BUCKETS:
        case VBA_DBG_PART_NEXT: return fetch_next(h, V, sc, window, what, o);
        case VBA_DBG_PART_TRIAL: {
            // the block sums of the last trial behind the geometry they were written in (launch_trial_emit reads the same fields)
            if (int rc = o.room(8 + (int64_t)V.trial_stride)) return rc;
            const bool split = V.fused_trial == 0 && !V.lat && !V.wbucket;
            const int emit = h->carry_enabled ? h->carry_ok : 0;
            out[0] = V.nblk_obs; out[1] = V.nblk_dyn; out[2] = h->last_init ? 0 : V.nblk_long; out[3] = V.fused_trial;
            out[4] = (V.fused_trial == 0 && !split && emit == 2) ? V.trial_tiles : 1; out[5] = emit; out[6] = split ? 1 : 0;
            out[7] = V.wbucket ? V.bucket_cap : 0;
            HIPCHK(hipMemcpy(out + 8, V.part_trial + (size_t)window * V.trial_stride, (size_t)V.trial_stride * 8, hipMemcpyDeviceToHost));
            return VBA_OK;
        }
        default: return fail(VBA_EINVAL, "unknown debug selector");
    }
}
