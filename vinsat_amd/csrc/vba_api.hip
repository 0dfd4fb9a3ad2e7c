// vba_api.hip -- C ABI of libvinsat_ba.so (see include/vinsat_ba.h): error reporting, what every entry point leans on (settle, ready,
// read_heads), and the getters that fit nowhere else.  The rest of the ABI lives by role: vba_handle.hip, vba_options.hip,
// vba_upload.hip, vba_debug.hip and the units listed at the top of vba_context.h.
#include "vba_context.h"

thread_local std::string g_err;
#ifdef VBA_ENTRY_STAMPS
EntryStamps g_estamps;
#endif

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

void fill_params(StepParams& p, int iter, int initialize) {
    // BA_filtering.py:22: alpha = min(max(1 - (2*(iter/5) - 1), 1), 2);  :26: Sigma = min(10000*(iter+1)**2, 1000000)
    double alpha = 1.0 - (2.0 * ((double)iter / 5.0) - 1.0);
    alpha = std::min(std::max(alpha, 1.0), 2.0);
    const double it1 = (double)iter + 1.0;
    const double sigma = std::min(10000.0 * it1 * it1, 1000000.0);
    p.alpha = alpha;
    p.am2 = std::fabs(alpha - 2.0);
    p.expo = alpha / 2.0 - 1.0;
    p.alpha_is_2 = alpha == 2.0;
    p.sigma = sigma;
    p.sqrt_sigma = std::sqrt(sigma);
    p.initialize = initialize ? 1 : 0;
    p.iter = iter;
    p.pad = 0;
}

int check_window(vba_handle h, int window) {
    if (!h) return fail(VBA_EINVAL, "null handle");
    if (window < 0 || window >= h->W) return fail(VBA_EINVAL, "window index out of range");
    return VBA_OK;
}

// k_decide wrote the outcome of the trial into mapped host memory; waiting for the stream is all that is needed
int read_heads(vba_handle h) {
    HIPCHK(hipStreamSynchronize(h->stream));
    VBA_ESTAMP(0);
    for (int w = 0; w < h->W; ++w)
        if (h->h_head[w].flags & 64u)       // k_solve_resident: a consumer block gave up waiting for its producers
            return fail(VBA_ESTATE, "resident solve: a block of window " + std::to_string(w) + " timed out waiting for its producers (vba_set_fusion bits 5, 6)");
    return VBA_OK;
}

const volatile WinHead* head(vba_handle h, int w) { return h->h_head + w; }

// A call that vba_iterate_resident enqueued speculatively (iterate_pipelined) and that the caller did not ask for after all
// -- or that anything else than the next resident call is about to disturb: wait for it and forget it.  It has run its
// front and its first trial but nobody decided it: its input states, the result the caller holds, are intact (call
// parity), its trial states and everything keyed to them are dropped.  `boundary`: the caller left the resident loop
// (uploads, new states): remember not to speculate behind a call with that iter again.
// Staged states go up first (flush_states, vba_upload.hip) unless `keep_staged`.
int settle(vba_handle h, bool boundary, bool keep_staged) {
    if (!h) return VBA_OK;
    if (!keep_staged) { if (int rc = flush_states(h)) return rc; }
    if (!h->spec.valid) {
        // the caller left the resident loop behind a call that had speculated nothing: what it does next is not "what follows
        // that iter" (learning across a window boundary made every second window waste a speculated call)
        if (boundary) h->prev_res_iter = -1;
        return VBA_OK;
    }
    HIPCHK(hipSetDevice(h->device));
    launch_reset_calls(h->V, h->stream);            // (also clears a missed warm select the dropped call may have recorded)
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int w = 0; w < h->W; ++w) h->h_head[w].flags = 0;
    h->par = (h->chain_par0 + h->spec.c) & 1;      // S[par]: the input of the speculated call = the last result
    h->carry_ok = 0;                                // its trial consumed the carried keys and left its own
    h->need_hist_reset = true;
    h->hist_dirty = false;
    h->spec.valid = false;
    h->spec_discards++;
    if (boundary && h->prev_res_iter >= 0) h->pred_iter[h->prev_res_iter & 63] = -2;
    h->prev_res_iter = -1;
    return VBA_OK;
}

int ready(vba_handle h) {
    for (int w = 0; w < h->W; ++w)
        if (!h->have_obs[w] || !h->have_win[w] || !h->have_state[w])
            return fail(VBA_ESTATE, "window " + std::to_string(w) + " is missing observations, pose constants or states");
    if (h->reg)
        for (int w = 0; w < h->W; ++w)
            if (!h->have_prior[w]) return fail(VBA_ESTATE, "window " + std::to_string(w) + " has no prior (vba_upload_prior)");
    return VBA_OK;
}

int vba_version(void) { return 230; }     // 2.3: vba_covariance; 2.2: VBA_OPT_JACOBIAN_F32 (2.1: vba_set_chunk_waves, fusion bits 2..4, warm select mode 3)

const char* vba_last_error(void) { return g_err.c_str(); }

int vba_device_count(int* count) {
    if (!count) return fail(VBA_EINVAL, "null count");
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
    *count = c;
    return VBA_OK;
}

int vba_has_variants(void) {
#ifdef VBA_VARIANTS
    return 1;
#else
    return 0;
#endif
}

int vba_get_mode(vba_handle h, int* mode, int* chunk) {
    if (!h) return fail(VBA_EINVAL, "null handle");
    if (mode) *mode = h->V.lat;
    if (chunk) *chunk = h->V.chunk;
    return VBA_OK;
}

int vba_last_step_ms(vba_handle h, float* ms) {
    if (!h || !ms) return fail(VBA_EINVAL, "null argument");
    if (!h->stepped) return fail(VBA_ESTATE, "no step has run");
    *ms = h->last_ms;
    return VBA_OK;
}
