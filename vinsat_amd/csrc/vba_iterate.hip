// vba_iterate.hip -- the driver loop that hands every BA() call its states over PCIe: vba_iterate (states up, one call, result
// down), vba_iterate_open / vba_iterate_resident (the states stay on the device; the pipelined loop with its speculated next call)
// and the host watch that tells such a loop when the caller's buffers have changed under it.
#include "vba_context.h"


static int take_back(vba_handle h, double* states_out, double* lamda_out, double* last_hessian, int* n_trials, unsigned* flags) {
    if (h->back_valid) {        // read back together with the step: no second wait
        const WinScalars* sc = reinterpret_cast<const WinScalars*>(h->h_back + (size_t)h->n_max * 10);
        if (states_out) std::memcpy(states_out, h->h_back, (size_t)h->n[0] * 80);
        unpack_scalars(sc, h->par, lamda_out, last_hessian, n_trials, flags);
        return VBA_OK;
    }
    return vba_get_states(h, 0, states_out, lamda_out, last_hessian, n_trials, flags);
}

int vba_iterate(vba_handle h, int iter, int initialize, double lamda_in, const double* states_in, double* states_out,
                double* lamda_out, double* last_hessian, int* n_trials, unsigned* flags) {
    if (int rc = vba_set_states(h, 0, states_in, lamda_in)) return rc;
    // the next call of this kind replaces the states again: nothing to carry over
    if (int rc = step_impl(h, iter, initialize, nullptr, false, 0)) return rc;
    return take_back(h, states_out, lamda_out, last_hessian, n_trials, flags);
}

// ---------------------------------------------------------------------------------------------- the host watch
// vba_set_host_watch: buffers of the caller that a resident loop relies on (the device holds what was made from them)
static bool host_watch_changed(vba_handle h) {
    for (const auto& w : h->watch)
        if (w.live && std::memcmp(w.live, w.copy, w.bytes) != 0) return true;
    return false;
}
// ... the same on the handle's helper thread: begin before the enqueues, end once the device has answered.  Small watch lists
// (under 64 kB) are compared in place by watch_end: waking a thread costs more than that.
static size_t host_watch_bytes(vba_handle h) {
    size_t b = 0;
    for (const auto& w : h->watch) if (w.live) b += w.bytes;
    return b;
}
static bool watch_begin(vba_handle h) {
    if (host_watch_bytes(h) < 65536) return false;
    auto& W = h->ww;
    if (W.started && W.owner != getpid()) return false;     // forked child: no helper here, the caller compares in place
    if (!W.started) {
        W.started = true;
        W.owner = getpid();
        W.th = std::thread([h]() {
            auto& Q = h->ww;
            unsigned long long taken = 0;
            for (;;) {
                {
                    std::unique_lock<std::mutex> lk(Q.m);
                    Q.cv.wait(lk, [&] { return Q.quit || Q.seq != taken; });
                    if (Q.quit) return;
                    taken = Q.seq;
                }
                Q.changed = host_watch_changed(h);
                Q.done_seq.store(taken, std::memory_order_release);
            }
        });
    }
    {
        std::lock_guard<std::mutex> lk(W.m);
        ++W.seq;
    }
    W.cv.notify_one();
    return true;
}
static bool watch_end(vba_handle h, bool begun) {
    if (!begun) return host_watch_changed(h);
    auto& W = h->ww;
    // (bounded: a helper that does not answer within 20 ms -- a forked child has none, a starved host may park it -- is not waited
    // for; the comparison is then made here, beside it if it still runs: both only read)
    const auto t0 = std::chrono::steady_clock::now();
    const unsigned long long mine = W.seq;      // (written by this thread only)
    for (unsigned spins = 0; W.done_seq.load(std::memory_order_acquire) != mine; ++spins) {
        __builtin_ia32_pause();
        if ((spins & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) return host_watch_changed(h);
    }
    return W.changed;
}
// the helper has answered every request (a wait that gave up after 20 ms may have left it comparing): before the watch list changes
void watch_quiesce(vba_handle h) {
    auto& W = h->ww;
    if (!W.started || W.owner != getpid()) return;          // (a forked child has no helper to wait for)
    while (W.done_seq.load(std::memory_order_acquire) != W.seq) std::this_thread::yield();
}
void watch_stop(vba_handle h) {
    auto& W = h->ww;
    if (!W.started) return;
    if (W.owner != getpid()) {      // forked child: the thread object refers to a thread of the parent -- let go of it, never join
        W.th.detach();
        W.started = false;
        return;
    }
    {
        std::lock_guard<std::mutex> lk(W.m);
        W.quit = true;
    }
    W.cv.notify_one();
    W.th.join();
    W.started = false;
}

// ---------------------------------------------------------------------------------------------- the pipelined loop
static bool can_pipeline(vba_handle h) {
    // (whichever kernel forms the trial states of an unpivoted call -- the trial kernel, or with fusion bit 0 off the fused landmark-only
    // assembly / the recovery of the partitioned solve -- also writes them to mapped host memory)
    return h->pipeline && h->W == 1 && h->h_states_map && h->carry_enabled && h->warm_enabled >= 1 && h->fold_enabled && h->inline_select &&
           h->V.wbucket != nullptr && h->pivot_mode == 0 && h->V.chunk > 0 && h->V.lat;
}

// The driver loop `for iter in range(20): states, ... = BA(iter, states, ...)` (od_pipe.py:1036-1040) hands every call the
// result of the one before, through the host.  Served call by call the device idles while the host unpacks one result and
// enqueues the next call, and the host idles while the device works.  Here the two overlap: behind the call that is being
// returned the NEXT call is enqueued speculatively (what follows iter k is learnt from the caller: k + 1 until told
// otherwise), its first kernel evaluates the accept test of the call in front -- exactly the chained schedule of
// vba_run_schedule, one link at a time -- and the host waits only for that kernel plus a 40 kB copy on a side stream,
// while the rest of the speculated call runs under the caller's feet.  When the caller comes back with the predicted
// arguments the call is already on its way.  A wrong guess costs one call's worth of device time and the carried keys
// (settle); a first trial that is not cleanly accepted sends this call through the ordinary LM loop.  Same bits as
// vba_step: the kernels, their order inside a call and the accept test are those of the chained schedule.
static int iterate_pipelined(vba_handle h, int iter, int initialize, double* states_out, double* lamda_out, double* last_hessian,
                             int* n_trials, unsigned* flags) {
    if (int rc = ready(h)) return rc;
    if (int rc = flush_states(h)) return rc;        // (vba_iterate_open: the states it staged go up in front of the call)
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    constexpr int emit_kind = 2;
    initialize = initialize ? 1 : 0;
    // what the caller did after the previous resident call: remember it
    if (h->prev_res_iter >= 0) {
        h->pred_iter[h->prev_res_iter & 63] = iter;
        h->pred_init[h->prev_res_iter & 63] = initialize;
    }
    bool consumed = false;
    if (h->spec.valid) {
        if (h->spec.iter == iter && h->spec.init == initialize && h->spec.reg == h->reg) {
            consumed = true;
            h->spec_hits++;
        } else if (int rc = settle(h)) {
            return rc;
        }
    }
    CallAbandon abandon{h, true};       // (the speculation and what was learnt from the previous call go with an abandoned call)
    auto call_spec = [&](int c, int it, int in, int carry, bool fold) {
        CallSpec q;
        q.iter = it; q.initialize = in; q.call = c; q.par = (h->chain_par0 + c) & 1;
        q.carry = carry; q.emit = emit_kind; q.fold = fold;
        q.host_out = true;
        return q;
    };
    bool watch_changed = false;
    int c;                      // index of THIS call in the open chain
    if (consumed) {
        c = h->spec.c;
        h->spec.valid = false;
    } else {                    // open a chain with this call as its call 0
        const int carry0 = h->carry_ok;
        h->carry_ok = 0;
        h->shc.carried = false;
        h->chain_par0 = h->par;
        c = 0;
        const CallSpec q = call_spec(0, iter, initialize, carry0, false);
        CallCtx C;
        view_for_call(h, C.V, q);
        clear_abandoned_hists(h, C.V, s);
        if (!carry0 && h->hist_dirty) launch_clear_hist(C.V, 0, s);
        launch_reset_calls(C.V, s);
        h->h_head[0].call_idx = 0; h->h_head[0].done = 0; h->h_head[0].flags = 0;
        if (int rc = enqueue_front(h, C, q, false, nullptr)) return rc;
        enqueue_trial(h, C, q, true);
    }
    h->hist_dirty = true;
    // the call behind it, speculatively: its first kernel decides this one
    int ni = h->pred_iter[iter & 63], nin = h->pred_init[iter & 63];
    if (ni == -1) { ni = iter + 1; nin = initialize; }
    const bool speculate = ni >= 0;
    const CallSpec qc = call_spec(c, iter, initialize, emit_kind, false);       // (this call, as the stalled path needs it)
    const int par_c = qc.par;
    const bool watching = watch_begin(h);
    struct WatchJoin {          // (an early return must not leave the helper comparing buffers the caller may free)
        vba_handle h; bool begun; bool joined = false;
        bool end() { joined = true; return watch_end(h, begun); }
        ~WatchJoin() { if (begun && !joined) (void)watch_end(h, true); }
    } wj{h, watching};
    if (speculate) {
        const CallSpec qn = call_spec(c + 1, ni, nin, emit_kind, true);
        CallCtx C;
        view_for_call(h, C.V, qn);
        fill_params(C.V.prev, iter, initialize);
        C.after_first = h->ev_first;
        if (int rc = enqueue_front(h, C, qn, false, nullptr)) return rc;
        enqueue_trial(h, C, qn, true);
        // the first kernel of the speculated call has decided this one; the trial states and the outcome are in mapped host
        // memory by then (k_trial, fold_commit): no copy, the rest of the speculated call runs on under the caller's feet
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventSynchronize(h->ev_first));
        watch_changed = wj.end();       // (compared while the device worked)
    } else {                    // nothing resident is expected behind this call: decide it with a launch of its own
        CallCtx C;
        view_for_call(h, C.V, qc);
        launch_decide(C.V, nullptr, 0, s);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));
        watch_changed = wj.end();
    }
    h->stepped = true;
    h->last_pipelined = true;
    h->last_iter = iter;
    h->last_init = initialize;
    h->back_valid = false;
    const bool clean = (int)head(h, 0)->call_idx >= c + 1;
    if (clean) {
        h->par = par_c ^ 1;             // the trial buffer of this call is the next call's input
        const volatile WinHead* hd = head(h, 0);
        if (states_out) std::memcpy(states_out, h->h_states_map + (size_t)par_c * h->n_max * 10, (size_t)h->n[0] * 80);
        if (lamda_out) *lamda_out = hd->lamda;
        if (last_hessian) for (int k = 0; k < 81; ++k) last_hessian[k] = hd->last_hessian[k];
        if (n_trials) *n_trials = 1;    // (a clean first trial)
        if (flags) *flags = (hd->flags & 7u) | (watch_changed ? VBA_FLAG_HOST_CHANGED : 0u);
        if (speculate) {
            h->spec.valid = true; h->spec.iter = ni; h->spec.init = nin; h->spec.reg = h->reg; h->spec.c = c + 1;
            h->carry_ok = 0;            // (the keys of the result belong to the speculated call now; settle() keeps the books)
        } else {
            h->carry_ok = emit_kind;
        }
        h->prev_res_iter = iter;
        abandon.armed = false;
        return VBA_OK;
    }
    // Not a clean first trial (rejected, pivot check failed, warm select missed): the speculated call has skipped itself
    // (the window never moved on to it); finish this call the ordinary way.
    HIPCHK(hipStreamSynchronize(s));
    {
        std::vector<int> stall_at(1, c);
        long trials = 0;
        if ((int)head(h, 0)->call_idx != c) return fail(VBA_ESTATE, "pipelined call: the window is at call " + std::to_string(head(h, 0)->call_idx) + ", expected " + std::to_string(c));
        if (int rc = finish_stalled_call(h, qc, stall_at, trials)) return rc;
    }
    h->par = par_c ^ 1;
    h->carry_ok = emit_kind;            // the accepted (or last) trial left the next call's keys behind
    h->prev_res_iter = iter;
    abandon.armed = false;
    if (int rc = vba_get_states(h, 0, states_out, lamda_out, last_hessian, n_trials, flags)) return rc;
    if (flags && watch_changed) *flags |= VBA_FLAG_HOST_CHANGED;
    return VBA_OK;
}

// vba_iterate as the FIRST call of a driver loop whose following calls will be vba_iterate_resident: the states go up, and the call
// itself is served like a resident one -- returned as soon as its accept test is known, with the next call already enqueued behind
// it (a caller that does not come back with a resident call pays for that speculation: use vba_iterate there).
int vba_iterate_open(vba_handle h, int iter, int initialize, double lamda_in, const double* states_in, double* states_out,
                     double* lamda_out, double* last_hessian, int* n_trials, unsigned* flags) {
    if (int rc = vba_set_states(h, 0, states_in, lamda_in)) return rc;
    if (can_pipeline(h)) return iterate_pipelined(h, iter, initialize, states_out, lamda_out, last_hessian, n_trials, flags);
    const bool watch_changed = host_watch_changed(h);       // (like every resident call: the caller relies on it)
    if (int rc = step_impl(h, iter, initialize, nullptr, false, 0)) return rc;
    if (int rc = take_back(h, states_out, lamda_out, last_hessian, n_trials, flags)) return rc;
    if (flags && watch_changed) *flags |= VBA_FLAG_HOST_CHANGED;
    return VBA_OK;
}

// The next call of a driver loop that hands BA() the states it got back from the previous call: nothing to upload, the
// device already holds them (and the carried keys of the last accepted trial stay usable).
int vba_iterate_resident(vba_handle h, int iter, int initialize, double* states_out, double* lamda_out, double* last_hessian,
                         int* n_trials, unsigned* flags) {
    if (!h) return fail(VBA_EINVAL, "null handle");
    if (!h->stepped) return fail(VBA_ESTATE, "vba_iterate_resident follows a call that left its result on the device");
    if (can_pipeline(h)) return iterate_pipelined(h, iter, initialize, states_out, lamda_out, last_hessian, n_trials, flags);
    const bool watch_changed = host_watch_changed(h);
    if (int rc = step_impl(h, iter, initialize, nullptr, true, 0)) return rc;
    if (int rc = take_back(h, states_out, lamda_out, last_hessian, n_trials, flags)) return rc;
    if (flags && watch_changed) *flags |= VBA_FLAG_HOST_CHANGED;
    return VBA_OK;
}
