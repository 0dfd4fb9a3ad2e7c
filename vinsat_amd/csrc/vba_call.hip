// vba_call.hip -- one BA() call as the host enqueues it: the view its kernels take, its front and its LM trials, the call on its
// own (vba_step, vba_step_profiled) and the rest of a call whose first trial a chained schedule or the pipelined loop left undecided.
//
// The kernels of a call (all asynchronous on the handle's stream):
//
//   front   [k_obs_residual]                     only when the host replaced the states (no carried keys)
//           [select]                             exact digits (2 passes; 3 when digit 0 is not there yet); on carried keys
//                                                ONE warm pass (k_select_warm) -- or, latency mode, nothing: the keys lie
//                                                in per-bin buckets and the accumulation selects in its prologue.  In a
//                                                chained schedule the kernel that starts the call also evaluates the
//                                                accept test of the call in front (fold)
//           k_obs_accumulate (+ dynamics blocks) median finish, weights, per-pose normal equations [+ orbit / attitude factor]
//           [k_assemble]                         only when something reads the bands from memory: batched windows, sharded
//                                                mode, the sequential / always-pivoting solvers
//   trial   [solve]                              full phase: chunk elimination (forming its own blocks in latency mode),
//                                                cyclic reduction of the separators; landmark-only phase: nothing in
//                                                latency mode (the trial kernel solves its 6x6 systems itself)
//           k_trial                              step + retraction (latency mode) + trial residuals + next call's keys
//   decide  [k_decide]                           own launch unless the next call's first kernel folds it
//
// Latency mode, landmark-only call: 2 kernels (accumulate, trial); full call: 6 (+ assembly, chunks, two
// cyclic-reduction kernels).  Call parity p: input states S[p], trial states S[p ^ 1] (see WinScalars).
#include "vba_context.h"


void view_for_call(vba_handle h, DevView& V, const CallSpec& c) {
    V = h->V;
    V.m_total = 0; V.abs_all = nullptr; V.abs_all_count = 0;
    V.reg = h->reg ? 1 : 0;
    V.n_min = *std::min_element(h->n.begin(), h->n.end());
    V.call = c.call;
    V.par = c.par;
    V.states = h->S[c.par];
    V.wraw = h->wraw2 + (size_t)c.par * h->W * h->V.m_max;
    V.Hraw = h->Hraw2 + (size_t)c.par * h->W * h->n_max * 21;
    V.braw = h->braw2 + (size_t)c.par * h->W * h->n_max * 6;
    {
        const size_t wn = (size_t)c.par * h->W * h->n_max;
        V.xhat = h->dyn2[0] + wn * 6; V.Phi = h->dyn2[1] + wn * 36; V.rorb = h->dyn2[2] + wn * 6; V.fatt = h->dyn2[3] + wn;
        V.qgrad = h->dyn2[4] + wn * 3; V.Hd = h->dyn2[5] + wn * 9; V.Hu = h->dyn2[6] + wn * 9; V.Hl = h->dyn2[7] + wn * 9;
    }
    V.states_new = h->S[c.par ^ 1];
    V.states_prev = h->S[c.par];
    if (!c.host_out) V.host_states = nullptr;
    V.emit = c.emit;
    V.carry = c.carry;
    V.fold = c.fold ? 1 : 0;
    V.sel_inline = 0;
    V.median_ready = 0;
    V.redo = 0;
    V.pending_only = 0;
    V.warm_force_miss = h->warm_enabled == 2;
    V.pivot = h->pivot_mode;
    // sequential driver with several windows: four chains per wavefront (k_solve_quad); vba_set_solver(h, -3) asks for the
    // older three-chain packing (equal pose counts only), -2 for one window per wavefront
    V.pack = 0;
    if (V.chunk <= 0 && !h->no_pack && h->W >= 2) {
        V.pack = 2;
        if (h->W >= h->pack_min) {
            V.pack = 1;
            for (int w = 1; w < h->W; ++w) if (h->n[w] != h->n[0]) V.pack = 2;
        }
    }
    fill_params(V.prm, c.iter, c.initialize);
    // who forms the step: latency mode lets the trial kernel do it (landmark-only: 6x6 solve per pose on the unpivoted
    // path; full phase: recovery of the partitioned solve)
    V.fused_trial = 0;
    if (V.lat && (h->fusion & 1)) {     // every trial kernel of such a handle uses the 16-lanes-per-pose geometry
        if (c.initialize) V.fused_trial = h->pivot_mode == 0 ? 1 : 3;
        else V.fused_trial = V.chunk > 0 ? 2 : 3;
        V.nblk_dyn = (V.n_max - 1 + 14) / 15;
    }
    V.fuse_blocks = (h->fusion & 2) ? 1 : 0;
    V.resident = !V.lat ? 0 : (h->fusion & 64) ? 2 : (h->fusion & 32) ? 1 : 0;
    V.chunk_waves = h->chunk_waves;
    V.asm_rows = (h->fusion & 8) ? 1 : 0;
    V.cr_levels = (h->fusion & 16) ? 1 : h->cr_levels;
    V.fuse_walk = ((h->fusion & 4) && !V.lat) ? 1 : 0;
}

// the kernels in front of the first LM trial; ev (profiled variant): events that bracket the kernel classes
int enqueue_front(vba_handle h, CallCtx& C, const CallSpec& c, bool exact_repeat, hipEvent_t* ev) {
    DevView& V = C.V;
    hipStream_t s = h->stream;
    auto mark = [&](int k) { if (ev && ev[k]) (void)hipEventRecord(ev[k], s); };
    const bool init = c.initialize != 0;
    V.sel_inline = 0;       // (a repeat of the front after a missed warm select takes the exact digits and the plain prologue)
    // the dynamics factor depends only on the states: with few windows its blocks ride in the accumulation's grid (no
    // second stream, no cross-stream join), with many it runs beside the observation kernels on a second stream
    const bool ride = !init && !c.prof && V.lat;
    V.dyn_in_acc = ride ? 1 : 0;
    static const bool no_overlap = std::getenv("VBA_NO_OVERLAP") != nullptr;     // diagnostic: dynamics in line on the main stream
    const bool overlap = !init && !c.prof && !ride && !no_overlap;
    auto fork_dynamics = [&]() -> int {
        HIPCHK(hipEventRecord(h->ev_fork, s));
        HIPCHK(hipStreamWaitEvent(h->aux_stream, h->ev_fork, 0));
        launch_dynamics(V, h->aux_stream);
        HIPCHK(hipEventRecord(h->ev_join, h->aux_stream));
        return VBA_OK;
    };
    // a folding select is what moves the window on to this call (and reads the block sums the previous call's dynamics
    // left): the second stream forks behind it, not in front
    const bool fork_late = overlap && c.fold;
    if (overlap && !fork_late) { if (int rc = fork_dynamics()) return rc; }
    mark(1);
    if (!c.carry) {
        launch_obs_residual(V, nullptr, s);
        mark(2);
        launch_select(V, false, s);
    } else if (c.carry == 2 && !exact_repeat) {
        mark(2);
        // bin buckets (latency mode): the accumulation resolves the histogram and ranks the wanted bin's bucket in its own
        // prologue -- and, in a chained schedule, evaluates the accept test of the call in front there: no select kernel
        V.sel_inline = (V.wbucket && h->inline_select) ? 1 : 0;
        if (!V.sel_inline) launch_select_warm(V, s);
    } else if (c.carry == 1 && !exact_repeat) {     // the trial left digit 0 (exponent histogram) behind: two passes
        mark(2);
        launch_select(V, false, s);
    } else {            // a warm select that missed: the digit-0 slot holds the warm histogram, rebuild it by exponent
        mark(2);
        launch_clear_hist(V, 2, s);
        launch_select(V, true, s);
    }
    if (fork_late) { if (int rc = fork_dynamics()) return rc; }
    V.median_ready = (!V.sel_inline && !V.lat) ? 1 : 0;
    if (V.median_ready) launch_select_finish(V, s);
    mark(3);
    launch_obs_accumulate(V, s);
    if (C.after_first && V.sel_inline) HIPCHK(hipEventRecord(C.after_first, s));
    mark(4);
    if (!init && !overlap && !ride) launch_dynamics(V, s);
    if (overlap) HIPCHK(hipStreamWaitEvent(s, h->ev_join, 0));
    mark(5);
    C.fuse_assemble = init && h->pivot_mode == 0 && V.fused_trial != 1;
    C.assembled = false;
    C.bands_ready = false;
    const bool need_bands = init ? V.fused_trial != 1 : !solve_forms_blocks(V);
    if (need_bands) {
        launch_assemble(V, C.fuse_assemble, s);
        C.assembled = true;
        C.bands_ready = !C.fuse_assemble;
    }
    mark(6);
    return VBA_OK;
}

// one LM trial: solve (unless the trial kernel or the assembly formed the step) + trial residuals; ev_solve (profiled
// variant): recorded between the two
void enqueue_trial(vba_handle h, CallCtx& C, const CallSpec& c, bool first, hipEvent_t ev_solve, int solve_redo) {
    DevView& V = C.V;
    hipStream_t s = h->stream;
    const bool init = c.initialize != 0;
    const int redo_all = V.redo;
    const bool pivoted_round = V.pivot != 0;
    // landmark-only phase: does a solve kernel run, i.e. does anything read the diagonal blocks from memory?  Not in the
    // first trial when the trial kernel or the fused assembly formed the step -- unless some window fell back to the
    // pivoted kernels
    const bool init_solve = init && (V.fused_trial == 1 ? pivoted_round : !(first && C.fuse_assemble));
    if (init_solve && !C.bands_ready) {
        launch_assemble(V, 0, s);
        C.assembled = C.bands_ready = true;
    }
    if (solve_redo >= 0) V.redo = solve_redo;       // which windows the solve kernels of this round take (see step_impl)
    if (init) {
        if (init_solve) launch_solve(V, 1, s);
    } else {
        launch_solve(V, 0, s);
    }
    V.redo = redo_all;
    if (ev_solve) (void)hipEventRecord(ev_solve, s);
    launch_trial(V, s);
}

void clear_abandoned_hists(vba_handle h, const DevView& V, hipStream_t s) {
    if (!h->need_hist_reset) return;
    DevView Q = V;
    for (int p = 0; p < 2; ++p) { Q.par = p; launch_clear_hist(Q, 1, s); }
    h->need_hist_reset = false;
    h->hist_dirty = false;
}

// readback >= 0: the states and scalars of that window are copied to the pinned read-back buffer right behind the first
// trial (valid if that trial ends the call: h->back_valid), so that vba_iterate needs one wait instead of two.
int step_impl(vba_handle h, int iter, int initialize, float* prof, bool emit, int readback) {
    if (!h) return fail(VBA_EINVAL, "null handle");
    if (int rc_settle = settle(h)) return rc_settle;
    if (int rc = ready(h)) return rc;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    CallSpec c;
    c.iter = iter; c.initialize = initialize; c.call = -1; c.par = h->par;
    const int emit_kind = h->warm_enabled ? 2 : 1;
    c.emit = (h->carry_enabled && emit) ? emit_kind : 0;
    c.carry = h->carry_enabled ? h->carry_ok : 0;
    c.prof = prof != nullptr;
    h->carry_ok = 0;
    h->shc.carried = false;         // (an unsharded call on a sharded handle: the gathered exchange of the last sharded trial is stale)
    CallCtx C;
    view_for_call(h, C.V, c);
    DevView& V = C.V;
    clear_abandoned_hists(h, V, s);
    if (!c.carry && h->hist_dirty) launch_clear_hist(V, 0, s);     // the states were replaced after the last trial
    h->hist_dirty = c.emit != 0;
    struct ProfEvents {         // destroyed on every exit path, error returns included
        hipEvent_t e[VBA_NKERNELS + 1] = {};
        ~ProfEvents() { for (hipEvent_t q : e) if (q) (void)hipEventDestroy(q); }
    } pe;
    hipEvent_t* ev = pe.e;
    if (prof) {
        for (int k = 0; k <= VBA_NKERNELS; ++k) HIPCHK(hipEventCreate(&ev[k]));
    }
    auto mark = [&](int k) { if (prof) (void)hipEventRecord(ev[k], s); };
    CallAbandon abandon{h};
    HIPCHK(hipEventRecord(h->ev0, s));
    mark(0);
    if (int rc = enqueue_front(h, C, c, false, prof ? ev : nullptr)) return rc;
    // LM loop (BA_filtering.py:52-77): lamda runs 1e-4 .. 1e4 in decades (at most 9 trials), plus one repeat per window for a
    // pivoted fallback and one for a missed warm select; a loop that is still not done after kMaxTrials means the device
    // never reported an outcome (a fault, a skipped window)
    constexpr int kMaxTrials = 24;
    bool finished = false, first = true;
    int solve_redo = -1;
    for (int trial = 0; trial < kMaxTrials; ++trial) {
        enqueue_trial(h, C, c, first, (first && prof) ? ev[7] : nullptr, solve_redo);
        solve_redo = -1;
        if (first) mark(8);
        launch_decide(V, nullptr, 0, s);
        if (first) {
            mark(9);
            HIPCHK(hipEventRecord(h->ev1, s));
        }
        h->back_valid = false;
        if (readback >= 0) {    // the trial states ARE the result if this trial ends the call
            HIPCHK(hipMemcpyAsync(h->h_back, V.states_new + (size_t)readback * h->n_max * 10, (size_t)h->n[readback] * 80, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(h->h_back + (size_t)h->n_max * 10, V.sc + readback, sizeof(WinScalars), hipMemcpyDeviceToHost, s));
        }
        HIPCHK(hipGetLastError());
        if (int rc = read_heads(h)) return rc;
        first = false;
        bool all = true, repeat = false, miss = false;
        for (int w = 0; w < h->W; ++w) {
            all = all && head(h, w)->done;
            repeat = repeat || (head(h, w)->flags & 8u);
            miss = miss || (head(h, w)->flags & 32u);
        }
        if (miss) {     // the warm select missed for some window: those repeat the call's front with the exact digits
            for (int w = 0; w < h->W; ++w) if (head(h, w)->flags & 32u) h->h_head[w].flags = 0;
            h->warm_misses++;
            V.redo = 1;
            CallSpec cr = c;
            cr.prof = false;
            if (int rc = enqueue_front(h, C, cr, true, nullptr)) return rc;
            V.redo = 2;             // this round: their first trial, the others' next one
            // ... whose solve the repeating windows skip when the assembly they just ran has formed their first step already
            solve_redo = (c.initialize && C.fuse_assemble) ? 0 : 2;
            continue;
        }
        V.redo = 0;
        if (repeat && V.pivot == 0) {   // a pivot check failed on the fast path: those windows repeat the trial with row pivoting
            V.pivot = 2;
            h->fallbacks++;
            continue;
        }
        if (all) {
            h->back_valid = readback >= 0;      // the copies queued behind this (final) trial hold the result
            finished = true;
            break;
        }
    }
    if (!finished)
        return fail(VBA_ESTATE, "LM loop did not terminate within " + std::to_string(kMaxTrials) + " trials (no outcome reported by the device)");
    abandon.armed = false;
    HIPCHK(hipEventElapsedTime(&h->last_ms, h->ev0, h->ev1));
    if (prof) {
        for (int k = 0; k < VBA_NKERNELS; ++k) {
            prof[k] = 0.f;
            (void)hipEventElapsedTime(&prof[k], ev[k], ev[k + 1]);
        }
        if (c.carry) prof[VBA_K_RESIDUAL] = 0.f;        // not launched: the previous trial left the keys behind
        if (c.initialize && (C.fuse_assemble || V.fused_trial == 1)) prof[VBA_K_SOLVE] = 0.f;   // no solve launch: formed inside k_assemble<true> / k_trial
        if (!C.assembled) prof[VBA_K_ASSEMBLE] = 0.f;
        if (c.initialize) prof[VBA_K_DYNAMICS] = 0.f;
    }
    h->par ^= 1;                    // the trial buffer is the next call's input
    h->carry_ok = c.emit;           // (the kind of histogram that came with the keys)
    h->stepped = true;
    h->last_pipelined = false;
    h->prev_res_iter = -1;          // (not a link of the resident loop: nothing to learn from what follows it)
    h->last_iter = iter;
    h->last_init = initialize;
    return VBA_OK;
}

int vba_step(vba_handle h, int iter, int initialize) { return step_impl(h, iter, initialize, nullptr); }

int vba_step_profiled(vba_handle h, int iter, int initialize, float* ms) {
    if (!ms) return fail(VBA_EINVAL, "null ms");
    return step_impl(h, iter, initialize, ms);
}

// The first trial of call q.call has been evaluated for the windows that stand at it (stall_at[w] == q.call) but was not
// cleanly accepted by the kernel that was to start the next call (or the call's warm select missed): finish the call the
// ordinary way -- decide, repeat the front with the exact digits where the select missed, further LM trials, the pivoted
// repeat -- until every such window has moved on.  Shared by vba_run_schedule and the pipelined vba_iterate_resident.
int finish_stalled_call(vba_handle h, const CallSpec& q, const std::vector<int>& stall_at, long& trials) {
    hipStream_t s = h->stream;
    const int sc_call = q.call;
    static const bool trace = std::getenv("VBA_TRACE") != nullptr;
    CallCtx C;
    view_for_call(h, C.V, q);
    DevView& V = C.V;
    // the front of this call has run (for the windows that reached it); what is on the device of it:
    C.fuse_assemble = q.initialize && h->pivot_mode == 0 && V.fused_trial != 1;
    C.assembled = q.initialize ? V.fused_trial != 1 : !solve_forms_blocks(V);
    C.bands_ready = C.assembled && !C.fuse_assemble;
    auto at_call = [&](int w) { return stall_at[w] == sc_call && head(h, w)->call_idx == sc_call; };
    bool any_miss = false;
    for (int w = 0; w < h->W; ++w) any_miss = any_miss || (at_call(w) && (head(h, w)->flags & 32u));
    // (1) the first trial of the windows that got that far has been evaluated but not decided (the decision was left
    //     to the next call's first kernel, which found it not clean): decide it now
    V.pending_only = 1;
    launch_decide(V, nullptr, 0, s);
    V.pending_only = 0;
    // (2) windows whose warm select missed repeat the front with the exact digits and run their first trial
    if (any_miss) {
        for (int w = 0; w < h->W; ++w) if (at_call(w) && (head(h, w)->flags & 32u)) h->h_head[w].flags = 0;
        h->warm_misses++;
        V.redo = 1;
        if (int rc = enqueue_front(h, C, q, true, nullptr)) return rc;
        enqueue_trial(h, C, q, true);
        launch_decide(V, nullptr, 0, s);
        V.redo = 0;
        ++trials;
    }
    HIPCHK(hipGetLastError());
    if (int rc = read_heads(h)) return rc;
    bool finished = false;
    for (int trial = 0; trial <= 24; ++trial) {
        bool repeat = false, all = true;
        for (int w = 0; w < h->W; ++w) {
            if (!at_call(w)) continue;
            all = false;
            repeat = repeat || (head(h, w)->flags & 8u);
        }
        if (all) { finished = true; break; }
        if (trial == 24) break;
        if (repeat && V.pivot == 0) { V.pivot = 2; h->fallbacks++; }
        enqueue_trial(h, C, q, false);
        launch_decide(V, nullptr, 0, s);
        HIPCHK(hipGetLastError());
        if (int rc = read_heads(h)) return rc;
        ++trials;
        if (trace) {
            std::fprintf(stderr, "[vba]   call %d round %d pivot %d:", sc_call, trial, V.pivot);
            for (int w = 0; w < h->W && w < 8; ++w)
                std::fprintf(stderr, " w%d(call %d done %d flags %u ntr %d lam %g)", w, head(h, w)->call_idx, head(h, w)->done, head(h, w)->flags, head(h, w)->n_trials, head(h, w)->lamda);
            std::fprintf(stderr, "\n");
        }
    }
    if (!finished)
        return fail(VBA_ESTATE, "LM loop of call " + std::to_string(sc_call) + " did not terminate (no outcome reported by the device)");
    return VBA_OK;
}
