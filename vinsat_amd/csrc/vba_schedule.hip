// vba_schedule.hip -- the calls of a driver loop chained on the device: vba_run_schedule (the 20-call loop as one host call), the
// cache of the graphs that replay its first pass, and the chain profile.
#include "vba_context.h"


// ---------------------------------------------------------------------------------------------- the graph cache (GraphCache, vba_context.h)
size_t GraphCache::find_ident() const {
    for (size_t k = 0; k < entries.size(); ++k)
        if (entries[k].ident == ident) return k;
    return npos;
}

size_t GraphCache::find_views(const std::vector<unsigned long long>& key, const std::vector<unsigned char>& views) {
    for (size_t k = 0; k < entries.size(); ++k)
        if (entries[k].key == key && entries[k].views == views) { entries[k].ident = ident; return k; }
    return npos;
}

hipGraphExec_t GraphCache::use(size_t k) {
    if (k != 0) std::rotate(entries.begin(), entries.begin() + k, entries.begin() + k + 1);     // most recently used first
    return entries[0].exec;
}

// a graph that was captured under `ident` and has been launched once
int GraphCache::store(const std::vector<unsigned long long>& key, std::vector<unsigned char>&& views, hipGraphExec_t exec, hipStream_t s) {
    if (entries.size() >= kCapacity) {
        // (the evicted graph may still be executing: the stream is idle here only if the caller made it so -- wait)
        HIPCHK(hipStreamSynchronize(s));
        (void)hipGraphExecDestroy(entries.back().exec);
        entries.pop_back();
    }
    entries.insert(entries.begin(), Entry{key, ident, std::move(views), exec});
    captures++;
    return VBA_OK;
}

void GraphCache::destroy() { for (auto& e : entries) if (e.exec) (void)hipGraphExecDestroy(e.exec); }

int vba_set_schedule_graph(vba_handle h, int on) {
    if (!h) return fail(VBA_EINVAL, "null handle");
    if (int rc = settle(h)) return rc;
    h->touch();
    h->graph_enabled = on != 0;
    return VBA_OK;
}

int vba_schedule_graph_stats(vba_handle h, int* captures, int* replays) {
    if (!h) return fail(VBA_EINVAL, "null handle");
    if (captures) *captures = (int)h->gcache.captures;
    if (replays) *replays = (int)h->gcache.replays;
    return VBA_OK;
}

// ---------------------------------------------------------------------------------------------- the chain profile
int vba_set_chain_profile(vba_handle h, int on) {
    if (!h) return fail(VBA_EINVAL, "null handle");
    if (int rc = settle(h)) return rc;
    h->touch();
    h->cprof.on = on != 0;
    return VBA_OK;
}

int vba_chain_profile(vba_handle h, double* ms, int64_t* launches, int reset) {
    if (!h) return fail(VBA_EINVAL, "null handle");
    for (int k = 0; k < 3; ++k) {
        if (ms) ms[k] = h->cprof.ms[k];
        if (launches) launches[k] = h->cprof.launches[k];
        if (reset) { h->cprof.ms[k] = 0.0; h->cprof.launches[k] = 0; }
    }
    return VBA_OK;
}

// the four events of each of ncalls calls exist (kept with the handle)
static int chain_profile_events(vba_handle h, int ncalls) {
    while ((int)h->cprof.ev.size() < 4 * ncalls) {
        hipEvent_t e = nullptr;
        HIPCHK(hipEventCreate(&e));
        h->cprof.ev.push_back(e);
    }
    return VBA_OK;
}

// every call of the profiled pass ran once, in order: its three intervals count
static void chain_profile_account(vba_handle h, int ncalls, const int* inits) {
    for (int c = 0; c < ncalls; ++c) {
        const hipEvent_t* pe = h->cprof.ev.data() + (size_t)4 * c;
        for (int k = 0; k < 3; ++k) {
            float ms = 0.f;
            if (k == 1 && inits[c]) continue;       // landmark-only call: the step is formed in front of or inside the trial kernel, no solve launch
            if (hipEventElapsedTime(&ms, pe[k], pe[k + 1]) == hipSuccess) {
                h->cprof.ms[k] += ms;
                h->cprof.launches[k]++;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- the chained schedule
namespace {
// One vba_run_schedule: the calls it was given and the state of the handle it starts from -- what every pass of it is made of.
struct Sched {
    vba_handle h;
    int ncalls;
    const int *iters, *inits;
    int par0 = 0, carry0 = 0, emit_kind = 0;
    int clear0 = 0, up_n10 = 0;         // what the entry kernel does beside resetting the call counters (see vba_run_schedule)

    CallSpec spec(int c, bool fold) const {
        CallSpec q;
        q.iter = iters[c]; q.initialize = inits[c]; q.call = c; q.par = (par0 + c) & 1;
        q.carry = c == 0 ? carry0 : emit_kind;              // every later call starts from a trial of this chain
        q.emit = emit_kind;
        q.fold = fold;
        return q;
    }
    // Call c of a pass that starts at call `first` folds the accept test of call c - 1: that call leaves its decision to this call's
    // warm select and no decide launch behind.  Not the first call of the pass -- the pass in front and the host's LM loop have
    // decided call first - 1 -- and only on warm-histogram keys.
    bool folds(int c, int first) const { return c > first && emit_kind == 2 && h->fold_enabled; }
    // ... and the view its kernels take
    CallSpec call(DevView& V, int c, int first) const {
        const CallSpec q = spec(c, folds(c, first));
        view_for_call(h, V, q);
        if (q.fold) fill_params(V.prev, iters[c - 1], inits[c - 1]);
        return q;
    }
};

// The calls first .. ncalls - 1, one LM trial each (speculative: a window whose trial is not cleanly accepted sits out the rest).
// profiled (chain profile, first pass only): events in front of / behind the accumulation (what runs in front of it -- select
// kernels of the bandwidth mode -- counts as accumulate class: the first event is moved there), behind the solve and behind the trial
static int enqueue_pass(const Sched& S, int first, bool profiled) {
    vba_handle h = S.h;
    hipStream_t s = h->stream;
    if (first == 0) {       // the entry kernel: only in front of call 0 (a re-issue from a later call finds the states moved on)
        DevView V0;
        view_for_call(h, V0, S.spec(0, false));
        launch_reset_calls(V0, s, S.up_n10 ? h->d_stage_map : nullptr, S.up_n10, S.clear0);
    }
    for (int c = first; c < S.ncalls; ++c) {
        CallCtx C;
        const CallSpec q = S.call(C.V, c, first);
        hipEvent_t marks[VBA_NKERNELS + 1] = {};
        hipEvent_t* pe = nullptr;
        if (profiled) {
            pe = h->cprof.ev.data() + (size_t)4 * c;
            marks[1] = pe[0];
            marks[6] = pe[1];
        }
        if (int rc = enqueue_front(h, C, q, false, pe ? marks : nullptr)) return rc;
        enqueue_trial(h, C, q, true, pe ? pe[2] : nullptr);
        if (pe) HIPCHK(hipEventRecord(pe[3], s));
        const bool next_folds = c + 1 < S.ncalls && S.folds(c + 1, first);
        if (!next_folds) launch_decide(C.V, nullptr, 0, s);
    }
    return VBA_OK;
}

// The identity of a first pass: the handle's generation (everything a view or an enqueue function reads that is not listed
// here: vba_context::gen) and what this call brings along.  A cached graph whose views were compared byte for byte under
// this identity would compare equal again -- nothing they are made from has changed -- so it is replayed without building them.
static void pass_identity(const Sched& S, hipStream_t s, std::vector<unsigned long long>& ident) {
    ident.clear();
    ident.push_back(S.h->gen); ident.push_back((unsigned long long)S.ncalls); ident.push_back((unsigned long long)S.par0);
    ident.push_back((unsigned long long)S.carry0); ident.push_back((unsigned long long)S.emit_kind); ident.push_back((unsigned long long)(uintptr_t)s);
    ident.push_back((unsigned long long)S.clear0); ident.push_back((unsigned long long)S.up_n10);
    for (int c = 0; c < S.ncalls; ++c) ident.push_back(((unsigned long long)(unsigned)S.iters[c] << 1) | (S.inits[c] ? 1ull : 0ull));
}

// What goes into the launches of a first pass: the views of its calls (every kernel takes its DevView by value) byte for byte, a
// hash of each for the quick reject, the schedule, and the handful of host-side switches the enqueue functions read.  The views
// are those of enqueue_pass(S, 0, ...): a pass is captured -- and replayed -- only from call 0 (vba_run_schedule tries the graph
// with next == 0 alone), so first = 0 is the only value the fold predicate ever takes inside a graph.
static void pass_key_views(const Sched& S, hipStream_t s, std::vector<unsigned long long>& key, std::vector<unsigned char>& views) {
    vba_handle h = S.h;
    key.reserve(9 + 3 * (size_t)S.ncalls);
    views.resize((size_t)S.ncalls * sizeof(DevView));
    key.push_back((unsigned long long)S.ncalls); key.push_back((unsigned long long)S.par0); key.push_back((unsigned long long)S.carry0);
    key.push_back((unsigned long long)S.emit_kind); key.push_back((unsigned long long)h->pivot_mode);
    key.push_back((unsigned long long)h->inline_select | ((unsigned long long)h->fold_enabled << 1));
    key.push_back((unsigned long long)(uintptr_t)s);
    key.push_back((unsigned long long)S.clear0 | ((unsigned long long)S.up_n10 << 1));
    for (int c = 0; c < S.ncalls; ++c) {
        DevView Vc;
        S.call(Vc, c, 0);
        unsigned long long hsh = 1469598103934665603ull;
        const unsigned char* bytes = reinterpret_cast<const unsigned char*>(&Vc);
        std::memcpy(views.data() + (size_t)c * sizeof(DevView), bytes, sizeof(DevView));
        for (size_t o = 0; o + 8 <= sizeof(DevView); o += 8) {
            unsigned long long wd;
            std::memcpy(&wd, bytes + o, 8);
            hsh = (hsh ^ wd) * 1099511628211ull;
            hsh ^= hsh >> 29;
        }
        key.push_back(hsh); key.push_back((unsigned long long)S.iters[c]); key.push_back((unsigned long long)S.inits[c]);
    }
}

struct CaptureGuard {       // (an early return between begin and end must not leave the stream capturing)
    hipStream_t s; bool on = false;
    ~CaptureGuard() {
        if (on) {
            hipGraph_t g = nullptr;
            (void)hipStreamEndCapture(s, &g);
            if (g) (void)hipGraphDestroy(g);
            (void)hipGetLastError();
        }
    }
};

// The first pass of a latency-mode handle -- ~70 dependent launches for the driver's 20 calls -- is captured once as a hipGraph and
// replayed while nothing that goes into its launches has changed: 45.2 -> 42.7 us per call at C3 (the packets of a graph reach the
// queue in one piece; launched one by one every kernel boundary also pays the runtime's per-launch bookkeeping on the device's
// clock).  Stalled calls are finished by the host afterwards exactly as without a graph.
// Here: replay the graph the handle has for this pass (found by identity; failing that by key and views, which are left in key /
// views) or begin to capture one.  Neither `replayed` nor cap.on: the handle has given up on graphs.
static void try_graph(const Sched& S, CaptureGuard& cap, std::vector<unsigned long long>& key, std::vector<unsigned char>& views, bool& replayed) {
    GraphCache& G = S.h->gcache;
    pass_identity(S, cap.s, G.ident);
    size_t hit = G.find_ident();
    if (hit == GraphCache::npos) {      // slow path: the views themselves
        pass_key_views(S, cap.s, key, views);
        hit = G.find_views(key, views);
    }
    if (hit != GraphCache::npos) {
        const hipGraphExec_t exec = G.use(hit);
        VBA_ESTAMP(4);
        const hipError_t launched = hipGraphLaunch(exec, cap.s);
        VBA_ESTAMP(5);
        if (launched == hipSuccess) { replayed = true; G.replays++; }
        else { (void)hipGetLastError(); G.broken = true; }
    } else if (hipStreamBeginCapture(cap.s, hipStreamCaptureModeRelaxed) == hipSuccess) {
        cap.on = true;
    } else { (void)hipGetLastError(); G.broken = true; }
}

// End the capture try_graph began: instantiate the graph, launch it, keep it.  A capture that cannot be ended, instantiated or
// launched has executed NOTHING (its kernels were only recorded): the handle gives up on graphs (broken: kernel by kernel from
// then on) and the pass is enqueued again, for real.  VBA_GRAPH_FAIL_INJECT = 1 / 2 / 3 pretends that step failed
// (tests/test_gpu_bench_paths.py).
static int end_capture(const Sched& S, CaptureGuard& cap, const std::vector<unsigned long long>& key, std::vector<unsigned char>& views) {
    static const int inject = std::getenv("VBA_GRAPH_FAIL_INJECT") ? std::atoi(std::getenv("VBA_GRAPH_FAIL_INJECT")) : 0;
    hipGraph_t g = nullptr;
    cap.on = false;
    hipGraphExec_t exec = nullptr;
    bool ok = hipStreamEndCapture(cap.s, &g) == hipSuccess && g != nullptr && inject != 1;
    if (ok) ok = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0) == hipSuccess && inject != 2;
    if (g) (void)hipGraphDestroy(g);
    if (ok && (inject == 3 || hipGraphLaunch(exec, cap.s) != hipSuccess)) ok = false;
    if (ok) return S.h->gcache.store(key, std::move(views), exec, cap.s);
    (void)hipGetLastError();
    if (exec) (void)hipGraphExecDestroy(exec);
    S.h->gcache.broken = true;
    return enqueue_pass(S, 0, false);       // (what was captured: the unprofiled pass from call 0)
}

// After a pass over calls next .. ncalls-1 every window whose counter is below ncalls is stalled AT that call.  Returns those
// calls in ascending order, and in stall_at[w] where window w stands.
static std::vector<int> stalled_calls(vba_handle h, int ncalls, std::vector<int>& stall_at) {
    std::vector<int> stalled;
    stall_at.resize((size_t)h->W);
    for (int w = 0; w < h->W; ++w) {
        const int c = (int)head(h, w)->call_idx;
        stall_at[w] = c;        // a window that finish_stalled_call moves on INTO a later stalled call has not run that call's front: it waits for the re-issue
        if (c < ncalls && std::find(stalled.begin(), stalled.end(), c) == stalled.end()) stalled.push_back(c);
    }
    std::sort(stalled.begin(), stalled.end());
    return stalled;
}

static void trace_pass(vba_handle h, int next) {
    static const bool trace = std::getenv("VBA_TRACE") != nullptr;
    if (!trace) return;
    std::fprintf(stderr, "[vba] pass from call %d:", next);
    for (int w = 0; w < h->W && w < 8; ++w)
        std::fprintf(stderr, " w%d(call %d done %d flags %u ntr %d)", w, head(h, w)->call_idx, head(h, w)->done, head(h, w)->flags, head(h, w)->n_trials);
    std::fprintf(stderr, "\n");
}
}   // namespace

// The 20-call loop of the driver (od_pipe.py:1036-1040) as ONE host call.  The kernels of every call are enqueued
// back to back with a single LM trial each and, on carried keys, without a decide launch between them: the first kernel
// of call c + 1 evaluates the accept test of call c itself.  A window whose first trial is not cleanly accepted (rejected,
// pivot check failed) or whose warm select misses does not advance its device-side call counter, all later kernels skip
// it, and the host finishes that call the ordinary way before re-enqueuing the rest.  Results are identical to ncalls
// vba_step calls.
int vba_run_schedule(vba_handle h, int ncalls, const int* iters, const int* inits, int* trials_total) {
    if (!h || !iters || !inits || ncalls < 1) return fail(VBA_EINVAL, "bad argument");
    VBA_ESTAMP(3);
    if (int rc_settle = settle(h, false, true)) return rc_settle;       // (staged states stay staged: the entry kernel takes them)
    if (int rc = ready(h)) return rc;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    Sched S{h, ncalls, iters, inits};
    S.par0 = h->par;
    S.emit_kind = h->carry_enabled ? (h->warm_enabled ? 2 : 1) : 0;
    S.carry0 = h->carry_enabled ? h->carry_ok : 0;
    h->carry_ok = 0;
    h->shc.carried = false;
    CallAbandon abandon{h};
    if (h->need_hist_reset) {
        DevView Q;
        view_for_call(h, Q, S.spec(0, false));
        clear_abandoned_hists(h, Q, s);
    }
    // What the entry kernel of the pass (k_reset_calls, the first launch of enqueue_pass) does beside resetting the call counters:
    // clear the digit-0 histogram that the exact select of call 0 fills (a trial whose states were then replaced may have left a
    // warm histogram there; cleared whenever call 0 starts without carried keys, dirty or not, so that one graph serves both), and
    // take the states vba_set_states staged.  Both change what is launched: part of the key and of the identity of a cached graph.
    S.clear0 = S.carry0 ? 0 : 1;
    if (h->pend.on && h->pend.par != S.par0) { if (int rc = flush_states(h)) return rc; }   // (cannot happen: the parity moves only with a call)
    S.up_n10 = h->pend.on ? h->pend.n * 10 : 0;
    if (h->pend.on) { h->pend.on = false; h->stage_kernel = true; }     // from here on the staged states belong to this schedule
    h->hist_dirty = S.emit_kind != 0;
    for (int w = 0; w < h->W; ++w) { h->h_head[w].call_idx = 0; h->h_head[w].done = 0; h->h_head[w].flags = 0; }
    long trials = 0;
    int next = 0;
    bool complete = false;
    const bool prof_pass = h->cprof.on;
    if (prof_pass) { if (int rc = chain_profile_events(h, ncalls)) return rc; }
    static const bool no_graph = std::getenv("VBA_NO_GRAPH") != nullptr;        // launches kernel by kernel (comparison)
    for (int guard = 0; guard <= ncalls; ++guard) {
        // The first pass goes through a graph (try_graph) -- on latency-mode handles only: with the second stream of the bandwidth mode
        // forked inside it the replay measured 1 .. 2.5 % SLOWER than the launches one by one, 40 .. 1024 windows
        // (... and not while the chain profile records its events: event records inside a capture fail on this runtime, "invalid resource
        // handle" -- the class times of vba_chain_profile are those of the kernel-by-kernel launches)
        // (... nor with the resident solve of the comparison build, vba_set_fusion bits 5 / 6: its kernels take the epoch of the launch as
        // an argument, which a replay would freeze -- the consumers' flags would read as already set)
        const bool graph = !no_graph && h->graph_enabled && guard == 0 && !prof_pass && h->V.lat && !h->gcache.broken && next == 0 && (h->fusion & 96) == 0;
        bool replayed = false;
        std::vector<unsigned long long> gkey;
        std::vector<unsigned char> gviews;
        CaptureGuard capture{s};
        if (graph) try_graph(S, capture, gkey, gviews, replayed);
        if (!replayed) { if (int rc = enqueue_pass(S, next, prof_pass && guard == 0)) return rc; }
        if (capture.on) { if (int rc = end_capture(S, capture, gkey, gviews)) return rc; }
        HIPCHK(hipGetLastError());
        if (int rc = read_heads(h)) return rc;
        h->stage_kernel = false;        // (the entry kernel has read the staged states)
        trials += (long)(ncalls - next);
        // Every stalled call is finished with the ordinary LM loop -- each one, not only the earliest: a window left at a
        // later call would otherwise run that call again from its start when the chain is re-issued.
        std::vector<int> stall_at;
        const std::vector<int> stalled = stalled_calls(h, ncalls, stall_at);
        if (prof_pass && guard == 0 && stalled.empty()) chain_profile_account(h, ncalls, inits);
        if (stalled.empty()) { complete = true; break; }
        trace_pass(h, next);
        for (int sc_call : stalled) {
            if (int rc = finish_stalled_call(h, S.spec(sc_call, false), stall_at, trials)) return rc;
        }
        next = stalled.front() + 1;
        if (next >= ncalls) { complete = true; break; }
    }
    if (!complete) {
        complete = true;
        for (int w = 0; w < h->W; ++w) complete = complete && head(h, w)->call_idx >= ncalls;
        if (!complete) return fail(VBA_ESTATE, "chained schedule did not complete (a window never reached its last call)");
    }
    abandon.armed = false;
    if (trials_total) *trials_total = (int)trials;
    h->par = (S.par0 + ncalls) & 1;
    h->carry_ok = S.emit_kind;
    h->stepped = true;
    h->last_pipelined = false;
    h->last_iter = iters[ncalls - 1];
    h->last_init = inits[ncalls - 1];
    return VBA_OK;
}
