// vba_context.h -- the host side of libvinsat_ba.so shared by its translation units: the context behind a vba_handle, error
// reporting, and the functions one file defines and another calls.
//   vba_api.hip          error reporting, settle / ready / read_heads, version and mode getters
//   vba_handle.hip       vba_create*, vba_destroy: mode defaults, the device arena and its layout, host resources
//   vba_options.hip      vba_set_option and the other setters, the counters beside them
//   vba_upload.hip       observations, pose constants, priors and states up; states back
//   vba_debug.hip        vba_debug_fetch
//   vba_call.hip         the kernels of one BA() call as the host enqueues them: vba_step, the rest of a stalled call
//   vba_schedule.hip     vba_run_schedule (chained calls), the graph cache that replays its first pass, the chain profile
//   vba_iterate.hip      vba_iterate* (states over PCIe, the pipelined driver loop, host watch)
//   vba_sharded_api.hip  observation-sharded mode (vba_sh_*)
//   vba_query.hip        the scaffold of the queries at the resident states: checks, scratch, timing, the shadow front they share
//   vba_cov.hip          per-pose marginal covariances (vba_covariance): the selected inversion behind that front
//   vba_rel.hip          per-row leverages and w-tests (vba_reliability)
//   vba_power.hip        per-row detectable biases and influences, the fit's variance factor (vba_outlier_power)
//   vba_snoop.hip        data snooping: rows rejected by their w-test on the device (vba_snoop, vba_snoop_scaled)
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include <dlfcn.h>
#include <unistd.h>
#include <rccl/rccl.h>      // types only: the library is resolved at run time (vba_sh_comm_init), never linked

#include "../../include/vinsat_ba.h"
#include "vba_device.h"
#include "vba_launch.h"
#include "vba_query_layout.h"

using namespace vba;

// (everything below is internal to the library: hidden, so that names such as fail / ready / head never meet a host program's)
#pragma GCC visibility push(hidden)
extern thread_local std::string g_err;
int fail(int code, const std::string& msg);
#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return fail(VBA_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));                  \
    } while (0)

// -DVBA_ENTRY_STAMPS (diagnostic build, tools/schedule_gap.py): host wall-clock stamps around the entry of a chained schedule.  Six
// points form a cycle -- 0 the wait of read_heads has returned, 1 / 2 entry / exit of vba_set_states, 3 entry of vba_run_schedule,
// 4 / 5 just before / after the launch of the pass's graph -- and interval k (from point k - 1 to point k) is summed whenever the
// two points were passed one after the other; vba_debug_fetch(what = 103) returns {count, sum in ns} per interval and clears them.
#ifdef VBA_ENTRY_STAMPS
struct EntryStamps { int last = -1; double t_last = 0.0; double sum[6] = {}; double cnt[6] = {}; };
extern EntryStamps g_estamps;
inline void entry_stamp(int k) {
    const double now = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now().time_since_epoch()).count();
    EntryStamps& E = g_estamps;
    if (E.last == (k + 5) % 6) { E.sum[k] += now - E.t_last; E.cnt[k] += 1.0; }
    E.last = k;
    E.t_last = now;
}
#define VBA_ESTAMP(k) entry_stamp(k)
#else
#define VBA_ESTAMP(k) ((void)0)
#endif

// What each uncertainty query keeps in the handle: its device scratch (grown on demand, never shrunk), the event behind its last
// kernel, and the device time of its last call.
struct QueryScratch {
    void* d = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
    float ms = 0.f;
    bool ran = false;
};

// The first passes of the last few chained schedules as graphs (vba_run_schedule), each with what it was made for; most recently
// used first, at most kCapacity of them (a driver alternates between a handful of schedules: the 20-call loop, its two phases).
//   key    a hash per call's view (the quick reject)
//   views  the bytes of those views, compared exactly on a key match (a 64-bit hash collision would replay another schedule's
//          launches silently; ncalls x sizeof(DevView) of memcmp is ~1 us)
//   ident  what the handle looked like when key and views were last found equal (pass_identity in vba_schedule.hip) -- a schedule
//          that finds it unchanged replays without building a single view
// Defined in vba_schedule.hip.
struct GraphCache {
    static constexpr size_t kCapacity = 8;
    static constexpr size_t npos = ~size_t(0);
    struct Entry { std::vector<unsigned long long> key, ident; std::vector<unsigned char> views; hipGraphExec_t exec = nullptr; };
    std::vector<Entry> entries;
    std::vector<unsigned long long> ident;      // identity of the pass being looked up (scratch, reused: a replay allocates nothing)
    bool broken = false;                        // capture or launch failed once: kernel by kernel from then on
    long captures = 0, replays = 0;
    size_t find_ident() const;                  // the entry made for `ident`, or npos
    size_t find_views(const std::vector<unsigned long long>& key, const std::vector<unsigned char>& views);    // ... for these views: a hit adopts `ident`
    hipGraphExec_t use(size_t k);               // entry k moves to the front
    // a new first entry for `ident`; a full cache drops its last one (once the stream s, where it may still execute, is idle)
    int store(const std::vector<unsigned long long>& key, std::vector<unsigned char>&& views, hipGraphExec_t exec, hipStream_t s);
    void destroy();                             // the graphs themselves (vba_destroy)
};

struct vba_context {
    int device = 0;
    int W = 0, n_max = 0;
    int64_t m_max = 0;
    hipStream_t own_stream = nullptr, stream = nullptr, aux_stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_fork = nullptr, ev_join = nullptr;
    char* arena = nullptr;                  // one device allocation behind every buffer of V (arena_layout, vba_handle.hip)
    DevView V{};
    // mutable device pointers (DevView holds const views of some)
    int *d_n = nullptr, *d_m = nullptr, *d_steps = nullptr;
    int *d_long_idx = nullptr, *d_n_long = nullptr, *d_long_off = nullptr;     // long edges of every window (vba_long.hip)
    std::vector<int> n_long;                // ... and how many each window has (host copy; DevView::nblk_long is their maximum)
    // per-observation weights and per-pose normal equations exist per call parity (DevView points at the slot of the call):
    // the accumulation of call c + 1 starts before the accept test of call c is known, whose later trials still read them
    double *wraw2 = nullptr, *Hraw2 = nullptr, *braw2 = nullptr;
    double* dyn2[8] = {};           // xhat, Phi, rorb, fatt, qgrad, Hd, Hu, Hl
    double* d_obs = nullptr;                // observation blocks, [W][obs_stride] (layout: DevView::ox)
    int64_t m_pad = 0;                      // doubles per observation array inside a block
    double *d_intr = nullptr, *d_cumrot = nullptr;
    // uploads go through pinned staging and are asynchronous on the handle's stream (ordered with the kernels that
    // read them); two buffers, so that the host packs window w + 1 while window w is on its way
    double* h_up[2] = {nullptr, nullptr};
    hipEvent_t ev_up[2] = {nullptr, nullptr};
    int up_next = 0;
    WinHead* h_head = nullptr;              // mapped pinned host memory, [W]
    double* h_stage = nullptr;              // pinned staging for vba_set_states: [n_max * 10 + 1]
    double* h_back = nullptr;               // pinned staging for vba_get_states: [n_max * 10] + one WinScalars
    bool back_valid = false;                // h_back holds window 0's states and scalars after the last step (vba_iterate)
    double* S[2] = {nullptr, nullptr};      // the two state buffers [W][n_max][10]; S[par] is the input of the next call
    int par = 0;                            // parity of the next call (WinScalars: what a call hands on lives in the slots of the reader's parity)
    bool need_hist_reset = false;           // a call was abandoned half way: its histograms may be dirty
    hipEvent_t ev_stage = nullptr;          // the last staged copy has left the staging buffer
    // One-window latency-mode handles: vba_set_states(window 0) only stages -- states and damping into mapped pinned memory -- and the
    // first kernel of the next chained schedule (k_reset_calls) copies them into S[par] / sc.lam[par]: no stream copy, no runtime call.
    // Every other consumer of the states sends them up with the two stream copies first (flush_states, called by settle()).
    // One buffer is enough: the kernel that reads it has finished when vba_run_schedule returns (read_heads), the copies of a flush
    // are waited for through ev_stage like those of h_stage.
    double* h_stage_map = nullptr;          // [n_max * 10 + 2]: states, damping
    const double* d_stage_map = nullptr;    // ... as the device sees it
    struct PendingStates { bool on = false; int par = 0, n = 0; } pend;    // staged, not yet on the device: for S[par], n poses
    bool stage_copy = false;                // copies of a flush may still be reading h_stage_map (ev_stage follows them)
    bool stage_kernel = false;              // a schedule that was to read h_stage_map did not return cleanly: wait for the stream
    std::vector<int> n, m;
    std::vector<char> have_obs, have_win, have_state, have_prior;
    bool reg = false;               // BA_reg semantics (per-pose prior) for the following calls
    double *d_prior_H = nullptr, *d_prior_x = nullptr;
    std::vector<std::vector<int64_t>> perm; // sorted position -> input row
    float last_ms = 0.f;
    bool stepped = false;
    int carry_ok = 0;               // every window's keys / histogram / sum |r| for its current states are on the device: 0 no, 1 with the
                                    // exponent histogram, 2 with the warm histogram (the kind the last trial emitted)
    bool carry_enabled = true;
    bool hist_dirty = false;        // a k_trial<true> has left a warm histogram (digit-0 slot of parity `par`) behind that nobody consumed
    bool fold_enabled = true;       // chained schedule: the first kernel of call c + 1 evaluates the accept test of call c (latency mode)
    int warm_enabled = 1;           // carried keys are selected with the one-pass warm select (vba_set_warm_select; 2: forced misses, test knob)
    int last_iter = 0, last_init = 0;
    int sh_pivot = 0;                       // sharded mode: solver variant of the current call (0 unpivoted, 2 mixed after a failed check)
    bool sh_rode = false, sh_bands_ready = false;   // sharded mode: the dynamics factor rode in the accumulation; bands / rhs are in memory
    // sharded mode with the exchanges issued by the library itself (vba_sh_comm_init / vba_sh_call): RCCL resolved at run time
    struct ShComm {
        void* dl = nullptr;
        ncclComm_t comm = nullptr;
        int nranks = 0, rank = 0;
        ncclResult_t (*all_gather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
        ncclResult_t (*comm_destroy)(ncclComm_t) = nullptr;
        const char* (*error_string)(ncclResult_t) = nullptr;
        double* buf = nullptr;              // one allocation: abs_local | abs_all | partial_local | partial_all | trial_local | trial_all
        int64_t m_total = 0, m_pad = 0;     // what buf was sized for
        int n = 0;
        int m_local = -1;                   // rows of this rank the +inf padding of abs_local was laid out for
        // carried-keys protocol (vba_sh_run_schedule): exchange buffers that the kernels write in place
        int protocol = 1;                   // 1 = carried keys (default), 0 = the round-3 protocol (every call gathers all keys)
        ncclResult_t (*group_start)() = nullptr;
        ncclResult_t (*group_end)() = nullptr;
        double* buf2 = nullptr;             // sendA[2] | recvA | sendB | recvB
        int lenA = 0, lenB = 0, n2 = 0, nbo2 = 0, nbd2 = 0, cap2 = 0;
        double *sendA[2] = {nullptr, nullptr}, *recvA = nullptr, *sendB = nullptr, *recvB = nullptr;
        bool carried = false;               // recvA holds the exchange of the trial that produced the resident states: the next call may start from it
        int carried_par = 0;                // ... whose parity (the parity of the call that will read it)
        long fallbacks_miss = 0, fallbacks_lm = 0;
        double *abs_local = nullptr, *abs_all = nullptr, *partial_local = nullptr, *partial_all = nullptr, *trial_local = nullptr, *trial_all = nullptr;
    } shc;
    int pack_min = 1 << 30;                 // windows from which three chains share a wavefront: never by default (measured at 1024 / 2048 / 4096
                                            // windows: one wave per window is as fast or faster, 1.52 / 1.96 / 2.70 ms vs 1.52 / 2.06 / 2.78 ms per solve);
                                            // vba_set_solver(h, -3) packs from 3 windows on
    int no_pack = 0;                        // diagnostic: force one window per wavefront in the sequential driver
    int pivot_mode = 0;                     // 0 = fast path with automatic fallback, 1 = always pivot
    int fallbacks = 0;                      // number of solves repeated with pivoting (diagnostic)
    int inline_select = 1;                  // latency mode: warm select inside the accumulation (bin buckets); vba_set_warm_select(h, 3) turns it off
    int chunk_waves = 2;                    // vba_set_chunk_waves
    int cr_levels = 2;                      // cyclic-reduction levels in front of the one-workgroup kernel (VBA_CR_LEVELS / vba_set_cr_levels: 2 or 3)
    int fusion = 15;                        // vba_set_fusion (default: the trial kernel forms the step, the solves form their own blocks, uniform-pass assembly)
    bool fusion_auto = true;                // the mask is the library's own choice (vba_set_fusion not called)
    GraphCache gcache;
    // Generation of everything a DevView of view_for_call or a branch of the enqueue functions is made from, apart from what
    // pass_identity (vba_schedule.hip) lists itself.  touch() -- called by every entry point that can change one of them -- covers:
    //   h->V.*          every field of the handle's base view: chunk, chunk2 (vba_set_solver / _solver2), hop, nblk_long
    //                   (vba_set_integrator, vba_upload_window), acc_lanes, trial_tiles, warm_shift, bucket_cap, jac_f32 (vba_set_option),
    //                   n_min (vba_upload_observations), m_total, warm_shift (vba_sh_*), inv_sigma2 (Schur add-on)
    //   h->n, n_long    pose counts (n_min of a view, the count of the staged states) and long edges: the uploads
    //   h->reg          vba_set_prior
    //   h->fusion, fusion_auto, chunk_waves, cr_levels, pivot_mode, no_pack, pack_min, warm_enabled, inline_select, carry_enabled,
    //   pipeline, graph_enabled, cprof.on          vba_set_option, vba_set_solver, vba_sh_run_schedule (fusion)
    //   h->stream       vba_set_stream (also in the identity itself)
    // fold_enabled and the VBA_* environment switches are fixed when the handle / the process starts.  A field that is missed here
    // replays a stale graph: a wrong result, not a slow one.
    unsigned long long gen = 0;
    void touch() { ++gen; }
    bool graph_enabled = true;              // vba_set_schedule_graph
    int bucket_cap_alloc = 0;               // allocated capacity of a bin bucket (vba_set_bucket_cap lowers the one in use)
    int warm_misses = 0;                    // number of calls whose warm select missed and was repeated with the exact digits (diagnostic)
    double* d_dbg = nullptr;                // lazily allocated scratch for debug fetch
    size_t dbg_cap = 0;
    // The uncertainty queries (vba_query.hip; vba_cov.hip, vba_rel.hip, vba_power.hip): each has a scratch allocated by its first call, and the
    // time of its last call from cov_ev0, recorded in front of the covariance step all three start with
    QueryScratch q_cov;                      // the shadow of every array the front of a call writes, Sigma's blocks (cov_layout)
    QueryScratch q_rel;                      // rel_layout: the two row arrays, the device copy of perm, the pose summary
    QueryScratch q_pow;                      // pow_layout: four row arrays, the pose and window summaries
    // Data snooping (vba_snoop.hip).  Its scratch is state, not a query's: the confidences the rejected rows had and the cumulative
    // mask (snoop_layout), allocated by the first vba_snoop.  snoop_total: rows rejected per window (empty until then)
    QueryScratch q_snoop;
    std::vector<int> snoop_total;
    QueryScratch q_snoop_fit;                // vba_snoop_scaled's own scratch, a query's (snoop_fit_layout): nothing in it outlives a call
    hipEvent_t cov_ev0 = nullptr;
    bool sharded = false;                   // an observation-sharded call has run (vba_sh_*): no covariance query
    std::vector<char> perm_stale;           // [W] once a row pass has run: the device copy of perm[w] predates the last upload
    // Pipelined driver loop (vba_iterate_resident, see iterate_pipelined): the call that was enqueued speculatively behind
    // the one that has just been returned, the chain it belongs to and what has been learnt about the caller's schedule
    struct Spec { bool valid = false; int iter = 0, init = 0; bool reg = false; int c = 0; } spec;
    int chain_par0 = 0;                     // parity of call 0 of the open chain
    int pred_iter[64], pred_init[64];       // what followed a resident call with iter & 63 (-1: not seen yet, -2: nothing resident)
    int prev_res_iter = -1;                 // iter of the previous resident call (for learning), -1: none
    int pipeline = 1;                       // vba_set_pipeline
    bool last_pipelined = false;            // the last call went through iterate_pipelined: a speculated call has reused its scratch
    int spec_hits = 0, spec_discards = 0;   // diagnostics (vba_pipeline_stats)
    struct Watch { const void* live = nullptr; const void* copy = nullptr; size_t bytes = 0; } watch[8];   // vba_set_host_watch
    // The watched buffers are compared by a helper thread of the handle while the calling thread enqueues the speculated call: the
    // comparison of the reference driver's `ii` (400 kB at C3) is ~9 us of memcmp, and a landmark-only call leaves the host no idle
    // time to hide it in (23 us of device work against ~29 us of host work per resident call before this).
    struct WatchWorker {
        std::thread th;
        std::mutex m;
        std::condition_variable cv;
        unsigned long long seq = 0;         // guarded by m: number of the last request
        bool quit = false;                  // guarded by m
        std::atomic<unsigned long long> done_seq{0};    // the request `changed` answers
        bool changed = false;
        bool started = false;
        pid_t owner = 0;                    // the process the helper thread lives in (a forked child inherits `started`, not the thread)
    } ww;
    // vba_set_chain_profile: HIP events at the class boundaries (accumulate | solve | trial) of every call of a chained schedule
    struct ChainProf {
        bool on = false;
        std::vector<hipEvent_t> ev;         // 4 per call: before / behind the accumulation, behind the solve, behind the trial
        double ms[3] = {0.0, 0.0, 0.0};
        int64_t launches[3] = {0, 0, 0};
    } cprof;
    double* h_states_map = nullptr;         // [2][n_max][10] mapped pinned host memory (DevView::host_states), one-window handles
    hipEvent_t ev_first = nullptr;
};

// ---- vba_api.hip
void fill_params(StepParams& p, int iter, int initialize);
int check_window(vba_handle h, int window);
int read_heads(vba_handle h);
const volatile WinHead* head(vba_handle h, int w);
int settle(vba_handle h, bool boundary = false, bool keep_staged = false);
int ready(vba_handle h);

// ---- vba_handle.hip
constexpr int kPartitionedWindowsMax = 1023;    // more windows than this: the sequential walk (measured: the comment over default_latency_mode)

// ---- vba_options.hip
int vba_set_accumulate_lanes(vba_handle h, int lanes);      // (behind vba_set_option; vba_create_mode sets the defaults through them)
int vba_set_trial_tiles(vba_handle h, int tiles);

// ---- vba_upload.hip
int flush_states(vba_handle h);
void unpack_scalars(const WinScalars* sc, int par, double* lamda, double* last_hessian, int* n_trials, unsigned* flags);

// ---- vba_call.hip (one BA() call: the kernels and their order are described at the top of that file)
struct CallSpec {
    bool host_out = false;  // pipelined vba_iterate_resident: trial states and last_hessian also go to mapped host memory
    int iter = 0, initialize = 0;
    int call = -1;          // index inside a chained schedule, -1: stand-alone
    int par = 0;
    int carry = 0;          // the keys of the input states are on the device: 0 no, 1 with their exponent histogram, 2 with a warm one
    int emit = 0;           // leave the next call's keys behind: 0 no, 1 with the exponent histogram, 2 with the warm one
    bool fold = false;      // first kernel evaluates the accept test of call - 1
    bool prof = false;      // serialised schedule with an event between kernel classes
};

struct CallCtx {
    DevView V;
    hipEvent_t after_first = nullptr;   // recorded behind the kernel that starts the call (the folded accept test of the call in front is in it)
    bool fuse_assemble = false;     // first trial's landmark-only solve rides in k_assemble<true> (batched windows)
    bool assembled = false;         // an assembly kernel ran (profile bookkeeping)
    bool bands_ready = false;       // bands / rhs are in memory (the fused landmark-only assembly does not write them)
};

void view_for_call(vba_handle h, DevView& V, const CallSpec& c);
int enqueue_front(vba_handle h, CallCtx& C, const CallSpec& c, bool exact_repeat, hipEvent_t* ev);
void enqueue_trial(vba_handle h, CallCtx& C, const CallSpec& c, bool first, hipEvent_t ev_solve = nullptr, int solve_redo = -1);
int step_impl(vba_handle h, int iter, int initialize, float* prof, bool emit = true, int readback = -1);
int finish_stalled_call(vba_handle h, const CallSpec& q, const std::vector<int>& stall_at, long& trials);
// Any error return while one of these is armed leaves a half-run call behind: counts in any histogram, states and carried keys that
// nobody can vouch for.  pipelined (iterate_pipelined): the speculated call and what the loop learnt from the previous one go as well.
struct CallAbandon {
    vba_handle h; bool pipelined = false; bool armed = true;
    ~CallAbandon() {
        if (!armed) return;
        h->need_hist_reset = true; h->have_state.assign(h->W, 0); h->carry_ok = 0;
        if (pipelined) { h->spec.valid = false; h->prev_res_iter = -1; }
    }
};
// ... whose histograms (an abandoned call may have left counts in any of them) the next call clears in front of its own kernels;
// V: any view of the handle.  Nothing unless need_hist_reset.
void clear_abandoned_hists(vba_handle h, const DevView& V, hipStream_t s);

// ---- vba_schedule.hip
int vba_set_schedule_graph(vba_handle h, int on);      // (options of vba_set_option that live with the schedule)
int vba_set_chain_profile(vba_handle h, int on);

// ---- vba_iterate.hip
void watch_stop(vba_handle h);
void watch_quiesce(vba_handle h);

// ---- vba_query.hip
// The step the queries share: the shadow front of a full-phase call and the selected inversion, into the scratch of the
// covariance query (see vba_cov.hip).
struct CovQuery {
    DevView V;                  // the shadow view: wraw, sc (maximum raw weight of parity V.par) and states are what the row pass reads
    double* diag = nullptr;     // [W][n_max][81] Sigma_ii
    double* sup = nullptr;      // [W][n_max][81] Sigma_i,i+1
    unsigned* flags = nullptr;  // [W]
};
int cov_begin(vba_handle h, int iter, const char* who);
int cov_build_invert(vba_handle h, int iter, int damped, CovQuery& q);
// The scaffold of a query around that step.  query_reserve: q.d holds at least `bytes` (the total of the query's layout,
// vba_query_layout.h), kept or grown; `what` ends the message of a failed allocation.  query_finish: the end event behind the
// query's last kernel, the wait for it, q.ms since cov_ev0.  query_last_ms: what the vba_last_*_ms getters return.
// query_copy_out: the copy of a per-window result to the host (`used[w] * per` doubles of every window's `stride`; the rest stays
// as the caller left it).
int query_reserve(vba_handle h, QueryScratch& q, size_t bytes, const char* what);
int query_finish(vba_handle h, QueryScratch& q);
int query_last_ms(vba_handle h, QueryScratch vba_context::*q, float* ms, const char* none_ran);
int query_copy_out(double* out, const double* dev, size_t W, size_t stride, const std::vector<int>& used, size_t per);

// ---- vba_cov.hip
// What of the covariance scratch is not the shadow view's (cov_layout, vba_query.hip), and the selected inversion of the shadow
// view's bands into it: the launches behind the front, on the path the solver setting selects.
struct CovBufs {
    WinScalars* sc;
    double* pool;
    double *diag, *sup;         // the two [W][n_max][81] result arrays
    unsigned* flags;
    double *X, *contrib, *sepb, *SSd, *SSs;     // partitioned path: X, chunk contributions, separator bands, separator blocks of Sigma
};
int launch_cov_invert(vba_handle h, const DevView& V, const CovBufs& b, int damped, hipStream_t s);

// ---- vba_rel.hip
// What the row passes behind the covariance step share on the host: the device copy of the upload's permutation (sorted position ->
// input row, [W][m_max], part of the reliability scratch, uploaded for the windows whose rows changed).
int rel_device_perm(vba_handle h, const int** d_perm);
int rel_device_bufs(vba_handle h, RelBufs& b);

// ---- vba_snoop.hip
// vba_upload_observations of a window whose handle has snooped: the window's mask is cleared (its rows are new ones)
int snoop_forget_window(vba_handle h, int window);
#pragma GCC visibility pop
