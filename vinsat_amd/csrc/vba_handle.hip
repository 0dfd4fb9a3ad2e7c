// vba_handle.hip -- the life of a handle: which kernel set and fusions it defaults to, the device arena and its layout, the host
// resources, vba_destroy (which also takes a half-built handle: every failure exit of vba_create_mode leaves through it).
#include "vba_context.h"

// The second stream of handles with many windows carries the dynamics factor beside the streaming observation kernels.
// VBA_AUX_PRIO (diagnostic): 1 = highest priority, -1 = lowest, unset / 0 = default.
static hipError_t create_aux_stream(hipStream_t* s) {
    // VBA_AUX_CUMASK (diagnostic): hex word repeated over the 8 x 32 compute units, e.g. 11111111 = every fourth one
    if (const char* m = std::getenv("VBA_AUX_CUMASK")) {
        const uint32_t word = (uint32_t)std::strtoul(m, nullptr, 16);
        uint32_t mask[8];
        for (auto& x : mask) x = word;
        return hipExtStreamCreateWithCUMask(s, 8, mask);
    }
    const char* e = std::getenv("VBA_AUX_PRIO");
    const int want = e ? std::atoi(e) : 0;
    if (want == 0) return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    return hipStreamCreateWithPriority(s, hipStreamNonBlocking, want > 0 ? greatest : least);
}

// Where the mode switches of a handle lie, chosen from the round-4 sweeps over W = 1 .. 4096 windows with the kernel set and the
// solver forced (tools/mode_sweep.py; DESIGN.md section 7, bench.py "batched_sweep").  C3 windows (500 poses / 50 000 rows),
// thousands of BA calls per second:
//   W            1    2    4    8   12   16   22   28   32   48   64  128  256  512 1024 2048 4096
//   latency     22   40   71  114  144  168  187  201  204    .  184  189  202  204    .    .    .   (best fusion mask, below)
//   bandwidth    .   23   38   64  112  139  167  194  212  245  273  314  342  361  367    .  369   (partitioned solve)
//   ... walk     .    2    4    9    .   17   23    .   34    .   63  114  187  277  366  435  479   (four windows per wavefront)
// (as measured when the switches were placed; with the tiled trial kernel and the chunk rules that followed the latency row reads
// 22 / 41 / 74 / 125 / 154 / 177 / 201 / 210 at W = 1 .. 28, bench.py "batched_sweep")
// and C2 windows (100 poses / 5 000 rows): latency 107 / 379 / 606 / 943 / 1230 / 1446 / 1541 at W = 4 / 16 / 32 / 64 / 128 / 256 /
// 512 against bandwidth 51 / 199 / 360 / 662 / 1145 / 1649 / 1931; walk against partitioned solve 954 : 1649 at 256 windows,
// 2183 : 2071 at 1024, 3227 : 2259 at 4096.
// * Kernel set: what fills the chip is rows AND windows -- the latency-mode kernels won up to 31 C3 windows, ~180 C2 windows, ~13
//   C4 windows in that sweep (38 / ~190 / ~20 with the latency set as it is now, see default_latency_mode below; until round 4 the
//   switch was at 16 windows whatever their size).
// * Solver: the sequential walk is a latency chain per window (~2.2 ms at 500 poses whatever the window count) and pays only
//   once ~1000 windows share it; below that the chains are cut into chunks (until round 4 the walk took over at 128 windows:
//   3.3 ms per step at 256 windows where the partitioned solve needs 0.75).  (kPartitionedWindowsMax, vba_context.h)
// * Inside latency mode the fusions that trade instructions for launches hold only while launches are what a call costs:
//   up to 175 000 rows mask 15 (the trial kernel forms the step, the chunk elimination its blocks); up to 450 000 rows 14 (the
//   trial kernel reads a step that a launch of its own formed: every observation block re-forming the steps of its poses costs
//   more than that launch as soon as a few windows share the chip); beyond 12 (the assembly is a launch of its own as well).
constexpr int kLatWindowsCap = 192;             // (33 MB of bin buckets per C3 window; per-window prologues)
// The crossover measured at three window sizes -- ~180 windows of 5 000 rows, 31 of 50 000, ~13 of 200 000 (C4: latency 55.1 / 64.0 /
// 65.7 k it/s at W = 8 / 12 / 16 against bandwidth 50.0 / 62.9 / 73.7) -- lies on W* = 31 (50 000 / m)^0.7: between "by windows"
// (exponent 0) and "by rows" (exponent 1), because both the per-window prologues and the rows fill the chip.
// Re-measured at the end of round 4, after the tiled trial kernel and the chunk rules had made the latency set 4 .. 20 % faster
// (k it/s, latency : bandwidth): C3 212 : 205 at 32 windows, 216 : 213 at 36, 223 : 226 at 40; C4 80.3 : 73.3 at 16, 79.7 : 80.0 at
// 20; 200 poses / 20 000 rows 502 : 480 at 64, 544 : 594 at 96; C2 1389 : 1251 at 160, 1399 : 1403 at 192 -- W* = 38 (50 000 / m)^0.7
// for windows up to C3's size, 38 (50 000 / m)^0.46 beyond.
static bool default_latency_mode(int windows, int64_t m_max) {
    const double x = m_max <= 50000 ? 0.7 : 0.46;
    return windows == 1 || (windows <= kLatWindowsCap && (double)windows <= 38.0 * std::pow(50000.0 / (double)m_max, x));
}
static int default_fusion(bool lat, int windows, int n_max, int64_t m_max) {
    const double rows = (double)windows * (double)m_max;
    // one window (round 4, with the trial kernel's observation blocks of several tiles, vba_set_trial_tiles): mask 15 : 14 = 19.8 : 19.6
    // k it/s at 75 000 rows, 19.3 : 18.8 at 100 000, 17.1 : 17.2 at 150 000, 15.4 : 17.4 at 200 000 (C4), 10.1 : 12.2 at 500 000 rows /
    // 2004 poses (C5), 15.4 : 16.3 at 100 000 rows / 2000 poses
    if (windows == 1) return (lat && (m_max >= 150000 || n_max >= 1500)) ? 14 : 15;
    return !lat ? 15 : rows <= 175e3 ? 15 : rows <= 450e3 ? 14 : 12;
}

// ---- the device arena: one allocation, cut into the buffers of every window by arena_layout

// What the layout depends on, computed once so that the counting and the placing pass see the same values.
struct ArenaShape {
    size_t W, N, M;
    size_t m_pad, obs_stride;       // doubles per observation array / per window's observation block
    int nblk_obs, nblk_dyn, nblk_pred;
    int trial_stride, pred_stride;
    size_t long_pool_cap;
    int warm_shift, bucket_cap;
    size_t p_max;
};

static ArenaShape arena_shape(int windows, int n_max, int64_t m_max, bool lat) {
    ArenaShape s;
    const size_t N = s.N = n_max, M = s.M = (size_t)m_max;
    s.W = windows;
    s.nblk_obs = (int)((M + kObsBlock - 1) / kObsBlock);
    s.nblk_dyn = (int)((N + kObsBlock - 1) / kObsBlock);
    const int nblk_dyn16 = (int)((N - 1 + 14) / 15);      // pose-chain blocks of the 16-lanes-per-pose geometry (vba_set_fusion bit 0)
    s.trial_stride = s.nblk_obs + std::max(s.nblk_dyn, nblk_dyn16) + kLongCap;     // (+ the slots of the long edges, vba_long.hip)
    s.m_pad = (M + 31) & ~size_t(31);
    s.obs_stride = (6 * s.m_pad + s.m_pad / 2 + (N + 2) / 2 + 31) & ~size_t(31);     // doubles
    s.nblk_pred = (int)((N * kDynLanes + 255) / 256);
    s.pred_stride = s.nblk_pred + kLongCap;
    s.long_pool_cap = windows <= kLongPoolFewWindows ? kLongPoolFew : kLongPool;
    // bin buckets of the carried keys (latency mode only): capacity ~6x the count of the densest warm bin -- the bin of the
    // median holds ~0.13 % of the keys with 1/256-binade bins, half of that with 1/512 (see warm_shift below)
    // ... and 2^46 (1/64 of a binade, range [c / 2^16, c * 2^16)) for handles of many windows: the flush of a block's
    // histogram costs a global atomic per bin it touched, coarser bins contend in LDS and lengthen the list the single pass
    // (k_select_warm) compacts and k_select_finish ranks -- about half a per cent of the keys here.  Swept 44 .. 51 at
    // 4096 x C3: 10.53 / 9.94 / 9.85 / 9.87 / 9.90 / 9.94 / 10.03 ms per step for 44 .. 50 (exact two-pass select: 10.12)
    // warm bins: 2^44 bit patterns (1/256 of a binade, range [c/16, c*8)) while a bin of the median's density stays short,
    // 2^43 (1/512, [c/4, c*2)) for the big windows
    s.warm_shift = !lat ? 46 : (2 * m_max <= 300000 ? 44 : 43);
    s.bucket_cap = 0;
    if (lat) {
        const double expect = 2.0 * (double)m_max * (s.warm_shift == 44 ? 0.0013 : 0.00065) * 6.0;
        s.bucket_cap = 256;
        while (s.bucket_cap < expect && s.bucket_cap < 4096) s.bucket_cap *= 2;
    }
    s.p_max = n_max / 2 + 1;
    return s;
}

// Every buffer of the arena, once: over a Carver without a base this counts, over the allocation it places (vba_query_layout.h).
// The order is part of the layout: each buffer starts where the one before it ended, rounded up to 256 bytes.
static void arena_layout(Carver& A, const ArenaShape& s, vba_context* h) {
    const size_t W = s.W, N = s.N, M = s.M, PM = s.p_max;
    DevView& V = h->V;
    V.n = h->d_n = A.take<int>(W);
    V.m = h->d_m = A.take<int>(W);
    V.sc = A.take<WinScalars>(W);
    h->d_obs = A.take<double>(W * s.obs_stride);
    h->S[0] = A.take<double>(W * N * 10); h->S[1] = A.take<double>(W * N * 10);
    V.part_pred = A.take<double>(W * 2 * s.pred_stride); V.part_prior = A.take<double>(W * 2 * s.pred_stride);
    V.long_idx = h->d_long_idx = A.take<int>(W * kLongCap); V.n_long = h->d_n_long = A.take<int>(W);
    V.long_off = h->d_long_off = A.take<int>(W * kLongCap);
    V.long_pool = A.take<double>(W * 2 * s.long_pool_cap * 6);
    V.lastD = A.take<double>(W * 81);
    V.intr = h->d_intr = A.take<double>(W * N * 4);
    V.cumrot = h->d_cumrot = A.take<double>(W * N * 4);
    V.steps = h->d_steps = A.take<int>(W * N);
    V.prior_H = h->d_prior_H = A.take<double>(W * N * 36);
    V.prior_x = h->d_prior_x = A.take<double>(W * N * 6);
    V.absr = A.take<double>(W * 2 * M); V.wraw = h->wraw2 = A.take<double>(2 * W * M); V.ckeys = A.take<double>(W * 2 * M);
    V.part_init = A.take<double>(W * s.nblk_obs); V.part_trial = A.take<double>(W * s.trial_stride);
    V.part_next = A.take<double>(W * s.nblk_obs);
    V.hist = A.take<unsigned>(W * kHistStride);
    // (latency mode only: ask bucket_cap, never the pointer, whether a handle has buckets -- the counting pass places nothing)
    V.wbucket = s.bucket_cap ? A.take<double>(W * 2 * (size_t)kSelBins * s.bucket_cap) : nullptr;
    V.Hraw = h->Hraw2 = A.take<double>(2 * W * N * 21); V.braw = h->braw2 = A.take<double>(2 * W * N * 6);
    // (the pose-chain factor's outputs: per call parity as well, see wraw2)
    V.xhat = h->dyn2[0] = A.take<double>(2 * W * N * 6); V.Phi = h->dyn2[1] = A.take<double>(2 * W * N * 36); V.rorb = h->dyn2[2] = A.take<double>(2 * W * N * 6);
    V.fatt = h->dyn2[3] = A.take<double>(2 * W * N); V.qgrad = h->dyn2[4] = A.take<double>(2 * W * N * 3);
    V.Hd = h->dyn2[5] = A.take<double>(2 * W * N * 9); V.Hu = h->dyn2[6] = A.take<double>(2 * W * N * 9); V.Hl = h->dyn2[7] = A.take<double>(2 * W * N * 9);
    V.bands = A.take<double>(W * N * 243); V.rhs = A.take<double>(W * N * 9);
    V.Xs = A.take<double>(W * N * 81); V.zs = A.take<double>(W * N * 9); V.dpose = A.take<double>(W * N * 9);
    V.csol = A.take<double>(W * N * 171);
    V.cL = A.take<double>(W * PM * 171); V.cR = A.take<double>(W * PM * 171);
    V.rXs = A.take<double>(W * PM * 81); V.rzs = A.take<double>(W * PM * 9); V.rx = A.take<double>(W * PM * 9);
    V.csol2 = A.take<double>(W * PM * 171); V.cL2 = A.take<double>(W * PM * 171); V.cR2 = A.take<double>(W * PM * 171);
    V.rx2 = A.take<double>(W * PM * 9);
    V.res_flags = A.take<unsigned>(W * (N + 8));        // flags of the resident solve (over-sized: chunks + groups + 1 <= n_max / 2 + 8)
}

// Bytes allocated behind the last buffer of the layout.  Nobody has shown that no kernel reads past the last buffer (the arena
// has always ended in a pad of this size), so the tail stays until somebody does.
constexpr size_t kArenaTail = size_t(1) << 16;

// count, allocate and clear, place
static int carve_arena(vba_context* h, const ArenaShape& s) {
    Carver count;
    arena_layout(count, s, h);
    const size_t bytes = count.total() + kArenaTail;
    if (hipMalloc(&h->arena, bytes) != hipSuccess) {
        h->arena = nullptr;
        return fail(VBA_ENOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes failed");
    }
    // (hipMemset of device memory returns before the fill has run, and the handle's streams are non-blocking: without the wait the
    // fill of a 50 GB arena was still running when the first windows were uploaded and zeroed their observations again)
    if (hipMemset(h->arena, 0, bytes) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess)
        return fail(VBA_EHIP, "hipMemset of the device arena failed");
    Carver place;
    place.base = h->arena;
    arena_layout(place, s, h);
    if (place.total() != count.total()) return fail(VBA_ENOMEM, "internal: device arena mis-carved");
    return VBA_OK;
}

// the view every call starts from: the shape, the pointers that lie inside a carved buffer, every switch at its resting value
static void init_view(vba_context* h, const ArenaShape& s, bool lat) {
    DevView& V = h->V;
    V.W = h->W; V.n_max = h->n_max; V.m_max = h->m_max; V.nblk_obs = s.nblk_obs; V.nblk_dyn = s.nblk_dyn;
    const size_t m_pad = s.m_pad;
    h->m_pad = (int64_t)m_pad;
    V.obs_stride = (int64_t)s.obs_stride;
    V.ox = h->d_obs; V.oy = V.ox + m_pad; V.oz = V.oy + m_pad; V.ou = V.oz + m_pad; V.ov = V.ou + m_pad; V.oconf = V.ov + m_pad;
    V.opose = reinterpret_cast<const int*>(V.oconf + m_pad);
    V.pose_ptr = V.opose + m_pad;
    V.states = V.states_prev = h->S[0]; V.states_new = h->S[1];
    V.nblk_pred = s.nblk_pred;
    V.pred_stride = s.pred_stride;
    V.nblk_long = 0;
    V.long_pool_cap = (int)s.long_pool_cap;
    V.reg = 0;
    V.acc_lanes = 8;    // set after construction by vba_set_accumulate_lanes(h, 0)
    V.trial_stride = s.trial_stride;
    V.bucket_cap = s.bucket_cap;
    h->bucket_cap_alloc = s.bucket_cap;
    V.sel_inline = 0;
    V.p_max = (int)s.p_max;
    V.res_stride = h->n_max + 8;
    V.resident = 0;
    V.m_total = 0; V.abs_all = nullptr; V.abs_all_count = 0;
    V.hop = 0; V.pivot = 0; V.call = -1; V.emit = 0; V.carry = 0; V.dyn_in_acc = 0;
    V.par = 0; V.fold = 0; V.redo = 0; V.fused_trial = 0; V.pending_only = 0; V.warm_force_miss = 0;
    V.lat = lat ? 1 : 0;       // latency mode: few windows cannot fill the chip, the kernel COUNT of a call is what costs
    V.trial_tiles = 1;          // set after construction by vba_set_trial_tiles(h, 0)
    V.warm_shift = s.warm_shift;
    V.chunk = 0; V.chunk2 = 0;      // set after construction by vba_set_solver(h, -1)
    V.host_states = nullptr;
}

// streams, events, pinned and mapped host buffers
static bool create_host_resources(vba_context* h, const ArenaShape& s, bool lat) {
    const int windows = h->W, n_max = h->n_max;
    // the two staging blocks of the uploads: a window's observation block, or its pose constants with the list of its long edges
    const size_t up_bytes = std::max(s.obs_stride, 9 * s.N + 160) * sizeof(double);
    // the second stream carries the dynamics factor beside the observation kernels and exists only where that is done (many
    // windows): a process maps its streams onto a few hardware queues, and every idle stream of another handle is one more
    // to share them with
    return !((windows == 1 && (hipEventCreateWithFlags(&h->ev_first, hipEventDisableTiming) != hipSuccess ||
                               hipHostMalloc((void**)&h->h_states_map, (size_t)2 * n_max * 10 * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
                               hipHostGetDevicePointer((void**)&h->V.host_states, h->h_states_map, 0) != hipSuccess)) ||
             (windows == 1 && lat && (hipHostMalloc((void**)&h->h_stage_map, ((size_t)n_max * 10 + 2) * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
                                      hipHostGetDevicePointer((void**)&h->d_stage_map, h->h_stage_map, 0) != hipSuccess)) ||
             hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess ||
             (!lat && create_aux_stream(&h->aux_stream) != hipSuccess) ||
             hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess ||
             hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess ||
             hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) != hipSuccess ||
             hipEventCreateWithFlags(&h->ev_stage, hipEventDisableTiming) != hipSuccess ||
             hipEventCreateWithFlags(&h->ev_up[0], hipEventDisableTiming) != hipSuccess ||
             hipEventCreateWithFlags(&h->ev_up[1], hipEventDisableTiming) != hipSuccess ||
             hipHostMalloc((void**)&h->h_up[0], up_bytes, hipHostMallocDefault) != hipSuccess ||
             hipHostMalloc((void**)&h->h_up[1], up_bytes, hipHostMallocDefault) != hipSuccess ||
             hipHostMalloc((void**)&h->h_stage, ((size_t)n_max * 10 + 1) * sizeof(double), hipHostMallocDefault) != hipSuccess ||
             hipHostMalloc((void**)&h->h_back, (size_t)n_max * 10 * sizeof(double) + sizeof(WinScalars), hipHostMallocDefault) != hipSuccess ||
             hipHostMalloc((void**)&h->h_head, s.W * sizeof(WinHead), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
             hipHostGetDevicePointer((void**)&h->V.host_head, h->h_head, 0) != hipSuccess);
}

int vba_create(int device, int windows, int n_max, int64_t m_max, vba_handle* out) {
    return vba_create_mode(device, windows, n_max, m_max, -1, out);
}

int vba_create_mode(int device, int windows, int n_max, int64_t m_max, int mode, vba_handle* out) {
    // 1. arguments (callers see which error wins: the order is part of the interface)
    if (!out) return fail(VBA_EINVAL, "null out");
    *out = nullptr;
    if (mode < -1 || mode > 1) return fail(VBA_EINVAL, "mode must be -1 (automatic), 0 (bandwidth-mode kernels) or 1 (latency-mode kernels)");
    if (windows < 1 || n_max < 2 || m_max < 1) return fail(VBA_EINVAL, "need windows >= 1, n_max >= 2, m_max >= 1");
    if (m_max > (int64_t)1 << 30) return fail(VBA_EINVAL, "m_max too large");
    // 2. device
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt == 0) return fail(VBA_ENODEV, "no HIP device visible");
    if (device < 0 || device >= cnt) return fail(VBA_EINVAL, "device index out of range");
    HIPCHK(hipSetDevice(device));
    HIPCHK(configure_solver_device());
    // 3. mode and layout parameters
    const bool lat = mode == -1 ? default_latency_mode(windows, m_max) : mode == 1;
    const ArenaShape shape = arena_shape(windows, n_max, m_max, lat);
    vba_context* h = new (std::nothrow) vba_context();
    if (!h) return fail(VBA_ENOMEM, "host allocation failed");
    h->device = device;
    h->W = windows;
    h->n_max = n_max;
    h->m_max = m_max;
    // from here on every failure leaves through vba_destroy, and reports after it: its settle may write the error text itself
    // 4. - 6. count, allocate and clear, place
    if (const int rc = carve_arena(h, shape)) {
        const std::string msg = g_err;
        vba_destroy(h);
        return fail(rc, msg);
    }
    init_view(h, shape, lat);
    // 7. host resources
    for (int k = 0; k < 64; ++k) h->pred_iter[k] = h->pred_init[k] = -1;
    h->fusion = default_fusion(lat, windows, n_max, m_max);
    if (!create_host_resources(h, shape, lat)) {
        vba_destroy(h);
        return fail(VBA_EHIP, "stream/event/pinned allocation failed");
    }
    h->stream = h->own_stream;
    const size_t W = windows;
    h->n.assign(W, 0); h->m.assign(W, 0); h->n_long.assign(W, 0);
    h->have_obs.assign(W, 0); h->have_win.assign(W, 0); h->have_state.assign(W, 0); h->have_prior.assign(W, 0);
    h->perm.resize(W);
    // 8. defaults that have a setter
    vba_set_accumulate_lanes(h, 0);
    vba_set_trial_tiles(h, 0);
    vba_set_solver(h, -1);
    // warm select everywhere; the accept test is folded into the next call's first kernel only in latency mode (with many
    // windows the decide launch is 20 us of a 10 ms step, and every block of the select would repeat the test)
    h->warm_enabled = 1;
    h->fold_enabled = lat;
    // 9. environment knobs
    if (const char* e = std::getenv("VBA_X_FOLD")) h->fold_enabled = std::atoi(e) != 0;     // (experiment knob)
#ifdef VBA_VARIANTS
    if (const char* e = std::getenv("VBA_CR_LEVELS")) h->cr_levels = std::atoi(e) == 3 ? 3 : 2;     // (three levels in front: measured slower, comparison build only)
#endif
    *out = h;
    return VBA_OK;
}

int vba_destroy(vba_handle h) {
    if (!h) return VBA_OK;
    h->pend.on = false;
    (void)settle(h);
    watch_stop(h);
    hipSetDevice(h->device);
    (void)vba_sh_comm_destroy(h);
    if (h->own_stream) { hipStreamSynchronize(h->own_stream); hipStreamDestroy(h->own_stream); }
    if (h->aux_stream) { hipStreamSynchronize(h->aux_stream); hipStreamDestroy(h->aux_stream); }
    for (hipEvent_t e : h->cprof.ev) if (e) hipEventDestroy(e);
    h->gcache.destroy();
    if (h->ev_first) hipEventDestroy(h->ev_first);
    if (h->h_states_map) hipHostFree(h->h_states_map);
    if (h->h_stage_map) hipHostFree(h->h_stage_map);
    if (h->ev_fork) hipEventDestroy(h->ev_fork);
    if (h->ev_join) hipEventDestroy(h->ev_join);
    if (h->ev0) hipEventDestroy(h->ev0);
    if (h->ev1) hipEventDestroy(h->ev1);
    if (h->ev_stage) hipEventDestroy(h->ev_stage);
    for (int k = 0; k < 2; ++k) {
        if (h->ev_up[k]) hipEventDestroy(h->ev_up[k]);
        if (h->h_up[k]) hipHostFree(h->h_up[k]);
    }
    if (h->h_stage) hipHostFree(h->h_stage);
    if (h->h_back) hipHostFree(h->h_back);
    if (h->h_head) hipHostFree(h->h_head);
    if (h->d_dbg) hipFree(h->d_dbg);
    for (QueryScratch* q : {&h->q_cov, &h->q_rel, &h->q_pow, &h->q_snoop, &h->q_snoop_fit}) {
        if (q->d) hipFree(q->d);
        if (q->ev) hipEventDestroy(q->ev);
    }
    if (h->cov_ev0) hipEventDestroy(h->cov_ev0);
    if (h->arena) hipFree(h->arena);
    delete h;
    return VBA_OK;
}
