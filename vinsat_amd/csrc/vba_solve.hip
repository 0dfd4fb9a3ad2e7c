// vba_solve.hip -- damped block-tridiagonal solve (A7) and retraction (A8): the host dispatch over the solver units, and the
// LM accept test.
//
// The reference forms the (9n)^2 matrix densely and calls LU (BA_filtering.py:54-55).  The matrix is exactly block tridiagonal
// in 9x9 blocks, so the solve here is a block elimination along the pose chain (vba_solve_step.h has the method and the lane
// layout).  launch_solve below is the decision tree of DESIGN.md section 4; the kernels live in
//   vba_solve_seq.hip      sequential walks: one or four windows per wave, and the block-diagonal landmark-only phase
//   vba_solve_chunks.hip   the partitioned chain: chunk eliminations, the walk of the reduced system, recovery
//   vba_solve_cr.hip       the reduced system by block cyclic reduction
//   vba_solve_variants.hip comparison builds only (make VARIANTS=1): the measured dead ends
#include "vba_decide.h"
#include "vba_device.h"
#include "vba_launch.h"
#include "vba_solve_units.h"

namespace vba {

// ================================================================================================== accept test
// LM accept test (BA_filtering.py:51, 66-79) as its own launch, one block per window: vba_decide.h has the arithmetic.
// ranks == 0: this window's block partials; ranks > 0: the observation part is the rank-ordered sum of the gathered
// per-rank sums (sharded mode).  What a call hands to the next is written to the slots of the other parity; the states
// need no copy (the buffer the last trial wrote IS the next call's input).
__global__ __launch_bounds__(256) void k_decide(DevView V, const double* trial_all, int ranks) {
    __shared__ double red[5][4];
    const int w = blockIdx.x;
    VBA_SKIP_CALL(V, w);
    WinScalars& sc = V.sc[w];
    const int t = threadIdx.x;
    const int par = V.par;
    if (sc.done || (V.pending_only && sc.pending != V.call)) return;
    const int n_trials = sc.n_trials;
    const double lam32 = sc.lam32;
    const DecideOut d = decide_eval(V, w, par, V.prm, n_trials, sc.init_residual, trial_all, ranks, red);
    unsigned* hist_next = hist0_of(V, w, par ^ 1);      // filled by k_trial<true>
    if (d.flags & 8u) {             // the un-pivoted solve failed its check: the host repeats it with pivoting
        if (V.emit) for (int b = t; b < kSelBins; b += 256) hist_next[b] = 0u;
        if (t == 0) {
            sc.miss = 0;
            V.host_head[w].flags = d.flags;
            V.host_head[w].done = 0;
        }
        return;
    }
    if (d.stop) {
        if (t < 81) {
            const double hv = V.lastD[(size_t)w * 81 + t] + ((t / 9 == t % 9) ? lam32 : 0.0);
            sc.last_hessian[t] = hv;
            if (V.host_states) V.host_head[w].last_hessian[t] = hv;     // (a pipelined call reads its result from host memory)
        }
    } else if (V.emit) {            // rejected: the next trial histograms its own keys
        for (int b = t; b < kSelBins; b += 256) hist_next[b] = 0u;
    }
    if (t == 0) {
        unsigned fl = d.flags;
        if (n_trials == 0) {
            sc.sum_abs_rpred = d.sum_pred;
            sc.init_residual = d.init_residual;
        }
        sc.trial_residual = d.residual;
        sc.n_trials = n_trials + 1;
        sc.pending = -1;
        sc.miss = 0;
        int call_idx = sc.call_idx;
        double lam_now = d.lam_next;
        if (d.stop) {
            sc.done = 1;
            if (V.call >= 0) sc.call_idx = call_idx = V.call + 1;
            if (!d.accept) fl |= 1u;
            if (!(d.residual == d.residual)) fl |= 2u;
            sc.fl[par] = fl;
            sc.lam[par ^ 1] = lam_now = d.lam_out;
            if (V.emit) sc.sum_in[par ^ 1] = d.sum_next;
        } else {
            sc.lam[par] = lam_now;
        }
        // read by the host after it has waited for the stream: no fence needed
        WinHead& hh = V.host_head[w];
        hh.lamda = lam_now;
        hh.trial_residual = d.residual;
        hh.n_trials = n_trials + 1;
        hh.flags = fl;
        hh.done = d.stop ? 1 : 0;
        hh.call_idx = call_idx;
    }
}

// latency mode with a partitioned chain whose chunk (blocks + staged inputs + elimination scratch) fits the LDS of a CU:
// the chunk kernel forms its blocks itself and k_assemble is not launched (vba_call.hip asks the same question)
// ... and the sequential walk of the batched mode forms them pose by pose (VBA_OPT_FUSION bit 2)
#ifdef VBA_VARIANTS
bool walk_forms_blocks(const DevView& V) { return !V.lat && V.fuse_walk && !V.prm.initialize && V.chunk <= 0 && V.pack != 1; }
#else   // (one window per wavefront forming its own blocks -- k_solve_forming -- is a comparison variant)
bool walk_forms_blocks(const DevView& V) { return !V.lat && V.fuse_walk && !V.prm.initialize && V.chunk <= 0 && V.pack == 2; }
#endif
bool solve_forms_blocks(const DevView& V) {
    // (latency-mode handles only.  Round 5 measured the forming chunk elimination on bandwidth-mode handles, chunks of 12: 260 / 324 /
    // 337 k it/s at 64 / 256 / 512 C3 windows against 270 / 347 / 367 with k_assemble_rows + k_solve_chunks_ts -- its 256-thread
    // blocks with the staged inputs in LDS leave fewer chunks resident than the assembly launch costs)
    return walk_forms_blocks(V) || (V.lat && V.fuse_blocks && !V.prm.initialize && V.chunk >= 2 && V.chunk <= kFusedChunkMax);
}

// One of the two sets of kernels (pivot: row pivoting inside a 9x9 block; see solver_mine, vba_solve_step.h), up to the
// solution of every pose (sequential walks: and its retraction) or, for a partitioned chain, of every separator.
static void launch_solve_variant(const DevView& V, bool pivot, int initialize, hipStream_t s) {
    if (initialize) {       // block diagonal: independent poses
        launch_solve_blockdiag(V, pivot, s);
        return;
    }
#ifdef VBA_VARIANTS
    if (launch_solve_comparison(V, pivot, s)) return;       // the handle's options select a comparison solver
#endif
    if (V.chunk <= 0) {     // one wave walks the whole chain
        launch_solve_walk(V, pivot, walk_forms_blocks(V), s);
        return;
    }
    // the chain in chunks; the reduced system over the separators by a second level of chunks (V.chunk2 > 0) and a sequential
    // walk, or (V.chunk2 < 0) by cyclic reduction
    launch_solve_chunks(V, pivot, solve_forms_blocks(V), s);
    if (V.chunk2 < 0) launch_solve_cr(V, pivot, s);
}

// Dynamic-LDS limits of the solver kernels.  HIP function attributes are per DEVICE, so this runs in every vba_create
// (after hipSetDevice); a refused size is reported there instead of surfacing later as a failed launch.
hipError_t configure_solver_device() {
    hipError_t rc = configure_chunks_device();
    if (rc == hipSuccess) rc = configure_cr_device();
#ifdef VBA_VARIANTS
    if (rc == hipSuccess) rc = configure_variants_device();
#endif
    return rc;
}

void launch_solve(const DevView& V, int initialize, hipStream_t s) {
    if (V.pivot != 1) launch_solve_variant(V, false, initialize, s);
    if (V.pivot != 0) launch_solve_variant(V, true, initialize, s);
    // interiors / retraction: shared by both variants (the sequential walks retract themselves)
    if (initialize) launch_solve_recover(V, 0, s);
    else if (V.chunk > 0) {
        if (V.chunk2 > 0) launch_solve_recover2(V, s);
        // latency mode: the trial kernel recovers the interiors and retracts (V.fused_trial == 2)
        if (V.fused_trial != 2) launch_solve_recover(V, V.chunk, s);
    }
}

void launch_decide(const DevView& V, const double* trial_all, int ranks, hipStream_t s) {
    hipLaunchKernelGGL(k_decide, dim3(V.W), dim3(256), 0, s, V, trial_all, ranks);
}

#ifdef VBA_RESIDENT_STAMPS
// diagnostic builds: per slot the latest stamp of the units' copies (see VBA_KSTAMP, vba_solve_step.h)
#pragma GCC visibility push(hidden)
void fetch_kstamps_chunks(unsigned long long* out);
void fetch_kstamps_cr(unsigned long long* out);
void fetch_kstamps_variants(unsigned long long* out);
#pragma GCC visibility pop
void fetch_kstamps(unsigned long long* out) {
    unsigned long long unit[128];
    fetch_kstamps_chunks(out);
    auto merge = [&]() { for (int k = 0; k < 128; ++k) out[k] = unit[k] > out[k] ? unit[k] : out[k]; };
    fetch_kstamps_cr(unit);
    merge();
#ifdef VBA_VARIANTS
    fetch_kstamps_variants(unit);
    merge();
#endif
}
#endif

}  // namespace vba
