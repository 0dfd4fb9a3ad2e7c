/*
 * vinsat_ba.h -- C ABI of libvinsat_ba.so: the VINSat bundle-adjustment iteration on MI355X.
 *
 * The reference exposes this path as ONE Python function (there is no FFI layer in it):
 *
 *   BA(iter, states, velocities, imu_meas, landmarks, landmarks_xyz, ii, time_idx, intrinsics,
 *      confidences, Sigma, V, lamda_init, poses_gt_eci, initialize=False)
 *        -> (states_new, velocities, lamda_init, last_hessian)
 *   reference: estimation/BA/BA_filtering.py:4-98, called from estimation/od_pipe.py:1038,1040.
 *
 * The entry points below are what a binding for that function needs: the arguments that stay constant
 * over the 20 iterations of a window are uploaded once (observations, per-pose constants), and
 * vba_iterate() is one call of BA().  Plain pointers and sizes only; all host buffers are caller
 * owned, row-major, fp64 unless stated; every call returns 0 on success or a VBA_E* code.
 *
 * A handle owns its device memory and (unless vba_set_stream is used) its HIP stream.  Calls are
 * synchronous on return unless documented otherwise.  One handle per host thread.
 *
 * A handle can hold W independent windows ("batched windows": the reference's outer loop over
 * sequences, estimation/od_pipe.py:1069-1077); every kernel launch then covers all of them.
 */
#ifndef VINSAT_BA_H
#define VINSAT_BA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vba_context* vba_handle;

enum {
    VBA_OK = 0,
    VBA_EINVAL = 1,     /* bad argument (null pointer, size out of range, unsorted input ...) */
    VBA_ENODEV = 2,     /* no usable HIP device */
    VBA_EHIP = 3,       /* a HIP runtime call failed; see vba_last_error() */
    VBA_ESTATE = 4,     /* call order violated (e.g. iterate before upload) */
    VBA_ENOMEM = 5
};

/* bits of the `flags` word returned by vba_iterate (reference behaviour is unchanged by them) */
enum {
    VBA_FLAG_LAMBDA_EXHAUSTED = 1u, /* "lamda too large": no trial improved, last trial kept (BA_filtering.py:75-77) */
    VBA_FLAG_NONFINITE = 2u,        /* NaN/Inf met in the solve or the residuals */
    VBA_FLAG_ZERO_PIVOT = 4u,       /* a diagonal block was numerically singular */
    VBA_FLAG_INDEFINITE = 8u,       /* vba_covariance only: a pivot of the symmetric block elimination was negative (not positive definite) */
    VBA_FLAG_HOST_CHANGED = 1u << 30 /* vba_iterate_resident only: a watched host buffer (vba_set_host_watch) no longer holds the bytes
                                       that were uploaded -- the result was computed from the OLD window: upload again and repeat the call */
};

/* selectors for vba_debug_fetch: intermediates of the LAST vba_iterate call, window 0 unless stated */
enum {
    VBA_DBG_EST = 0,        /* [m,2]   reprojection at the input states (BA_utils.py:30-43), input order */
    VBA_DBG_WEIGHT = 1,     /* [m]     final robust weight w_k (BA_filtering.py:24-25), input order */
    VBA_DBG_H = 2,          /* [n,6,6] per-pose sum of w J^T J, scaled as the reference (BA_filtering.py:32-36) */
    VBA_DBG_B = 3,          /* [n,6]   per-pose sum of w J^T r (BA_filtering.py:44) */
    VBA_DBG_PHI = 4,        /* [n,6,6] d x_hat_i / d x_i of the orbit propagation (BA_utils.py:73-87) */
    VBA_DBG_RPRED = 5,      /* [n-1,7] dynamics residuals (BA_utils.py:476) */
    VBA_DBG_QGRAD = 6,      /* [n,3]   attitude gradient, rotation slots (BA_utils.py:520) */
    VBA_DBG_HQ = 7,         /* [n,3,3,3] attitude Newton blocks (sub, diag, super) rot-rot (BA_utils.py:521-523) */
    VBA_DBG_BANDS = 8,      /* [n,3,9,9] undamped block-tridiagonal system (sub, diag, super) (BA_filtering.py:54) */
    VBA_DBG_RHS = 9,        /* [n,9]   JTr (BA_filtering.py:48) */
    VBA_DBG_DPOSE = 10,     /* [n,9]   solution of the last LM trial (BA_filtering.py:55) */
    VBA_DBG_SCALARS = 11,   /* [8]     c_obs, w_max, init_residual, last trial residual, lamda32 of last trial, sigma, alpha, n_trials */
    VBA_DBG_JG = 12,        /* [m,2,6] reprojection Jacobian (BA_utils.py:44-48), input order */
    /* What the trial kernel of the last call left behind for the NEXT call, as that call will read it (read-only; VBA_ESTATE when
       the call carried nothing: key carry off, or the states replaced behind it): */
    VBA_DBG_NEXT_KEYS = 13,     /* [m,2]   carried keys |uv - est| at the trial states, input order */
    VBA_DBG_NEXT_HIST = 14,     /* [4 + bins] kind (1 exponent digit: 1024 bins, 2 warm: 2048 bins), warm_lo (raw 64 bits), warm shift,
                                   sel_rank[0], then the digit-0 histogram of the next call's parity */
    VBA_DBG_NEXT_BUCKETS = 15,  /* [1 + 2048 cap] cap, then the bin buckets of that parity, bin-major (VBA_ESTATE on handles without
                                   buckets and behind an exponent histogram) */
    VBA_DBG_PART_TRIAL = 16,    /* [8 + trial_stride] observation blocks, pose-chain blocks, long-edge slots, FUSED, TILES, EMIT,
                                   split launches (PART 1 + 2), bucket cap in use (0: none); then the block sums of the last trial:
                                   observation tiles, pose-chain blocks, long edges, unused slots */
    VBA_DBG_PART_NEXT = 17      /* [observation blocks] block sums of |r| at the trial states (carried with the keys) */
};

/* library / device */
int vba_version(void);
/* 1 if the library was built with -DVBA_VARIANTS (make VARIANTS=1 -> libvinsat_ba_variants.so): the solver variants that were
 * measured slower and are kept for comparison only -- three windows per wavefront (vba_set_solver -3), one window per wavefront
 * forming its own blocks, one cyclic-reduction level in front (VBA_OPT_FUSION bit 4), the solve as one grid of waiting blocks
 * (bits 5, 6).  The default build does not carry them: those settings return VBA_EINVAL. */
int vba_has_variants(void);
const char* vba_last_error(void);
int vba_device_count(int* count);

/* Create a context on HIP device `device` able to hold `windows` windows of at most n_max poses and
 * m_max observations each.  Replaces nothing in the reference (it allocates per call). */
int vba_create(int device, int windows, int n_max, int64_t m_max, vba_handle* out);
/* The same with the kernel set named by the caller.  A handle runs one of two kernel sets, fixed at creation because the
 * device memory differs (bin buckets of the carried keys exist in latency mode only):
 *   mode 1  latency mode: few kernels per call (select inside the accumulation, accept test folded into the next call, the
 *           chunk elimination forms its own blocks, the trial kernel forms the step), 64 lanes per pose -- what a handle
 *           whose windows cannot fill the chip by themselves wants;
 *   mode 0  bandwidth mode: streaming kernels with few registers and many windows per launch;
 *   mode -1 (what vba_create passes) chooses by window count and window size -- latency mode up to 38 (50 000 / m_max)^0.7 windows
 *           (exponent 0.46 for windows of more than 50 000 rows; at most 192),
 *           the crossover of the measured sweeps over W = 1 .. 4096 windows of 5 000 / 20 000 / 50 000 / 200 000 rows (bench.py
 *           "batched_sweep").
 * Both modes give the same results to rounding (and the same bits for equal lanes per pose / solver settings). */
int vba_create_mode(int device, int windows, int n_max, int64_t m_max, int mode, vba_handle* out);
/* *mode receives the kernel set of the handle (0 / 1 as above), *chunk the solver partition in use (0: sequential walk). */
int vba_get_mode(vba_handle h, int* mode, int* chunk);
int vba_destroy(vba_handle h);

/* external != 0: run all work of this handle on the caller's HIP stream `hip_stream` (a hipStream_t; NULL is the
 * legacy default stream), e.g. the stream RCCL collectives are ordered against.  external == 0: back to the
 * handle's own stream. */
int vba_set_stream(vba_handle h, void* hip_stream, int external);

/* Choice of the block-tridiagonal solve: chunk = 0 one wavefront walks the whole pose chain (work optimal, used
 * when many windows are batched); chunk in [2,60] cuts the chain into chunks of that many poses that are
 * eliminated in parallel plus a reduced system over the separators; chunk = -1 restores the default
 * (0 for more than 1023 windows -- the walk is a latency chain of ~2.2 ms at 500 poses that only so many windows amortise, see the
 * sweep in DESIGN.md section 3 --; bandwidth-mode handles: chunks of 12 poses (fewer separators: throughput); otherwise chunks of 8 poses
 * (n_max / 3 for chains shorter than 24; more beyond 1032 poses; several latency-mode windows: up to 12 where that keeps the chunk
 * elimination of all windows in one round of the chip, 1024 two-wave blocks) and the reduced
 * system by cyclic reduction, see vba_set_solver2; two levels of ~n^(1/3) beyond 7700 poses).  With chunk = 0 a
 * wavefront walks one window; chunk = -3 makes three windows of equal pose count share a wavefront (no faster on
 * MI355X at any batch size measured, kept for comparison), chunk = -2 forbids it.  All variants agree to rounding. */
int vba_set_solver(vba_handle h, int chunk);
/* Explicit partition: chunks of `chunk` poses; the reduced system over their separators is
 *   chunk2 = 0       walked by one wavefront,
 *   chunk2 in [2,60] cut again into chunks of `chunk2` separators (two levels),
 *   chunk2 = -1      solved by block cyclic reduction (log2 of the separator count levels): inside one workgroup with
 *                    the whole reduced system in LDS up to 23 separators; from 24 on the first level runs as its own
 *                    kernel on one CU per separator pair and the workgroup continues with the halved system
 *                    (at most 128 separators, i.e. chunk >= ceil(n_max / 129)). */
int vba_set_solver2(vba_handle h, int chunk, int chunk2);

/* Orbit integrator of the dynamics factor.  0 (default): one-second RK4 steps, the reference's CPU branch `predict`
 * (BA_utils.py:73-87) -- the parity target.  A gap of more than 64 s between two poses (time_idx of vba_upload_window; a knot
 * every 1000 s makes every later-pass window hold such gaps, od_pipe.py:213-221) is propagated PARALLEL IN TIME: the same
 * one-second steps in ~sqrt(gap) chunks side by side, their start states found by a parareal iteration whose fixed point is the
 * serial chain (stopped when every chunk's end state meets the next chunk's start state to 2^-48 relative), the transition matrix
 * as the ordered product of the chunks' matrices -- equal to the serial chain to rounding (csrc/vba_long.hip).  1: the coarse schedule of `propagate_orbit_dynamics_skip`
 * (BA_utils.py:52-71: steps of 100 s plus one remainder step) that the reference itself switches to when it sees a
 * GPU (`predict_gpu`, BA_filtering.py:16-17); results differ from mode 0 by the integration error. */
int vba_set_integrator(vba_handle h, int hop100);



/* ---- settings a caller of BA() never needs: ONE entry point.  Every option keeps results identical to rounding (most: bit for
 * bit); defaults are chosen from the handle's geometry by measured sweeps (docs/NOTEBOOK.md).  A value an
 * option does not take returns VBA_EINVAL.  The tests and the A/B tools are the users of these. */
enum {
    VBA_OPT_ACCUMULATE_LANES = 1,   /* lanes per pose of the accumulation (4, 8, 16, 32, 64; 0 = from the geometry, ~12 rows per lane):
                                       the shape of its reduction tree -- equal settings give equal bits */
    VBA_OPT_TRIAL_TILES = 2,        /* tiles of 256 rows per observation block of the plain latency-mode trial kernel (0 = automatic, 1, 2,
                                       4, 8): one pass of bin reservations per block; block sums stay per tile: bit-identical for every value */
    VBA_OPT_KEY_CARRY = 3,          /* 1 (default): an accepted trial leaves the next call's |r| keys, histogram and sum |r| behind (it is
                                       evaluated at exactly the states the next call starts from, BA_filtering.py:61-66 / :12-21); 0: every
                                       call recomputes them (same bits) */
    VBA_OPT_WARM_SELECT = 4,        /* exact lower median (torch.median, BA_filtering.py:23) of carried keys: 1 (default) from the warm bins
                                       the producing trial binned them into (latency mode: the bucket of one bin, ranked inside the
                                       accumulation, which also evaluates the accept test of the call in front; else one compaction pass), a
                                       rank outside the bins repeats the select with the exact digits (vba_warm_select_misses); 0: exact digit
                                       passes and a decide launch per call; 2: every warm select misses (test); 3: the select stays a kernel */
    VBA_OPT_WARM_SHIFT = 5,         /* log2 of a warm bin's width in bit patterns (52 = a binade; defaults 44 / 43 latency, 46 bandwidth
                                       mode); the median is exact for every width */
    VBA_OPT_BUCKET_CAP = 6,         /* test knob: keys a bin bucket holds (8 .. allocated; 0 = default): a fuller bin is a miss */
    VBA_OPT_FUSION = 7,             /* bit mask: 0 the trial kernel forms the step of each pose (latency mode), 1 the chunk elimination
                                       forms the blocks of its chunk (latency mode), 2 the sequential walk forms its blocks (bandwidth mode),
                                       3 full-phase assembly in uniform passes; bits 4 .. 6 (one cyclic-reduction level in front; the solve as
                                       one grid of waiting blocks: measured slower) exist in the comparison build only (vba_has_variants).
                                       Default 15, latency-mode handles of many rows 14 / 12 */
    VBA_OPT_CHUNK_WAVES = 8,        /* partitioned solve: 2 (default) = a chunk is eliminated from both ends by two waves, 1 = one wave
                                       left to right (another rounding, ~1e-9 on the step; each deterministic) */
    VBA_OPT_PIVOTING = 9,           /* 0 (default): 9x9 blocks eliminated without row exchanges, every pivot checked against the diagonal
                                       entry it started from, a failed check repeats that solve with pivoting (vba_solver_fallbacks);
                                       1: pivot from the start */
    VBA_OPT_PIPELINE = 10,          /* 1 (default, one-window handles): vba_iterate_resident returns call k once its accept test is known
                                       and has enqueued call k + 1 speculatively (a wrong guess is dropped with the carried keys); bits of
                                       vba_step; vba_debug_fetch refuses after a pipelined call */
    VBA_OPT_SCHEDULE_GRAPH = 11,    /* 1 (default, latency mode): vba_run_schedule replays the launches of its first pass as a hipGraph while
                                       nothing that goes into them has changed (per-call kernel arguments compared exactly); a capture that
                                       fails switches it off for the handle and the pass is launched kernel by kernel; also VBA_NO_GRAPH */
    VBA_OPT_CHAIN_PROFILE = 12,     /* 1: vba_run_schedule records HIP events at the class boundaries of every call (~1 us each, no graph
                                       replay meanwhile): vba_chain_profile */
    VBA_OPT_JACOBIAN_F32 = 13       /* 0 (default): fp64 throughout.  1: the terms of the reprojection Jacobian in fp32 (contract below)
                                       -- the one option that changes results beyond the last bits */
};
/* VBA_OPT_JACOBIAN_F32 = 1, the precision contract.  Only the observation accumulation changes:
 *   fp32: the camera-frame point p_c and d = 1/z rounded to fp32; the camera-frame Jacobian terms -- A = d uv / d p_c (four
 *         non-zeros) and Gr = 2 A hat(p_c) -- evaluated in fp32 (cam_jacobian_f32, vba_math.h).
 *   fp64, unchanged: projection, residual, robust weights, the exact median and c_obs; the weighted products and the per-lane
 *         sums of BOTH parts, H (w A^T A, w A^T Gr, w Gr^T Gr) and b (w A^T r, w Gr^T r), formed from the fp32 terms widened;
 *         the cross-lane reduction, the rotation to the world frame and the assembly; the dynamics, attitude and long-gap
 *         factors; trial residuals, the LM test, the solve.
 *   The H sums are kept in fp64 because a measurement decided it: a pose's 6x6 block is nearly singular along "translate across
 *   the line of sight = rotate" (condition ~1e10 in the landmark-only calls), and fp32 sums moved the first call's states of
 *   the C3 window by 5e-4 (position, relative) and 2e-3 rad against the reference.
 *   Every accumulation shape (VBA_OPT_ACCUMULATE_LANES 4 .. 64, either kernel set) uses the camera-frame form in this mode, so
 *   shapes differ only in summation order.  vba_debug_fetch(VBA_DBG_JG) returns the fp32 terms rotated in fp64 -- the Jacobian
 *   the sums were formed from.  A schedule graph or a speculated call of one mode is never replayed in the other.  It does not
 *   pay on the MI355X; it exists because BASELINE config 5 names it. */
int vba_set_option(vba_handle h, int option, int value);

/* BA_reg (BA_filtering.py:100-210): the BA call with a propagated-covariance prior per pose.
 * vba_upload_prior: states_prior [n,10] (arguments states_prior / velocity_prior of BA_reg: positions and the velocity
 * columns are used), hessian_state [n,6,6] (argument hessian_state_t: information matrix over [position, velocity]).
 * The reference's hessian_rot_t has no effect on its result: the rotation term of prior_gpu (BA_utils.py:626) is
 * quat_coeff (1 - |q_p^T G(q_p) H_rot G(q)^T q|) with G(q)^T q = 0 identically, i.e. a constant -- it is reproduced
 * as that constant (1 per pose in the initial residual mean, 100 per pose in every trial mean, as the reference
 * passes its coefficients) and takes no matrix.
 * vba_set_prior(h, 1): the following vba_step / vba_iterate / vba_run_schedule calls are BA_reg calls (the prior is
 * inactive in landmark-only calls, BA_utils.py:609-612, but still counts in the residual means); 0 (default): BA. */
int vba_upload_prior(vba_handle h, int window, int n, const double* states_prior, const double* hessian_state);
int vba_set_prior(vba_handle h, int on);


/* Carried-key selects that fell outside the warm bins and were repeated with the exact digits (VBA_OPT_WARM_SELECT). */
int vba_warm_select_misses(vba_handle h, int* count);



/* Solves repeated with row pivoting after a failed pivot check (VBA_OPT_PIVOTING). */
int vba_solver_fallbacks(vba_handle h, int* count);

/* Observation rows of window `window`: landmarks_xyz [m,3] (ECI km), landmarks (uv) [m,2] px,
 * confidences [m], ii [m] pose index of each row (BA arguments landmarks_xyz, landmarks, confidences, ii:
 * BA_filtering.py:4; ii is int64 as at BA_filtering.py:35).  n is the number of poses the indices refer to.
 * Uploading with a pose count different from the window's current one starts a new window: the other upload
 * (pose constants / observations) and the states must follow before the next step.
 * The rows are packed into pinned memory and sent with one asynchronous copy on the handle's stream (ordered in
 * front of the kernels that read them); the caller's arrays may be reused as soon as the call returns. */
int vba_upload_observations(vba_handle h, int window, int n, int64_t m, const double* landmarks_xyz,
                            const double* landmarks_uv, const double* confidences, const int64_t* ii);

/* The longest gap between two consecutive poses that vba_upload_window accepts, in seconds (2^20 s, ~12 days).  A gap is walked
 * in one-second RK4 steps; a long one is cut into at most 64 chunks of L >= gap / 64 steps (csrc/vba_long.hip), and a gap the
 * window's chain pool has no room for takes one lane's serial walk -- the limit keeps either within 2^20 steps of one lane.
 * The reference's driver inserts a knot every 1000 s (od_pipe.py:213-221): its gaps never come near it. */
enum { VBA_MAX_GAP = 1 << 20 };

/* Per-pose constants of window `window`: intrinsics [n,4] = fx,fy,cx,cy; cumrot_last [n,4] =
 * imu_meas[0,:,-1,6:10], the attitude increment over the gap that follows each pose (the only part of
 * imu_meas the reference's CPU path reads, BA_utils.py:295); time_idx [n] seconds, strictly increasing, no two consecutive
 * ones more than VBA_MAX_GAP apart (VBA_EINVAL otherwise, before anything is uploaded). */
int vba_upload_window(vba_handle h, int window, int n, const double* intrinsics, const double* cumrot_last,
                      const int64_t* time_idx);

/* Device-resident state of a window: [n,10] = p(3) q(4, scalar last) v(3); lamda is the LM damping.
 * window == -1 in vba_set_states gives every window the same states (equal pose counts required). */
int vba_set_states(vba_handle h, int window, const double* states, double lamda);
int vba_get_states(vba_handle h, int window, double* states, double* lamda, double* last_hessian /*[81] or NULL*/,
                   int* n_trials /*or NULL*/, unsigned* flags /*or NULL*/);

/* The same for every window of the handle at once -- the batch dimension of BA()'s `states [bsz, n, 10]` (BA_filtering.py:14):
 * states [W][n_max][10] (rows beyond a window's pose count are ignored / left untouched), lamda [W], last_hessian [W][81],
 * n_trials [W], flags [W] (each of the last three may be NULL).  One copy each way instead of W. */
int vba_set_states_all(vba_handle h, const double* states, const double* lamda);
int vba_get_states_all(vba_handle h, double* states, double* lamda, double* last_hessian, int* n_trials, unsigned* flags);

/* One BA() call (BA_filtering.py:4-98) on EVERY window of the handle, states and lamda device resident:
 * states <- states_new, lamda <- lamda_out.  `iter` selects alpha and Sigma (BA_filtering.py:22,26);
 * `initialize` != 0 is the landmark-only phase (BA_utils.py:463-466).  Synchronous. */
int vba_step(vba_handle h, int iter, int initialize);

/* ncalls consecutive BA() calls on every window -- the driver's loop `for iter in range(20): BA(iter, ...)`
 * (od_pipe.py:1036-1040) -- issued as one host call: iters[c] / inits[c] are the `iter` and `initialize` arguments
 * of call c.  The calls are chained on the device (a window that needs further LM trials in some call stalls there
 * and is finished by the host before the rest is re-issued); the results are bit-identical to ncalls vba_step
 * calls.  *trials_total (optional) receives the number of LM trials issued.  Synchronous. */
int vba_run_schedule(vba_handle h, int ncalls, const int* iters, const int* inits, int* trials_total);

/* Convenience: set_states(window 0) + step + get_states(window 0); the exact shape of one BA() call. */
int vba_iterate(vba_handle h, int iter, int initialize, double lamda_in, const double* states_in,
                double* states_out, double* lamda_out, double* last_hessian, int* n_trials, unsigned* flags);

/* The same call when the states argument IS the result of the previous vba_iterate / vba_iterate_resident /
 * vba_run_schedule on this handle (the driver loop `states = BA(iter, states, ...)`, od_pipe.py:1036-1040) and lamda_in
 * the lamda it returned: nothing is uploaded, the device-resident states and damping are used, and the call starts
 * from the keys the last accepted trial left behind (VBA_OPT_KEY_CARRY).  Same bits as vba_iterate. */
int vba_iterate_resident(vba_handle h, int iter, int initialize, double* states_out, double* lamda_out,
                         double* last_hessian, int* n_trials, unsigned* flags);

/* vba_iterate as the FIRST call of a driver loop whose following calls are vba_iterate_resident (a new window, or states the caller
 * changed): the states go up and the call is served like a resident one -- returned as soon as its accept test is known, the next
 * call enqueued behind it (VBA_OPT_PIPELINE); the watched host buffers are compared as in a resident call (VBA_FLAG_HOST_CHANGED).
 * Same bits as vba_iterate.  A caller that replaces the states before every call
 * should use vba_iterate: there the speculated call would be waited for and dropped each time. */
int vba_iterate_open(vba_handle h, int iter, int initialize, double lamda_in, const double* states_in, double* states_out,
                     double* lamda_out, double* last_hessian, int* n_trials, unsigned* flags);

/* Host buffers of the caller whose content was uploaded (e.g. the ndarray arguments ii / time_idx of BA()) and that the caller
 * might edit in place: every vba_iterate_resident compares `live` with the reference `copy` (bytes each, both must stay valid;
 * 8 slots -- one per array argument of BA() --, live == NULL clears one) while the device works -- from 64 kB of watched bytes on a helper
 * thread of the handle, beside the enqueue of the speculated call -- and reports a difference as VBA_FLAG_HOST_CHANGED. */
int vba_set_host_watch(vba_handle h, int slot, const void* live, const void* copy, int64_t bytes);
/* Speculated calls of the pipelined driver loop that were used / dropped (VBA_OPT_PIPELINE). */
int vba_pipeline_stats(vba_handle h, int* hits, int* discards);

/* Copy an intermediate of the last step of `window` to host memory; *count receives the number of
 * doubles written (capacity is checked). */
int vba_debug_fetch(vba_handle h, int window, int what, double* out, int64_t capacity, int64_t* count);

/* ---- per-pose marginal covariances.  For every window, at the RESIDENT states (what the last call returned), the full-phase
 * system a vba_step(h, iter, 0) would factor there: the observation, dynamics and attitude factors (long gaps and the integrator as
 * set), and the BA_reg prior if vba_set_prior(h, 1) is on.
 *   A      the undamped bands as VBA_DBG_BANDS defines them; damped != 0 adds float32(lamda_resident) I, the damping the next
 *          call's first trial would use (BA_filtering.py:54) -- that matrix is the reference's JTwJ;
 *   A^     (A + A^T) / 2: A is symmetric but for the 3x3 rot-rot diagonal blocks Sigma Hd of the attitude factor;
 *   diag   [W][n_max][9][9]  Sigma_ii = (A^-1)_ii, exactly symmetric (one triangle computed, mirrored); zeros for rows beyond n,
 *          on both paths;
 *   super  [W][n_max][9][9]  Sigma_i,i+1 = (A^-1)_i,i+1 for i < n - 1 (zeros for i = n - 1 and for rows beyond n);
 *   flags  [W]  VBA_FLAG_ZERO_PIVOT: numerically singular (e.g. the velocities of a one-pose window, undamped): that window's blocks
 *               are NaN; VBA_FLAG_INDEFINITE: the blocks are returned but are no covariance; VBA_FLAG_NONFINITE as elsewhere.
 * Any of diag / super / flags may be NULL.  Coordinates are those of the step dpose: [dp (km), dtheta, dv (km/s)], where dtheta
 * linearises a rotation of angle 2 |dtheta| (the retraction q (x) [dtheta, 1], normalised): the attitude sigma in radians is
 * 2 sqrt(Sigma_theta).  The robust weights are normalised by their maximum w_max, so Sigma is a covariance up to a scale factor
 * that this library does not estimate (no a-posteriori variance factor).
 * Algorithm: block LDL^T and selected inversion (csrc/vba_cov.hip), fp64; the path follows vba_set_solver: chunk 0 one wavefront
 * walks each window, a chunked setting eliminates the same chunks in parallel and inverts the separator system (the two agree to
 * rounding, ~1e-10).  The system is built by the kernels of a call's front into scratch of the query.  The query changes nothing: states, lamda, flags, carried keys, schedule
 * graphs and the long-gap chain pool stay as they were, the following calls give the same bits; a speculated call of the
 * pipelined loop is dropped as a mismatched resident call drops it.  Scratch is allocated on the first query (about
 * 700 doubles per pose and 5 per observation row, per window, plus a copy of the long-gap chain pool).  VBA_ESTATE before every window has states,
 * and on observation-sharded handles.  Synchronous. */
int vba_covariance(vba_handle h, int iter, int damped, double* diag, double* super, unsigned* flags);
/* HIP-event time of the last vba_covariance on the handle's stream (front + inversion), milliseconds. */
int vba_last_covariance_ms(vba_handle h, float* ms);

/* ---- observation reliability: per row, how much of the fit hangs on it (leverage) and how far its residual lies from what the
 * model predicts for it (standardised residual, Baarda's w-test).  At the RESIDENT states, for a full-phase call BA(iter), with
 * the system of vba_covariance(h, iter, damped, ...): the same A^, the same damping and symmetrisation rules, Sigma = A^^-1.  For
 * observation row k of pose i = ii[k]:
 *   J_k [2,6]  the reprojection Jacobian over [dp, dtheta], as VBA_DBG_JG;
 *   r_k [2]    the residual uv - est;
 *   w_k        the final robust weight (w_raw / w_max) conf, as VBA_DBG_WEIGHT;
 *   S_i        Sigma_ii[:6, :6];
 *   P_k        w_k J_k S_i J_k^T (2x2); only its symmetric part is formed;
 *   leverage [W][m_max]  tr(P_k), in [0, 2); the redundancy of the row is 2 - leverage;
 *   wtest    [W][m_max]  sqrt(w_k r_k^T (I - P_k)^-1 r_k), the 2x2 inverse in closed form.  (I - P_k) / w_k is the covariance of the
 *                        row's residual under the linearised model.  Unitless, in units of the same unestimated variance factor
 *                        that vba_covariance documents;
 *   pose_stats [W][n_max][3]  per pose: the sum of leverage over its rows (= tr(S_i H_i), H_i as VBA_DBG_H), the largest finite
 *                        wtest of its rows, the count of its rows with w_k > 0; poses without rows get 0, 0, 0;
 *   flags [W]  the flags of the covariance step (see vba_covariance).
 * Both row arrays are in the INPUT order of the rows (the order of vba_upload_observations).  Degenerate rows are flagged in the
 * value, not hidden: w_k == 0 gives leverage = 0, wtest = 0; det(I - P_k) <= 0 or a negative quadratic form gives wtest = NaN; a
 * window flagged VBA_FLAG_ZERO_PIVOT / VBA_FLAG_NONFINITE has no Sigma: wtest = NaN for every row of it (those of weight zero
 * included), leverage = NaN for its rows of non-zero weight (and so is the pose's sum).
 * Any output may be NULL, in every combination; rows beyond a window's m and poses beyond its n are left untouched.
 * Precision: with VBA_OPT_JACOBIAN_F32 = 1 the row pass still evaluates J_k in fp64 (the query is a diagnostic, not the hot loop);
 * Sigma comes from the system the handle builds in its mode, as in vba_covariance.
 * Algorithm: the shadow front and the selected inversion of vba_covariance into the scratch of the query, then one streaming pass
 * over the rows (csrc/vba_rel.hip): no atomics, equal settings give equal bits, and a window has the same bits alone and in a batch.
 * The promises are those of vba_covariance: the query changes nothing (states, lamda, flags, carried keys, schedule graphs, long-gap
 * pool), drops a speculated pipelined call as a mismatched resident call does, returns VBA_ESTATE before every window has states
 * and on observation-sharded handles, and is synchronous.  Scratch beyond the covariance query's is allocated on the first
 * reliability query: two doubles and an index per observation row and window, whichever outputs are asked for (W = 4096 windows
 * of 50 000 rows: 1.6 GB per row array); VBA_ENOMEM if that fails.  Only the non-NULL outputs are copied to the host. */
int vba_reliability(vba_handle h, int iter, int damped, double* leverage, double* wtest, double* pose_stats, unsigned* flags);
/* HIP-event time of the last vba_reliability on the handle's stream (front + inversion + row pass), milliseconds. */
int vba_last_reliability_ms(vba_handle h, float* ms);

/* ---- outlier power: per row, how large an error in it could pass the w-test unnoticed (minimal detectable bias), how far such an
 * error would move the pose (external reliability) and how far the row itself moves it (deletion influence); per pose and per
 * window, the weighted residual sum, the redundancy and the a-posteriori variance factor of the fit.  At the RESIDENT states, for a
 * full-phase call BA(iter), with the system of vba_covariance(h, iter, damped, ...): the same A^, the same damping and
 * symmetrisation rules, Sigma = A^^-1.  J_k, r_k, w_k, S_i and P_k are those of vba_reliability, for observation row k of pose
 * i = ii[k]; further
 *   R_k        I - P_k (2x2); only its symmetric part is formed.  R_k / w_k is the covariance of the row's residual;
 *   B_k [6,2]  w_k S_i J_k^T: the change of the pose's [dp, dtheta] per pixel of error in the row; B_p its rows 0..2, B_t rows 3..5;
 *   ncp > 0    the non-centrality parameter of the test, the caller's choice (17.075 for a 0.1 % test of 80 % power);
 *   crit > 0   the critical value wtest is counted against, the caller's choice (+inf counts nothing);
 *   mdb      [W][m_max]  sqrt(ncp / (w_k mu_min(R_k))), pixels: the minimal detectable bias along the direction the test sees
 *                        worst.  mu_min, the smaller eigenvalue of the symmetric 2x2, is (tr - sqrt((a - d)^2 + 4 b^2)) / 2:
 *                        continuous in its inputs, no tie rule;
 *   ext_pos  [W][m_max]  sqrt(ncp / w_k  mu_max(B_p^T B_p, R_k)), km: the largest displacement of the pose's position that a bias
 *                        at the detection limit causes.  mu_max(M, R) is the larger root of det(M - mu R) = 0, a quadratic in
 *                        closed form (csrc/vba_power_math.h); no eigenvector of R_k is formed, so the value stays continuous
 *                        where the eigenvalues of R_k coincide and no row is excluded;
 *   ext_att  [W][m_max]  2 sqrt(ncp / w_k  mu_max(B_t^T B_t, R_k)), radians by the 2 |dtheta| convention of vba_covariance;
 *   del_pos  [W][m_max]  | B_p R_k^-1 r_k |, km: under the linearised model, the distance the pose's position moves if row k is
 *                        removed;
 *   pose_fit [W][n_max][4]  per pose: Omega_i = sum of w_k |r_k|^2 over its rows; the sum of its leverages (the bits of
 *                        vba_reliability's pose_stats[..., 0]); the largest finite ext_pos of its rows; the count of its rows
 *                        with wtest > crit.  Poses without rows get 0, 0, 0, 0;
 *   fit      [W][8]      per window: Omega = sum of Omega_i; m_eff, the number of rows with w_k > 0; t, the sum of the
 *                        leverages; rho = 2 m_eff - t, the redundancy; s0sq = Omega / rho (NaN if rho <= 0); the largest finite
 *                        wtest (the maximum of vba_reliability's wtest, bit for bit); the count of rows with wtest > crit; the
 *                        largest finite ext_pos;
 *   flags [W]  the flags of the covariance step (see vba_covariance).
 * What s0sq is and is not.  It is the a-posteriori variance factor of the OBSERVATION class -- the 2 m_eff reprojection residuals
 * against the parameters they determine --, in the units of the normalised weights (w_raw / w_max) conf: with s0 = sqrt(s0sq),
 * s0^2 Sigma is the covariance vba_covariance leaves unscaled, s0 scales the sigmas, mdb and ext_* linearly and wtest inversely
 * (wtest / s0 is what compares with a critical value of the standard normal / chi distribution).  It is NOT a variance factor
 * of the whole system: the orbit and attitude factors carry weights of 1e4 .. 1e6 (times 100 on the velocities), which makes
 * them constraints in all but name; the redundancy of such an edge is a difference of two numbers equal to rounding in a system
 * of condition ~1e11, so no variance component of those classes is computed.  They enter every number here through Sigma only.
 * The row arrays are in the INPUT order of the rows.  Degenerate rows are flagged in the value: w_k == 0 gives mdb = +inf,
 * ext_pos = ext_att = del_pos = 0; det R_k <= 0 or mu_min(R_k) <= 0 gives NaN in all four; a window flagged VBA_FLAG_ZERO_PIVOT /
 * VBA_FLAG_NONFINITE has no Sigma: NaN in all four for every row of it (those of weight zero included); its Omega and m_eff
 * stand, t, rho and s0sq are NaN if a row of it has weight.
 * Any output may be NULL, in every combination; rows beyond a window's m and poses beyond its n are left untouched.  VBA_EINVAL
 * if ncp is not positive and finite or crit is not positive.  Precision: as vba_reliability (J_k in fp64 whatever
 * VBA_OPT_JACOBIAN_F32 says).
 * Algorithm: the shadow front and the selected inversion of vba_covariance into the scratch of the query, one streaming pass over
 * the rows with the mapping and the leverage / w-test arithmetic of vba_reliability, and one wavefront per window for the totals
 * (csrc/vba_power.hip): no atomics, equal settings give equal bits, a window has the same bits alone and in a batch.  The
 * promises are those of vba_covariance: the query changes nothing (states, lamda, flags, carried keys, schedule graphs, long-gap
 * pool), drops a speculated pipelined call as a mismatched resident call does, returns VBA_ESTATE before every window has states
 * and on observation-sharded handles, and is synchronous.  Scratch beyond the reliability query's (which is allocated too: its
 * index per row is read) is allocated on the first query: four doubles per observation row and window, whichever outputs are asked
 * for; VBA_ENOMEM if that fails.  Only the non-NULL outputs are copied to the host. */
int vba_outlier_power(vba_handle h, int iter, int damped, double ncp, double crit, double* mdb, double* ext_pos, double* ext_att,
                      double* del_pos, double* pose_fit, double* fit, unsigned* flags);
/* HIP-event time of the last vba_outlier_power on the handle's stream (front + inversion + row pass + window totals), milliseconds. */
int vba_last_outlier_power_ms(vba_handle h, float* ms);

/* ---- data snooping (Baarda): ACT on the w-test.  Per pose, the observation row whose w-test exceeds a critical value by most is
 * rejected ON THE DEVICE: its confidence in the device observation block becomes 0, its original value and a mask byte are kept.
 * Without it the only way to reject a row is to zero its confidence on the host and call vba_upload_observations again, which
 * packs and uploads every row of the window.
 * System and w-test: exactly the system of vba_reliability(h, iter, damped, ...) at the RESIDENT states; wtest of every row has the
 * bits vba_reliability would return at that moment (the same row pass with the same mapping, csrc/vba_rowpass.h).
 *   crit > 0   the critical value, in wtest's own units: a caller who wants a quantile of the normal distribution passes
 *              quantile * s0 (s0 of vba_outlier_power); +inf rejects nothing;
 *   candidates of pose i: its rows with current weight w_k > 0, wtest finite and wtest > crit.  A row whose wtest is NaN is never
 *              rejected;
 *   cnt_i      the pose's rows of non-zero weight;
 *   mode 0     snooping: the candidate with the largest wtest is rejected -- ties go to the smallest input row index -- and only
 *              if cnt_i - 1 >= min_rows;
 *   mode 1     every flagged row: all candidates of the pose are rejected if cnt_i - #candidates >= min_rows; otherwise the rule
 *              of mode 0 applies to that pose;
 *   min_rows >= 0  the rows of non-zero weight a pose keeps at least;
 *   a window the covariance step flagged VBA_FLAG_ZERO_PIVOT, VBA_FLAG_NONFINITE or VBA_FLAG_INDEFINITE rejects nothing;
 *   rejected [W][m_max]  bytes, 1 = rejected, in the INPUT order of the rows, CUMULATIVE over the calls since the window's rows
 *              were uploaded; the whole array is written, bytes beyond a window's m are 0;
 *   counts [W][2]  rows rejected by this call, rows rejected in total;
 *   flags [W]  the flags of the covariance step (see vba_covariance).
 * A rejected row STAYS in the window with weight zero, exactly as the reference treats a row of confidence 0: it still counts in
 * the median of |r| (BA_filtering.py:23) and in m, the divisor of the residual means.  Nothing is compacted.
 * The promise: from the call's return on the handle gives, bit for bit, what a handle would give on which
 * vba_upload_observations had been called with those confidences zeroed and the same states and lamda set -- calls, schedules,
 * graph replays and all three queries.  So the call is a boundary as an upload is: carried keys are dropped, a speculated call of
 * the pipelined loop is dropped, schedule graphs are matched again; states, lamda and flags are untouched and the permutation
 * stays valid -- also when nothing is rejected.
 * vba_snoop_restore puts the original confidences of `window` (-1: every window) back and clears its mask, a boundary of the
 * same kind.  vba_upload_observations of a window clears that window's mask: those are new rows.  vba_get_rejected returns the
 * cumulative mask (as `rejected` above) and the totals [W]; either may be NULL.
 * VBA_EINVAL: crit not positive or NaN, mode not 0 / 1, min_rows < 0.  VBA_ESTATE before every window has states, and on
 * observation-sharded handles.  Scratch beyond the reliability query's (allocated too: its wtest array and its index per row are
 * used) is allocated by the first vba_snoop: a double and a byte per observation row and window, an int per pose; VBA_ENOMEM if
 * that fails.  Synchronous; only the non-NULL outputs are copied to the host.
 * Algorithm: the shadow front and the selected inversion of vba_covariance, then ONE launch (csrc/vba_snoop.hip): the row pass of
 * vba_reliability, a segmented arg-max per pose by a butterfly of fixed shape, and the stores of the lanes that own rejected
 * rows.  No atomics; equal settings give equal bits; a window has the same result alone and in a batch. */
int vba_snoop(vba_handle h, int iter, int damped, double crit, int mode, int min_rows,
              unsigned char* rejected /*[W][m_max], input order, cumulative; or NULL*/,
              int* counts /*[W][2]: rejected by this call, rejected in total; or NULL*/,
              unsigned* flags /*[W] or NULL*/);
int vba_snoop_restore(vba_handle h, int window /* -1: every window */);
int vba_get_rejected(vba_handle h, unsigned char* rejected /*[W][m_max]*/, int* totals /*[W]*/);
/* HIP-event time of the last vba_snoop or vba_snoop_scaled on the handle's stream (front + inversion + the snooping launches),
 * milliseconds. */
int vba_last_snoop_ms(vba_handle h, float* ms);

/* ---- scaled data snooping: vba_snoop with a critical value PER WINDOW, quantile * s0 of the window's own fit, formed on the
 * device behind ONE covariance step.  A quantile of the normal distribution compares with wtest / s0 (see vba_outlier_power),
 * and s0 is one number per window: with vba_snoop a caller needs vba_outlier_power, a host multiply and one vba_snoop per
 * distinct critical value -- two covariance steps for one window, W + 1 for a batch.
 * For window w:
 *   s0sq [W]       the variance factor of the observation class at the resident states: the bits of fit[w][4] that
 *                  vba_outlier_power(h, iter, damped, ...) would return at that moment;
 *   crit_used [W]  quantile * sqrt(s0sq[w]): the IEEE double product of the correctly rounded square root (what
 *                  numpy.float64(quantile) * numpy.sqrt(s0sq) gives on the host).  NaN if s0sq[w] is NaN or not > 0 -- a window
 *                  without redundancy, without Sigma, or with every confidence zero -- and such a window rejects nothing;
 *   candidates, mode, min_rows, the tie rule, barred windows, rejected, counts, flags and the kept confidences are exactly those
 *                  of vba_snoop at crit = crit_used[w].
 * The contract in one sentence: for every window the handle ends in the state, with the mask and the counts, that
 * vba_outlier_power, a host multiply and vba_snoop(crit_used[w]) would leave on a handle that holds only that window -- bit for
 * bit, whatever the batch.
 * The promise and the boundary behaviour are vba_snoop's, also when nothing is rejected; vba_snoop_restore, vba_get_rejected and
 * vba_upload_observations treat the mask as they do after vba_snoop, and calls of the two may be mixed.
 * VBA_EINVAL: quantile not positive or NaN (+inf rejects nothing), mode not 0 / 1, min_rows < 0.  VBA_ESTATE before every window
 * has states, and on observation-sharded handles.  Scratch beyond vba_snoop's: three doubles per pose and two per window,
 * allocated by the first call; VBA_ENOMEM if that fails.  Synchronous; only the non-NULL outputs are copied to the host;
 * vba_last_snoop_ms reports this call as well.
 * Algorithm: the shadow front and the selected inversion of vba_covariance once, then three launches (csrc/vba_snoop.hip): the row
 * pass of vba_snoop, which stores every wtest and, per pose, the sums vba_outlier_power's row pass forms (in its order and with
 * its rounding); one wavefront per window for the totals, in the order of vba_outlier_power's, s0sq and the critical value; and a
 * pass over the stored wtests with vba_snoop's butterfly, decision and stores.  No atomics; equal settings give equal bits; a
 * window has the same result alone and in a batch. */
int vba_snoop_scaled(vba_handle h, int iter, int damped, double quantile, int mode, int min_rows,
                     unsigned char* rejected /*[W][m_max], input order, cumulative; or NULL*/,
                     int* counts /*[W][2]: rejected by this call, rejected in total; or NULL*/,
                     double* crit_used /*[W] or NULL*/, double* s0sq /*[W] or NULL*/, unsigned* flags /*[W] or NULL*/);

/* Timing of the last vba_step measured with HIP events on the handle's stream, milliseconds. */
int vba_last_step_ms(vba_handle h, float* ms);

/* Same work as vba_step, with every kernel class bracketed by HIP events on the handle's stream (first LM
 * trial only).  ms[VBA_NKERNELS] receives the durations in the order of the VBA_K_* enum; a class that did
 * not run (dynamics in the landmark-only phase) reports 0.  VBA_K_BEGIN has no kernel any more: it is the
 * interval between two back-to-back event records, i.e. the measurement overhead contained in every class.
 * In the landmark-only phase the first trial's solve rides in the assemble class (k_assemble<true>). */
enum { VBA_K_BEGIN = 0, VBA_K_RESIDUAL, VBA_K_SELECT, VBA_K_ACCUMULATE, VBA_K_DYNAMICS, VBA_K_ASSEMBLE, VBA_K_SOLVE,
       VBA_K_TRIAL, VBA_K_DECIDE, VBA_NKERNELS };
int vba_step_profiled(vba_handle h, int iter, int initialize, float* ms);

/* Graphs captured / replays of vba_run_schedule so far (VBA_OPT_SCHEDULE_GRAPH). */
int vba_schedule_graph_stats(vba_handle h, int* captures, int* replays);

/* Class times of the CHAINED schedule (VBA_OPT_CHAIN_PROFILE on): ms[3] = summed milliseconds of the classes {accumulate (with
 * the select / accept test folded into it, or launched in front of it), solve, trial}, launches[3] = how many intervals each sum
 * holds (a landmark-only call whose step the trial kernel forms has no solve interval); reset != 0 clears the sums. */
int vba_chain_profile(vba_handle h, double* ms, int64_t* launches, int reset);

/* ---- observation-sharded multi-GPU operation (one rank per GPU, window 0 only) -------------------------
 * Each rank uploads its slice of the observation rows and the full per-pose constants.  One BA() call is
 * the sequence   stage1 -> all-gather -> stage2 -> all-gather -> stage3 -> all-gather -> stage4 [-> stage3 ...]
 * where the exchanges are done by the caller (RCCL through torch.distributed) on DEVICE buffers; all
 * stage calls are asynchronous on the handle's stream except stage4.
 */
/* number of doubles each rank contributes to the second exchange: per-pose blocks + gradient + scalars */
int64_t vba_sh_partial_count(int n);
/* stage 1: residuals of the local rows at the resident states; writes 2*m_local |r| values to d_abs_local.
 * m_total = number of observation rows over all ranks (fixes the median rank and the residual means). */
int vba_sh_stage1(vba_handle h, int iter, int initialize, int64_t m_total, double* d_abs_local);
/* stage 2: exact lower median over the gathered |r| of all ranks, robust weights and the local per-pose
 * accumulation; writes vba_sh_partial_count(n) doubles to d_partial_local.  d_abs_all holds count_all values of
 * which 2*m_total are keys; slots that pad unequal shards must hold +inf (they sort above every key). */
int vba_sh_stage2(vba_handle h, const double* d_abs_all, int64_t count_all, double* d_partial_local);
/* stage 3: reduce the R gathered partials in rank order, build + solve the system (every rank redundantly),
 * retract, and evaluate the local part of the trial residual into d_trial_local[0..1].  d_partial_all == NULL
 * runs another LM trial (next damping) on the system already built. */
int vba_sh_stage3(vba_handle h, const double* d_partial_all, int ranks, double* d_trial_local);
/* stage 4: accept test on the gathered trial sums (2 doubles per rank); *done = 1 when the LM loop ended
 * (states/lamda updated).  Synchronous. */
int vba_sh_stage4(vba_handle h, const double* d_trial_all, int ranks, int* done);
/* The same protocol with the three exchanges issued by the LIBRARY: RCCL all-gathers on the handle's stream between the
 * stage kernels -- one host call per BA() call and one host synchronisation per LM trial instead of four stage calls and
 * three collectives dispatched by the caller.  RCCL is resolved at run time from `rccl_path` (a process that also uses
 * torch.distributed names the copy it has loaded already; /opt/rocm/lib/librccl.so otherwise); libvinsat_ba.so itself does
 * not link it.
 *   vba_sh_unique_id: rank 0 draws the 128-byte id (ncclGetUniqueId) and hands it to the other ranks by any means;
 *   vba_sh_comm_init: every rank of the window joins (ncclCommInitRank: collective, returns when all have);
 *   vba_sh_call:      one BA() call (BA_filtering.py:4-98) on the sharded window (protocol below); this rank's rows
 *                     (vba_upload_observations) must number at most ceil(m_total / ranks);
 *   vba_sh_comm_destroy: leaves the communicator (vba_destroy does it as well).
 * Protocol of the library-issued form (vba_sh_set_protocol; default 1):
 *   1  carried keys.  An accepted trial is evaluated at the states the next call starts from, so the trial kernel of every rank
 *      leaves the |r| keys of ITS rows behind in per-bin buckets, with their warm histogram (VBA_OPT_WARM_SELECT) and block sums,
 *      written straight into the exchange buffer.  Per call: all-gather A [histogram | block sums] (~12 kB per rank at 500 / 50k;
 *      the next call's first kernel evaluates the accept test on it and resolves the bin of the global median from the summed
 *      histograms), all-gather B [this rank's bucket of that bin] (<= 8 kB), all-gather C [per-pose normal equations, written
 *      by the accumulation in place].  No pass over all keys, no glue launches; the calls of a schedule are chained on the device
 *      and every rank enqueues the same collectives whether a call runs or skips, one host synchronisation per schedule.  A call
 *      whose select misses (median outside the binned range, a bucket overflowed) is repeated with protocol 0's front; a trial
 *      that is not cleanly accepted is finished by the ordinary LM loop with the trial sums gathered per round.  All decisions
 *      are taken on gathered data: every rank takes the same.  Needs a latency-mode handle with its default kernel fusion,
 *      created for exactly m_max = ceil(m_total / ranks) rows on every rank (the exchange buffers follow the handle's geometry);
 *      any other handle takes protocol 0.
 *   0  the round-3 protocol: every call recomputes its keys and gathers all of them (16 B per observation). */
int vba_sh_unique_id(const char* rccl_path, void* id128);
int vba_sh_comm_init(vba_handle h, const char* rccl_path, const void* id128, int nranks, int rank);
int vba_sh_call(vba_handle h, int iter, int initialize, int64_t m_total, int* n_trials);
/* ncalls consecutive BA() calls on the sharded window as one host call (the driver's loop od_pipe.py:1036-1040), chained on the
 * device in protocol 1; *trials_total: LM rounds issued.  vba_sh_call is the schedule of one call. */
int vba_sh_run_schedule(vba_handle h, int ncalls, const int* iters, const int* inits, int64_t m_total, int* trials_total);
int vba_sh_set_protocol(vba_handle h, int carried_keys);
/* bytes this rank contributes to the first exchange of a call; calls repeated after a missed select; calls finished by the LM loop */
int vba_sh_stats(vba_handle h, int64_t* bytes_first_exchange, int64_t* fallbacks_miss, int64_t* fallbacks_lm);
int vba_sh_comm_destroy(vba_handle h);

/* ---- host-side helpers of the driver around BA() (streaming_version, od_pipe.py:911-1062).  No device is
 * involved and no handle is needed: the serial recurrences of the driver's data preparation, which as interpreted loops cost more
 * than the BA calls they sit between.
 *   vba_host_orbit_chain:   `steps` one-second RK4 steps of the J2 orbit dynamics from x0 = [p (km), v (km/s)] -- the dead
 *                           reckoning across the gap between two batches (propagate_dynamics_init, BA_utils.py:114-129; RK4 :901-912;
 *                           driver od_pipe.py:1011, 1052); out[k] = the state after k + 1 steps.
 *   vba_host_quat_chain:    running Hamilton product (scalar last, BA_utils.py:992-1000) out[k] = q0 (x) r[0] (x) ... (x) r[k]
 *                           (q0 NULL: out[k] = r[0] (x) ... (x) r[k]) -- the attitude of the same dead reckoning
 *                           (propagate_rotation_dynamics_init, BA_utils.py:105-112).  Every product and sum is rounded on its own in
 *                           the order of the reference's expression: the bits of the array code.
 *   vba_host_gap_rotations: the attitude increment accumulated over the gap after each pose, cum[i] = r[t_i] (x) ... (x)
 *                           r[t_{i+1} - 1] with r[N,4] the per-second increments exp(dt * omega) and cum[T - 1] the identity
 *                           (precompute_cum_rotations, BA_utils.py:278-288, of which only [..., -1] is read, :295; driver
 *                           od_pipe.py:945-961).  Same rounding rule. */
int vba_host_orbit_chain(const double* x0 /*[6]*/, int steps, double* out /*[steps,6]*/);
int vba_host_quat_chain(const double* q0 /*[4] or NULL*/, const double* r /*[K,4]*/, int K, double* out /*[K,4]*/);
int vba_host_gap_rotations(const double* r /*[N,4]*/, int64_t N, const int64_t* time_idx /*[T]*/, int T, double* cum /*[T,4]*/);

/* ---- the per-row part of the driver's data preparation ON THE DEVICE (no handle; synchronous; a process-wide workspace).
 * For every detection row det[k] = [frame (s), lon (deg), lat (deg), u, v, confidence] (sim/nadir_sim.py:236, 256) with pose index
 * ii[k] into the T ground-truth poses (pos_gt [T,3] ECI km, rot_gt [T,9] row-major camera->inertial rotation):
 *   xyz[k]  = the landmark in ECI km at the frame's second (latlon_to_eci, BA_utils.py:1238-1251 with the ellipsoid of :1221-1236 and the
 *             Greenwich angle of :1172-1218),
 *   proj[k] = its reprojection at that ground-truth pose (landmark_project, BA_utils.py:30-43; depth clamped at 0.1 km, :13),
 *   mask[k] = the driver's outlier test (od_pipe.py:930): 0 < proj < (4700, 2600), |proj - uv| < 1000 px, confidence > 0.8.
 * Agrees with the host path (vinsat_amd/od_pipe.py without a device, which is bit-identical to the reference's arrays) to rounding:
 * the device library's sin / cos are not the host's. */
int vba_prepare_rows(int device, int64_t M, const double* det /*[M,6]*/, const int64_t* ii /*[M]*/, int T, const double* pos_gt /*[T,3]*/,
                     const double* rot_gt /*[T,9]*/, const double* intrinsics /*[4] fx fy cx cy*/, double* xyz /*[M,3]*/, double* proj /*[M,2]*/,
                     unsigned char* mask /*[M]*/);

/* ---- free-landmark Schur-complement BA: ADD-ON, PARITY UNPINNED ------------------------------------------
 * The reference keeps its landmarks fixed (BA_filtering.py:32-37) and has nothing to marginalise; this mode is the
 * variant BASELINE.json's north_star describes on top of it and has NO counterpart in the reference.  Unknowns: 6 per
 * pose (position, rotation; velocities untouched unless vba_schur_enable_dynamics adds them) and 3 per landmark, the landmarks held by a catalogue prior
 * N(X0, sigma_prior^2 I); weights = confidences (the reference's alpha = 2 case) until vba_schur_reweight is called.  One call of vba_schur_iterate builds the
 * normal equations at the resident state, marginalises the landmarks (3x3 inversions), factorises the dense reduced
 * camera system on the matrix cores (blocked Cholesky), back-substitutes, and keeps the step if the cost
 * sum w |r|^2 + |X - X0|^2 / sigma^2 went down.  Validated against oracle/schur_oracle.py (this repository's own CPU
 * restatement) only.  It shares nothing with a vba_handle and never runs inside vba_iterate.
 *
 * Structure arrays (built by the host once per window, vinsat_amd/schur.py): rows sorted by landmark with CSR lm_ptr[L+1];
 * row_pose / row_lm [m]; the rows of every pose as CSR pose_ptr[n+1] -> pose_rows[m]; and, for every 6x6 block (i >= j) of
 * the reduced system that two poses sharing a landmark touch (every diagonal block included), the list of row pairs
 * (pair_k of pose i, pair_k2 of pose j, same landmark) as CSR blk_ptr[nblk+1], with blk_i / blk_j [nblk]. */
typedef struct vba_schur_context* vba_schur_handle;
const char* vba_schur_last_error(void);
int vba_schur_create(int device, int n, int64_t m, int L, int nblk, int64_t npairs, vba_schur_handle* out);
int vba_schur_destroy(vba_schur_handle h);
int vba_schur_upload(vba_schur_handle h, const int* lm_ptr, const int* row_pose, const int* row_lm, const double* row_u,
                     const double* row_v, const double* row_w, const int* pose_ptr, const int* pose_rows, const int* blk_i,
                     const int* blk_j, const int* blk_ptr, const int* pair_k, const int* pair_k2, const double* intrinsics /*[n,4]*/,
                     const double* X0 /*[L,3] catalogue positions*/, double sigma_prior);
int vba_schur_set_state(vba_schur_handle h, const double* states /*[n,10]*/, const double* landmarks /*[L,3]*/);
int vba_schur_get_state(vba_schur_handle h, double* states, double* landmarks);
/* one LM trial at damping lamda (added to every diagonal entry of B and C); *accepted = the cost went down and the state moved.
 * A reduced camera system that is not positive definite at this damping is a REJECTED trial (*accepted = 0, *cost_after =
 * *cost_before, state untouched; vba_schur_last_info tells the failing row): the caller raises lamda as after any rejection. */
int vba_schur_iterate(vba_schur_handle h, double lamda, double* cost_before, double* cost_after, int* accepted);
/* 0 if the last factorisation went through, else 1 + the row of the reduced system at which it met a non-positive pivot
 * (the first such row: the factorisation goes on with that pivot replaced by 1, what it meets later is not recorded) */
int vba_schur_last_info(vba_schur_handle h, int* info);
/* HIP-event times of the last iterate: build (blocks + Schur complement), factor (Cholesky), solve (substitutions + update) */
int vba_schur_last_ms(vba_schur_handle h, float* build_ms, float* factor_ms, float* solve_ms);
/* what = 0: the step of the last iterate [6 n + 3 L]; 1: its Cholesky factor, dense lower triangular [6n, 6n] ([9n, 9n] on a handle
 * with the dynamics factor); 2: the 2 m keys |r| of the last vba_schur_reweight, sorted row order, row by row, u before v (VBA_ESTATE
 * if none since the upload).  On a handle with the dynamics factor (VBA_ESTATE without it) 3: the velocity step dv [n, 3] of the
 * last iterate; 4: the residuals r [n - 1, 6] and 5: the Jacobians D Phi [n - 1, 6, 6] of the edges at the state the last iterate
 * started from; 6: the edges' shares sigma_dyn |r|^2 [n - 1] of the cost there.  On a handle with the attitude factor (VBA_ESTATE
 * without it), all at the state the last iterate started from, 7: the residuals a [n - 1, 3]; 8: the Jacobian pairs [n - 1, 2, 3, 3]
 * (d a_i / d theta_i, then d a_i / d theta_{i+1}, row major); 9: the edges' shares sigma_att |a|^2 [n - 1] of the cost.  On a handle
 * with the state prior (VBA_ESTATE without it), all at the state the last iterate started from, 10: the residuals e [count, 9];
 * 11: the Jacobians J [count, 3, 3]; 12: the priors' shares e^T Lambda e [count] of the cost. */
int vba_schur_debug_fetch(vba_schur_handle h, int what, double* out, int64_t capacity);
/* The orbit-dynamics factor with the velocities as unknowns, opt-in per handle, after vba_schur_upload.  time_idx [n]: the second
 * of every pose; every gap time_idx[i + 1] - time_idx[i] in 1 .. 64 (the domain of the sequential propagation; longer gaps are
 * vba_schur_enable_dynamics_long's, below).  For every edge i -> i + 1 the reference's residual (BA_utils.py:467-476, 501-509)
 *   r_i = D (propagate(p_i, v_i; gap one-second RK4 steps of the J2 model) - (p_{i+1}, v_{i+1})),  D = diag(1, 1, 1, 100, 100, 100),
 * Jacobians D Phi_i at pose i and -D at pose i + 1, weight sigma_dyn, Gauss-Newton (sigma J^T J, -sigma J^T r); the cost gains
 * sigma_dyn sum |r_i|^2.  No wmax_scale: the rows keep the weights the handle holds.  The ATTITUDE factor of the fixed-landmark
 * path is not part of this mode: its Newton blocks are not symmetric and the reduced system here is factorised by a Cholesky.
 * Unknowns become dc [n, 6], dv [n, 3] and dl [L, 3]; the reduced system is ordered [6 n pose | 3 n velocity] unknowns, N = 9 n
 * (S, g and the factor's arrays are re-sized), lamda goes on the velocity diagonal too, vba_schur_get_state returns the updated
 * velocities, and the build time of vba_schur_last_ms includes the factor's kernels.  vba_schur_reweight, vba_schur_get_weights
 * and vba_schur_median work unchanged; vba_schur_covariance, vba_schur_reliability and vba_schur_snoop return VBA_ESTATE on such a
 * handle (their redundancy counts and gathers assume the 6 n system); vba_schur_covariance_dyn, vba_schur_reliability_dyn and
 * vba_schur_snoop_dyn are its queries.  A handle that never calls this behaves as before.  (vba_schur_enable_attitude, below, adds
 * a Gauss-Newton statement of the attitude term -- symmetric, so the Cholesky stands -- on a handle that has called this.)
 * Errors: VBA_EINVAL for n < 2, a gap outside 1 .. 64, a time_idx that does not increase, a sigma_dyn that is not positive and
 * finite; VBA_ESTATE before the upload or on a handle that has the factor already. */
int vba_schur_enable_dynamics(vba_schur_handle h, const int* time_idx /*[n]*/, double sigma_dyn);
/* vba_schur_enable_dynamics for the window of a later pass of a sequence: the same factor, contract, errors and downstream entries
 * (vba_schur_enable_attitude and every _dyn / _att query serve such a handle as a dynamics handle), except that gaps of
 * 65 .. VBA_MAX_GAP steps are accepted (VBA_EINVAL beyond, naming the poses).  An edge of more than 64 steps is propagated parallel
 * in time (the parareal chain and the ordered product of sub-chunk transition matrices of the fixed-landmark path), within rounding
 * of the serial walk up to ~1000 s and within the defect of the stop rule (~1e-13 relative) beyond; edges of 64 steps or fewer keep
 * the kernels and the bits of vba_schur_enable_dynamics, and on a window without a long gap every output has the bits of that entry.
 * The chain of an accepted trial is carried into the next call.  No cap on the number of long edges.  With VBA_SCHUR_LONG_SERIAL=1
 * in the environment when this is called, the long edges take the serial lanes too (a comparison: ~10^5 dependent instructions per
 * edge at 935 s). */
int vba_schur_enable_dynamics_long(vba_schur_handle h, const int* time_idx /*[n]*/, double sigma_dyn);
/* The poses i whose edge i -> i + 1 is propagated parallel in time on this handle, in index order: *count of them (none on a handle
 * of vba_schur_enable_dynamics or under VBA_SCHUR_LONG_SERIAL=1); idx (may be null) receives them, VBA_EINVAL if cap < *count.
 * VBA_ESTATE on a handle without the dynamics factor. */
int vba_schur_long_edges(vba_schur_handle h, int* idx, int cap, int* count);
/* Milliseconds (HIP events) of the cost kernels of the last trial of vba_schur_iterate: the rows, the prior and, on a handle with
 * them, the dynamics and attitude edges at the trial state; 0 before the first trial.  Beside vba_schur_last_ms, whose three
 * intervals end before the trial's cost. */
int vba_schur_last_trial_cost_ms(vba_schur_handle h, float* ms);
/* The Gauss-Newton attitude factor, opt-in per handle, after vba_schur_enable_dynamics.  cumrot [n][4]: the rotation accumulated over
 * the gap after pose i (scalar last, as vba_host_gap_rotations gives it); row n - 1 is ignored.  Rows are used as given, not
 * renormalised.  For every edge i -> i + 1, with (x) the Hamilton product:
 *   [e, d] = conj(q_i (x) cumrot_i) (x) q_{i+1},   s = d >= 0 ? +1 : -1,   a_i = s e   (|a_i|^2 = 1 - d^2; d is the reference's d),
 *   d a_i / d theta_{i+1} = 1/2 s (d I + [e]x),   d a_i / d theta_i = -1/2 s (L(conj cumrot_i) R(conj(q_i) (x) q_{i+1}))[0:3, 0:3]
 * along the mode's retraction q <- normalise(q (x) qexp(dtheta)); weight sigma_att, Gauss-Newton: sigma_att J^T J into the attitude
 * 3x3 blocks (rows and columns 6 i + 3 .. 6 i + 5) of the pose part, -sigma_att J^T a into the right-hand side; the cost gains
 * sigma_att sum |a_i|^2.  These blocks are symmetric positive semidefinite (the Newton blocks of the fixed-landmark path are not),
 * so the factorisation, the substitutions and the updates are unchanged.  The reference's term is sigma 100 (1 - |d|) =
 * sigma 100 |a|^2 / (1 + |d|): sigma_att = sigma_dyn * 100 / 2 weights the attitude as the reference does near the solution.  With
 * the factor the attitude of a pose without rows is held by its two edges and not by the damping alone.
 * vba_schur_covariance_dyn includes the factor; vba_schur_reliability_dyn, vba_schur_snoop_dyn and vba_schur_outlier_power_dyn return
 * VBA_ESTATE on such a handle (their redundancy counts and edge leverages do not know the 3 (n - 1) attitude equations):
 * vba_schur_reliability_att, vba_schur_snoop_att and vba_schur_outlier_power_att are its queries, and count them;
 * vba_schur_reweight, vba_schur_get_weights and vba_schur_median see rows only and work unchanged.  A handle that never calls this
 * launches what it launched before and returns the same bits.
 * Errors: VBA_EINVAL for a null pointer, a sigma_att that is not positive and finite, a cumrot row 0 .. n - 2 that is not finite or
 * whose norm is further than 1e-6 from 1; VBA_ESTATE before the upload, on a handle without the dynamics factor, or on a handle that
 * has the attitude factor already. */
int vba_schur_enable_attitude(vba_schur_handle h, const double* cumrot /*[n][4]*/, double sigma_att);
/* A Gaussian prior on the 9-DoF state of chosen poses, opt-in per handle, on a handle with the dynamics factor (either enable entry;
 * the attitude factor may be on or off, enabled before or after).  Coordinates are those of state_cov (vba_schur_covariance_dyn):
 * x = [dp (km), dtheta, dv (km/s)], unknown u(i, c) as documented there.  For prior k on pose i = pose_idx[k], anchor [k] =
 * (pbar [3], qbar [4] scalar last, vbar [3]) and info[k] = Lambda (9x9, symmetric, row major), with (x) the Hamilton product:
 *   [eps, d] = conj(qbar) (x) q_i,   s = d >= 0 ? +1 : -1,   e = [p_i - pbar, 2 s eps, v_i - vbar],
 *   F = blockdiag(I, J, I),   J = d (2 s eps) / d theta_i = s (d I + [eps]x)
 * along the mode's retraction q <- normalise(q (x) qexp(dtheta)), so J = I at q_i = +-qbar.  Gauss-Newton: F^T Lambda F into the
 * entries (u(i, a), u(i, b)) of the reduced system (the lower triangles of the 6x6 pose block and of the 3x3 velocity block, the whole
 * 3x6 velocity-pose block), -F^T Lambda e into the right-hand side; the cost gains sum e^T Lambda e, at the resident and at the
 * trial state.  Factorisation, substitutions and updates are unchanged.  A singular Lambda (position only, say) is accepted; an
 * indefinite one shows as a non-positive pivot (vba_schur_last_info) like any other.  vba_schur_covariance_dyn includes the factor;
 * vba_schur_reliability_dyn / _att, vba_schur_snoop_dyn / _att and vba_schur_outlier_power_dyn / _att return VBA_ESTATE on such a
 * handle (their redundancy counts do not know the prior's equations); vba_schur_reweight, vba_schur_get_weights and vba_schur_median
 * work unchanged.  A handle that never calls this launches what it launched before and returns the same bits.
 * Errors: VBA_ESTATE before the upload, without the dynamics factor, or with the prior enabled already; VBA_EINVAL (the message
 * names the entry) for a null pointer, count outside 1 .. n, an index outside 0 .. n - 1 or given twice, an anchor that is not finite
 * or whose quaternion norm is further than 1e-6 from 1, an info block that is not finite, not symmetric to 1e-12 of its largest
 * entry, or has a negative diagonal entry.  The handle stays usable after a refusal. */
int vba_schur_enable_state_prior(vba_schur_handle h, int count, const int* pose_idx /*[count]*/, const double* anchor /*[count][10]*/,
                                 const double* info /*[count][9][9]*/);
/* The hand-off of a solved window into the prior of the next one, on a handle with the dynamics factor, at its resident state: the
 * marginal Sigma = state_cov[n - 1] of vba_schur_covariance_dyn(h, lamda, ...) (its device part; nothing of the handle changes),
 * propagated over `steps` one-second RK4 steps of the J2 model on the device:
 *   (phat, vhat), Phi = the propagation of (p, v) of pose n - 1 with its transition matrix (the lanes of the dynamics factor up to 64
 *                       steps, its parallel-in-time bodies beyond),
 *   G      = Phi on the [dp, dv] components, R on dtheta: the matrix of dtheta' = conj(c) dtheta c, c = cumrot_gap (the rotation
 *            accumulated over the gap, scalar last), since q (x) qexp(d) (x) c = (q (x) c) (x) qexp(conj(c) d c),
 *   Sigma' = G Sigma G^T + steps diag(process_noise[0] x3, process_noise[1] x3, process_noise[2] x3)   (variances per second; NULL = 0),
 *   info_out = Sigma'^-1 by a 9x9 Cholesky, one triangle computed and mirrored;  anchor_out = [phat, normalise(q (x) c), vhat]:
 * what vba_schur_enable_state_prior takes for pose 0 of the next window.  *info: 0; 1 + the row of a non-positive pivot of the
 * query's factorisation; -1 if Sigma' is not positive definite; when it is not 0 the outputs are NaN and the call returns VBA_OK.
 * VBA_EINVAL: a null pointer (process_noise may be NULL), lamda negative or NaN, steps outside 1 .. VBA_MAX_GAP, a cumrot_gap that is
 * not a unit quaternion (finite, norm within 1e-6 of 1), negative or non-finite noise; VBA_ESTATE: before the upload or before a
 * state is set, or a handle without the dynamics factor. */
int vba_schur_handoff(vba_schur_handle h, double lamda, int steps, const double* cumrot_gap /*[4]*/, const double* process_noise /*[3] or NULL*/,
                      double* anchor_out /*[10]*/, double* info_out /*[9][9]*/, int* info);
/* HIP-event time of the last vba_schur_handoff on this handle (the device part of vba_schur_covariance_dyn and the hand-off kernel) */
int vba_schur_last_handoff_ms(vba_schur_handle h, float* ms);
/* Covariances of the free-landmark system at the resident state: blocks of the inverse of H = [[B, E], [E^T, C]] as
 * vba_schur_iterate(h, lamda, ...) would build it there (lamda on every diagonal entry of B and C; lamda = 0, the usual
 * case, gives the undamped covariance -- the catalogue prior fixes the gauge).  With S = B - E C^-1 E^T and Y_k = E_k C_l^-1:
 *   pose_cov[i] = (S^-1)_ii: the marginal of pose i over all landmarks and all other poses, coordinates [dp (km), dtheta]
 *                 (dtheta as in vba_covariance: the attitude sigma is 2 sqrt(.)); one triangle computed and mirrored;
 *   pair_cov[b] = (S^-1)_{blk_i[b], blk_j[b]} for every block of the uploaded block list (i >= j, diagonal blocks included,
 *                 bitwise the blocks of pose_cov): the cross-covariances of poses that share a landmark;
 *   lm_cov[l]   = C_l^-1 + sum over the rows k, k' of l of Y_k^T (S^-1)_{pose(k), pose(k')} Y_k', exactly symmetric.  For a
 *                 landmark without rows: d I with d = 1.0 / (1.0 / (sigma_prior * sigma_prior) + lamda), each of the three
 *                 operations rounded to double in that order, and exact zeros off the diagonal.
 * Any output may be NULL.  The weights are the confidences as uploaded, so -- as for vba_covariance -- this is a covariance up
 * to the variance factor of the weights.  *info is as vba_schur_last_info reports it for an iterate at this damping: 0, or 1 +
 * the first row with a non-positive pivot; then every requested output is filled with NaN and the call still returns VBA_OK.
 * VBA_EINVAL: null handle, null info, lamda negative or NaN (or uploaded pair lists that do not enumerate the row pairs of
 * every landmark); VBA_ESTATE: before upload or before a state is set; VBA_ENOMEM: no room for the scratch.
 * The query changes nothing: it builds and factorises into scratch of its own (allocated by the first query of a handle; a
 * handle that never asks allocates none).  State, last_info, last_ms and debug_fetch read as before, and the following
 * iterates return the bits they would have returned without it.  Fixed order of operations: equal bits for equal problems. */
int vba_schur_covariance(vba_schur_handle h, double lamda, double* pose_cov /*[n][6][6] or NULL*/, double* pair_cov /*[nblk][6][6] or NULL*/,
                         double* lm_cov /*[L][3][3] or NULL*/, int* info);
/* HIP-event time of the last vba_schur_covariance on this handle (build, factorisation, selected inverse and gathers) */
int vba_schur_last_covariance_ms(vba_schur_handle h, float* ms);
/* State covariances on a handle with the dynamics factor (vba_schur_enable_dynamics), at the resident state: blocks of the inverse
 * of H = [[B9, E9], [E9^T, C]] as vba_schur_iterate(h, lamda, ...) builds it on such a handle (the dynamics blocks and lamda on
 * the velocity diagonal included).  S9 = B9 - E9 C^-1 E9^T is ordered [6 n pose | 3 n velocity]; with x_i = [dp (km), dtheta,
 * dv (km/s)] of pose i -- the coordinates of vba_covariance -- component c of x_i is unknown u(i, c) = 6 i + c for c < 6 and
 * 6 n + 3 i + (c - 6) for c >= 6.
 *   state_cov[i] = the 9x9 marginal of x_i: the entries of S9^-1 at u(i, .); the lower triangle is read and mirrored, so every
 *                  block is exactly symmetric, and state_cov[i][:6][:6] has the bits of the diagonal block i of pair_cov;
 *   edge_cov[i]  = Sigma(x_i, x_{i+1}), rows of pose i and columns of pose i + 1 (the super-diagonal convention of vba_covariance):
 *                  what propagating or differencing consecutive states needs;
 *   pair_cov[b], lm_cov[l]: as vba_schur_covariance defines them, the 6x6 blocks out of the pose part (top-left 6 n x 6 n) of
 *                  S9^-1 (E9 has no velocity rows: the landmark formula is unchanged).
 * state_cov and edge_cov are required, pair_cov and lm_cov may be NULL.  *info as for vba_schur_covariance: 0, or 1 + the first
 * row with a non-positive pivot; then every output is filled with NaN and the call returns VBA_OK.  VBA_EINVAL: null handle,
 * info, state_cov or edge_cov, lamda negative or NaN; VBA_ESTATE: before upload or before a state is set, or a handle without
 * the dynamics factor (vba_schur_covariance is the query of those; it, vba_schur_reliability and vba_schur_snoop keep refusing
 * a handle that has the factor).  The query changes nothing: it builds and factorises into scratch of its own, the residuals,
 * Jacobians and edge costs of its build included, so vba_schur_debug_fetch 3 .. 6 (and 7 .. 9 on a handle with the attitude factor, which the build includes) still report the last iterate; the following
 * iterates return the bits they would have returned without it.  Fixed order of operations: equal bits for equal problems.  Only
 * the tiles of S9^-1 that an output reads are formed; VBA_SCHUR_COV_FULL=1 in the environment at vba_schur_create forms all of
 * them by the kernel of vba_schur_covariance (comparison: the outputs have the same bits either way). */
int vba_schur_covariance_dyn(vba_schur_handle h, double lamda, double* state_cov /*[n][9][9]*/, double* edge_cov /*[n-1][9][9]*/,
                             double* pair_cov /*[nblk][6][6] or NULL*/, double* lm_cov /*[L][3][3] or NULL*/, int* info);
/* HIP-event time of the last vba_schur_covariance_dyn on this handle (build, factorisation, selected inverse and gathers) */
int vba_schur_last_covariance_dyn_ms(vba_schur_handle h, float* ms);
/* Reliability of the free-landmark fit at the resident state: which observation row, and which catalogue position, the window
 * contradicts.  H, S, Y_k and the covariance blocks are those of vba_schur_covariance(h, lamda, ...); Sigma = H^-1.  For row k
 * (landmark-sorted order as uploaded; pose i, landmark l) with A_k = d uv / d [dp, dtheta] (2x6), Al_k = d uv / d X = -A_k[:, :3],
 * r_k = uv - est and weight w_k:
 *   Sigma_il    = -sum over the rows k' of l, upwards, of (S^-1)_{i, pose(k')} Y_k'   (6x3 pose-landmark cross-covariance)
 *   P_k         = w_k [A_k Al_k] [[Sigma_ii, Sigma_il], [Sigma_il^T, Sigma_ll]] [A_k Al_k]^T   (symmetric part)
 *   leverage[k] = tr P_k,   wtest[k] = sqrt(w_k r_k^T (I - P_k)^-1 r_k)   (2x2 inverse in closed form).
 *   w_k == 0: leverage 0 and wtest 0; det(I - P_k) <= 0 or a negative quadratic form: wtest NaN (as vba_reliability).
 * The catalogue prior N(X0, sigma^2 I) of landmark l as an observation, e_l = X_l - X0_l, P_l = Sigma_ll / sigma^2:
 *   lm_leverage[l] = tr P_l in (0, 3],   lm_wtest[l] = sqrt(e_l^T (I - P_l)^-1 e_l / sigma^2)   (3x3 inverse in closed form; NaN
 *   for a non-positive determinant or a negative form).  At lamda = 0 a landmark seen from ONE pose has an exactly singular
 *   I - P_l (its depth is held by the prior alone): its lm_wtest is NaN or a number without meaning -- lm_stats[l][2] tells the
 *   track length.  A landmark without rows is tested by nothing: lm_wtest 0 and
 *   lm_leverage = (3.0 * d) * (1.0 / (sigma_prior * sigma_prior)) with the d of vba_schur_covariance, rounded in that order.
 *   lm_stats[l] = {sum of leverage over the rows of l in row order, largest finite wtest among them (0 if none), number of them
 *   with w > 0};  pose_stats[i] = the same three over the rows of pose i in the order of pose_rows.
 *   fit[8] = {Omega = sum w |r|^2 + sum |e_l|^2 / sigma^2 (the cost of vba_schur_iterate, in a summation order of its own),
 *             m_eff = rows with w > 0, t_rows = sum leverage, t_prior = sum lm_leverage, rho = 2 m_eff + 3 L - t_rows - t_prior,
 *             s0sq = Omega / rho (NaN if rho <= 0), largest finite row wtest, largest finite landmark wtest}.
 * Any output may be NULL, in any combination; what is asked for decides the copies only, so the bits do not depend on it.  *info
 * and the error codes are those of vba_schur_covariance: with *info != 0 every requested output is NaN and the call returns VBA_OK.
 * The query changes nothing: state, last_info, last_ms, debug_fetch and last_covariance_ms read as before, and the following
 * iterates and covariance queries return the bits they would have returned without it.  Synchronous.  It uses the covariance
 * query's scratch and a little of its own, allocated by the first reliability query of a handle.  Every sum has one order (no
 * float atomics): equal problems give equal bits, across calls and across handles. */
int vba_schur_reliability(vba_schur_handle h, double lamda, double* leverage /*[m] or NULL*/, double* wtest /*[m] or NULL*/,
                          double* lm_leverage /*[L] or NULL*/, double* lm_wtest /*[L] or NULL*/, double* lm_stats /*[L][3] or NULL*/,
                          double* pose_stats /*[n][3] or NULL*/, double* fit /*[8] or NULL*/, int* info);
/* HIP-event time of the last vba_schur_reliability on this handle (the covariance query's device part and the three passes) */
int vba_schur_last_reliability_ms(vba_schur_handle h, float* ms);
/* Data snooping of the free-landmark fit: one call runs the device part of vba_schur_reliability(h, lamda, ...) at the resident
 * state, picks what to reject by the fixed rule below and zeroes the weights of the rejected rows in place, on the device.
 * Rejecting a ROW: its weight in the handle's weight array becomes 0.0; the value it had is kept.  Rejecting a CATALOGUE ENTRY:
 * the landmark leaves the window -- every row of it with w > 0 gets weight 0 (values kept likewise) and its byte in the landmark
 * mask is set; its prior then holds it at X0 and it no longer pulls any pose.  At most one rejection per group and call.
 *   c = crit, or crit * sqrt(s0sq) with scaled != 0, s0sq = fit[5] read on the device (the correctly rounded root, one product);
 *   returned in *crit_used.  A non-finite c rejects nothing; so does a call with *info != 0 (then *crit_used is NaN if scaled).
 *   cntl_l / cnt_i = rows of landmark l / pose i with w > 0.  Row candidate: w_k > 0, wtest[k] finite and > c.  Prior candidate:
 *   cntl_l >= min_track, lm_wtest[l] finite and > c.
 *   1. Per landmark: among its row candidates and its prior candidate the largest test wins; among rows ties go to the smaller
 *      sorted row; a row beats the prior on a tie; a NaN never wins.  The prior wins: the landmark is MARKED.  A row wins: the
 *      landmark PROPOSES that row.
 *   2. Per pose, in pose_rows order: c_lm_i = its weighted rows on marked landmarks; the pose is SHORT if cnt_i - c_lm_i <
 *      min_rows; its best proposed row (largest wtest, ties to the smaller sorted row) is rejected iff the pose is not short and
 *      cnt_i - c_lm_i - 1 >= min_rows.
 *   3. Per landmark: a marked landmark is rejected iff none of the poses of its weighted rows is short; otherwise nothing happens
 *      to it in this call (no cascade).
 * counts[3] = {rows rejected by their own test, landmarks rejected, rows zeroed through rejected landmarks} of this call;
 * counts and crit_used may be NULL.  *info as vba_schur_reliability.  From the call's return the handle gives, bit for bit, what a
 * fresh handle gives that was uploaded with the same structure, those rows' weights zeroed, and the same state set
 * (vba_schur_iterate, vba_schur_covariance, vba_schur_reliability).  A call that rejects nothing changes nothing: state,
 * last_info, last_ms, debug_fetch, last_covariance_ms and last_reliability_ms read as before.  The feature's state (a double and
 * a byte per row, a byte per landmark, a few ints per pose and landmark) is allocated by the first snoop of a handle and lives
 * until vba_schur_upload, which clears it.  Synchronous; no atomics: equal problems give equal masks.
 * Errors: as vba_schur_reliability; VBA_EINVAL also for a NaN or negative crit and for a negative min_rows or min_track. */
int vba_schur_snoop(vba_schur_handle h, double lamda, double crit, int scaled, int min_rows, int min_track, int* counts /*[3] or NULL*/,
                    double* crit_used /*or NULL*/, int* info);
/* Cumulative since the last upload or restore: row_mask [m] in the sorted row order of the upload, lm_mask [L], totals[3] as the
 * counts of vba_schur_snoop.  Any output may be NULL.  All zero on a handle that never snooped. */
int vba_schur_rejected(vba_schur_handle h, unsigned char* row_mask /*[m] or NULL*/, unsigned char* lm_mask /*[L] or NULL*/, int* totals /*[3] or NULL*/);
/* The saved weights back in place, both masks and the totals cleared: the handle gives the bits of one that never snooped.  A
 * no-op on a handle that never snooped. */
int vba_schur_snoop_restore(vba_schur_handle h);
/* HIP-event time of the last vba_schur_snoop on this handle (the reliability query's device part and the passes of the rule) */
int vba_schur_last_snoop_ms(vba_schur_handle h, float* ms);
/* Reliability on a handle with the dynamics factor (vba_schur_enable_dynamics), at the resident state: which observation row and
 * which catalogue position the window contradicts when the factor ties every pose to its neighbours, and how much redundancy the
 * fit has.  H = [[B9, E9], [E9^T, C]] is as vba_schur_covariance_dyn(h, lamda, ...) builds it, Sigma = H^-1.
 *   leverage, wtest, lm_leverage, lm_wtest, lm_stats, pose_stats: word for word as vba_schur_reliability defines them (the NaN
 *   rules, the w == 0 rule and the closed form of a landmark without rows included), with Sigma_ii, Sigma_il and Sigma_ll blocks
 *   of THIS Sigma.  Rows do not depend on the velocity and E9 has no velocity rows, so these are the 6x6 blocks out of the pose
 *   part (top-left 6 n x 6 n) of S9^-1 and the landmark marginals of vba_schur_covariance_dyn.
 *   Edge i (pose i -> pose i + 1) is a 6-row observation of weight sigma_dyn with J_i = [A_i | -D] (6x12) over
 *   x = [dp_i, dv_i, dp_{i+1}, dv_{i+1}], A_i = D Phi_i of the query's own build at the resident state; Sigma12 = the components
 *   {0, 1, 2, 6, 7, 8} of state_cov[i], edge_cov[i] and state_cov[i + 1] of vba_schur_covariance_dyn:
 *     edge_leverage[i] = tr(sigma_dyn J_i Sigma12 J_i^T) in (0, 6]  (each diagonal entry of J Sigma12 J^T on its own, summed in
 *                        index order),   edge_omega[i] = sigma_dyn |r_i|^2.
 *   There is NO w-test of an edge, on purpose.  At the weights of this project (sigma_dyn = 1e4) an edge's leverage lies between
 *   5.89 and 5.999 of 6, the smallest eigenvalue of I - P_e between -4e-10 and 1e-11: sqrt(sigma_dyn r^T (I - P_e)^-1 r) divides
 *   by rounding.  Two NumPy routes to it (dense inverse, Schur route) disagree by 2e-3 to 0.7 relative and give NaN on one or
 *   two edges; the edges carry next to no redundancy (0.18 of 66 on 12 poses / 150 landmarks).  The leverage itself is well
 *   conditioned (the routes agree to 1.5e-10) and the redundancy of the fit needs it, so it is returned.  Edges are never rejected.
 *   fit[10] = {Omega = rows, priors and edges: the cost of vba_schur_iterate on this handle, in a summation order of its own;
 *              m_eff; t_rows; t_prior; rho = 2 m_eff + 3 L + 6 (n - 1) - t_rows - t_prior - t_edges; s0sq = Omega / rho (NaN if
 *              rho <= 0); largest finite row wtest; largest finite landmark wtest; t_edges = sum edge_leverage;
 *              Omega_edges = sum edge_omega}: slots 0 .. 7 are those of vba_schur_reliability.  The traces obey
 *              t_rows + t_prior + t_edges + lamda tr(H^-1) = 9 n + 3 L.
 * Any output may be NULL, in any combination; what is asked for decides the copies only.  *info, the NaN-everywhere rule and the
 * error codes are those of vba_schur_covariance_dyn; a handle without the factor gets VBA_ESTATE (vba_schur_reliability is its
 * query, which keeps refusing a handle that has the factor).  The query changes nothing: state, last_info, last_ms, debug_fetch
 * 3 .. 6 and last_covariance_dyn_ms read as before, and the following iterates and vba_schur_covariance_dyn queries return the bits
 * they would have returned without it.  No float atomics, every sum has one order: equal problems give equal bits. */
int vba_schur_reliability_dyn(vba_schur_handle h, double lamda, double* leverage /*[m] or NULL*/, double* wtest /*[m] or NULL*/,
                              double* lm_leverage /*[L] or NULL*/, double* lm_wtest /*[L] or NULL*/, double* lm_stats /*[L][3] or NULL*/,
                              double* pose_stats /*[n][3] or NULL*/, double* edge_leverage /*[n-1] or NULL*/,
                              double* edge_omega /*[n-1] or NULL*/, double* fit /*[10] or NULL*/, int* info);
/* HIP-event time of the last vba_schur_reliability_dyn on this handle (the device part of vba_schur_covariance_dyn and the passes) */
int vba_schur_last_reliability_dyn_ms(vba_schur_handle h, float* ms);
/* Data snooping on a handle with the dynamics factor: the rule of vba_schur_snoop, steps 1 to 3 as they stand, with the same
 * counts, crit_used, min_rows and min_track, fed by the device part of vba_schur_reliability_dyn(h, lamda, ...); with scaled it
 * uses that query's fit[5].  Edges are never rejected.  vba_schur_rejected and vba_schur_snoop_restore serve both snoops.  From the
 * call's return the handle gives, bit for bit, what a fresh handle gives that has the same structure, the same time_idx and
 * sigma_dyn, those rows' weights zeroed and the same state (vba_schur_iterate, vba_schur_covariance_dyn,
 * vba_schur_reliability_dyn).  A call that rejects nothing changes nothing.  Errors: as vba_schur_snoop, and VBA_ESTATE on a
 * handle without the factor. */
int vba_schur_snoop_dyn(vba_schur_handle h, double lamda, double crit, int scaled, int min_rows, int min_track, int* counts /*[3] or NULL*/,
                        double* crit_used /*or NULL*/, int* info);
/* HIP-event time of the last vba_schur_snoop_dyn on this handle */
int vba_schur_last_snoop_dyn_ms(vba_schur_handle h, float* ms);
/* Outlier power of the free-landmark fit: how large an error in a row, or in a catalogue entry, passes the w-test unnoticed, and how
 * far such an error moves the orbit, the attitude and the landmark.  H, Sigma = H^-1, A_k, Al_k, r_k, w_k, Sigma_ii, Sigma_il,
 * Sigma_ll and P_k are those of vba_schur_reliability(h, lamda, ...); rows in the sorted order of the upload.  ncp > 0 and finite
 * is the non-centrality of the test at the chosen power (17.075 for alpha = 0.001, power 0.8 with two degrees of freedom), crit > 0
 * the critical value the counts use (+inf counts nothing).
 *
 * Row k of pose i and landmark l: J_k = [A_k Al_k] (2x9), Sigma_k = [[Sigma_ii, Sigma_il], [Sigma_il^T, Sigma_ll]], R_k = I - P_k
 * (symmetric part), B_k = w_k Sigma_k J_k^T (9x2; rows 0..2 B_p, 3..5 B_t, 6..8 B_l).  mu_min(R) is the smaller eigenvalue,
 * mu_max(M, R) the larger root of det(M - mu R) = 0.
 *   mdb     [m]  sqrt(ncp / (w_k mu_min(R_k)))                    px: the smallest bias in its worst direction the test detects
 *   ext_pos [m]  sqrt(ncp / w_k  mu_max(B_p^T B_p, R_k))          km: the largest move of the pose's position by an undetected bias
 *   ext_att [m]  2 sqrt(ncp / w_k  mu_max(B_t^T B_t, R_k))        rad, the 2 |dtheta| convention of vba_covariance
 *   ext_lm  [m]  sqrt(ncp / w_k  mu_max(B_l^T B_l, R_k))          km: the same for the row's own landmark
 *   del_pos [m]  |B_p R_k^-1 r_k|                                 km: the move of the pose's position if the row is deleted
 *   del_lm  [m]  |B_l R_k^-1 r_k|                                 km: the move of the row's landmark if the row is deleted
 * Catalogue prior of landmark l as an observation: P_l = Sigma_ll / sigma^2, p_max its largest eigenvalue, q = 1 - p_max,
 * e_l = X_l - X0_l.
 *   lm_mdb     [L]  sigma sqrt(ncp / q)                           km: the smallest catalogue error the test detects
 *   lm_ext     [L]  sigma sqrt(ncp) p_max / sqrt(q)               km: the move of the landmark's own estimate by a catalogue error at
 *                   that limit.  P_l and I - P_l commute, so mu_max(P_l^T P_l, I - P_l) = p_max^2 / q: the roots are p^2 / (1 - p)
 *                   over the eigenvalues p of P_l, and p^2 / (1 - p) rises on [0, 1).
 *   lm_del_pos [L]  the largest finite |Sigma_il[0:3,:] (I - P_l)^-1 e_l| / sigma^2 over the rows of l with w > 0 (km): the move of
 *                   the worst-hit pose if the prior is taken away.
 * Summaries: pose_fit[i] = {Omega_i = sum w |r|^2 over the rows of pose i in pose_rows order, the sum of their leverages (the bits of
 * pose_stats[i][0] of vba_schur_reliability), the largest finite ext_pos of its rows, the count of its rows with wtest > crit};
 * fit[12] = the fit[8] of vba_schur_reliability with its bits, then {rows with wtest > crit, largest finite ext_pos, landmarks with
 * lm_wtest > crit, largest finite lm_del_pos}.
 *
 * Degenerate input is flagged in the value.  w_k == 0: mdb = +inf, the other five 0.  det R_k <= 0 or mu_min(R_k) <= 0: NaN in all
 * six.  q <= 0 or not finite: lm_mdb and lm_ext NaN.  det(I - P_l) <= 0: lm_del_pos NaN.  A landmark without rows is tested by
 * nothing: lm_mdb = +inf, lm_ext = 0, lm_del_pos = 0.  *info != 0 (as vba_schur_reliability): every requested output is NaN and the
 * call returns VBA_OK.
 *
 * Any output may be NULL, in any combination: what is asked for decides the copies only.  The promises are those of
 * vba_schur_reliability: the query changes nothing, later iterates and queries return the bits they would have returned without it,
 * no float atomics, every sum in one order, equal problems give equal bits.  Synchronous.  Scratch is allocated by the first query of
 * a handle.  Errors: VBA_EINVAL for a NaN or negative lamda, an ncp that is not positive and finite, a crit that is not positive, a
 * null handle or info; VBA_ESTATE as vba_schur_reliability, a handle with the dynamics factor included (vba_schur_outlier_power_dyn
 * is its query).
 *
 * Not provided: an external reliability in VELOCITY on a handle with the dynamics factor needs the velocity-pose tiles of S9^-1 for
 * every pair of poses that share a landmark, which the selected inverse of vba_schur_covariance_dyn does not form; and there is no
 * power figure for dynamics edges, for the reason vba_schur_reliability_dyn gives for the edge w-test. */
int vba_schur_outlier_power(vba_schur_handle h, double lamda, double ncp, double crit, double* mdb /*[m] or NULL*/,
                            double* ext_pos /*[m] or NULL*/, double* ext_att /*[m] or NULL*/, double* ext_lm /*[m] or NULL*/,
                            double* del_pos /*[m] or NULL*/, double* del_lm /*[m] or NULL*/, double* lm_mdb /*[L] or NULL*/,
                            double* lm_ext /*[L] or NULL*/, double* lm_del_pos /*[L] or NULL*/, double* pose_fit /*[n][4] or NULL*/,
                            double* fit /*[12] or NULL*/, int* info);
/* HIP-event time of the last vba_schur_outlier_power on this handle (the device part of the reliability query and the passes) */
int vba_schur_last_outlier_power_ms(vba_schur_handle h, float* ms);
/* vba_schur_outlier_power on a handle with the dynamics factor: every quantity above with the blocks of the Sigma of
 * vba_schur_reliability_dyn(h, lamda, ...) -- the same row and prior formulas, the same degenerate rules and promises.  fit[14] =
 * the fit[10] of vba_schur_reliability_dyn with its bits, edges included, then the four slots above; pose_fit[i][1] has the bits of
 * that query's pose_stats[i][0].  VBA_ESTATE on a handle without the factor (vba_schur_outlier_power is its query). */
int vba_schur_outlier_power_dyn(vba_schur_handle h, double lamda, double ncp, double crit, double* mdb /*[m] or NULL*/,
                                double* ext_pos /*[m] or NULL*/, double* ext_att /*[m] or NULL*/, double* ext_lm /*[m] or NULL*/,
                                double* del_pos /*[m] or NULL*/, double* del_lm /*[m] or NULL*/, double* lm_mdb /*[L] or NULL*/,
                                double* lm_ext /*[L] or NULL*/, double* lm_del_pos /*[L] or NULL*/, double* pose_fit /*[n][4] or NULL*/,
                                double* fit /*[14] or NULL*/, int* info);
/* HIP-event time of the last vba_schur_outlier_power_dyn on this handle */
int vba_schur_last_outlier_power_dyn_ms(vba_schur_handle h, float* ms);
/* Reliability on a handle with the dynamics factor AND the attitude factor (vba_schur_enable_attitude), at the resident state: the
 * query of vba_schur_reliability_dyn with the 3 (n - 1) attitude equations counted, and a test of every attitude edge -- which gyro
 * gap rotation the window contradicts.  H = [[B9, E9], [E9^T, C]] is as vba_schur_covariance_dyn(h, lamda, ...) builds it on this
 * handle, both factors included, Sigma = H^-1.
 *   leverage, wtest, lm_leverage, lm_wtest, lm_stats, pose_stats: word for word as vba_schur_reliability defines them (the NaN
 *   rules, the w == 0 rule and the closed form of a landmark without rows included), with the Sigma_ii, Sigma_il and Sigma_ll blocks
 *   of THIS Sigma, as vba_schur_reliability_dyn takes them from its own.
 *   edge_leverage, edge_omega: the orbit edges, as vba_schur_reliability_dyn defines them, from the state_cov / edge_cov of THIS
 *   Sigma.  Still no w-test of an orbit edge, for the reason given there.
 *   Attitude edge i (pose i -> pose i + 1) is a 3-row observation of weight sigma_att with J_i = [J_own | J_next] (3x6) over
 *   x = [dtheta_i, dtheta_{i+1}] and the residual a_i (vba_schur_enable_attitude), both of the query's own build at the resident
 *   state; Sigma6 = the components {3, 4, 5} of state_cov[i], edge_cov[i] (rows of pose i, columns of pose i + 1; the lower left of
 *   Sigma6 is the transpose of the same stored block) and state_cov[i + 1] of vba_schur_covariance_dyn; P_a = sigma_att J_i Sigma6 J_i^T:
 *     att_leverage[i] = tr P_a in (0, 3]  (each diagonal entry on its own, summed in index order),
 *     att_omega[i]    = sigma_att |a_i|^2,
 *     att_wtest[i]    = sqrt(sigma_att a_i^T (I - P_a)^-1 a_i)  with the symmetric part of I - P_a, by cofactors over the determinant
 *                       as lm_wtest; NaN where the determinant is not positive or the quadratic form is negative or not finite.
 *   This test exists where the orbit edge's does not: an attitude edge keeps nearly all of its three units of redundancy (leverage
 *   4e-4 .. 9e-3 of 3 at sigma_att = 5e5 on windows whose poses all have rows; 1.5 on each of the two edges around a pose without
 *   rows, which alone determine that pose's attitude), the smallest eigenvalue of I - P_a is at least 0.49, and two NumPy routes
 *   to the test agree to 3e-14.  An edge next to a bad gap rotation absorbs part of it: the bad gap ranks first, its neighbours
 *   follow.  Edges of either kind are never rejected.
 *   fit[13] = {Omega = rows, priors, orbit edges and attitude edges: the cost of vba_schur_iterate on this handle, in a summation
 *              order of its own; m_eff; t_rows; t_prior;
 *              rho = 2 m_eff + 3 L + 6 (n - 1) + 3 (n - 1) - t_rows - t_prior - t_edges - t_att; s0sq = Omega / rho (NaN if rho <= 0);
 *              largest finite row wtest; largest finite landmark wtest; t_edges; Omega_edges; t_att = sum att_leverage;
 *              Omega_att = sum att_omega; largest finite att_wtest}: slots 0 .. 9 are those of vba_schur_reliability_dyn.  The traces
 *              obey t_rows + t_prior + t_edges + t_att + lamda tr(H^-1) = 9 n + 3 L; at lamda = 0 with every weight positive
 *              rho = 2 m - 9.
 * Any output may be NULL, in any combination; what is asked for decides the copies only.  *info, the NaN-everywhere rule and the
 * error codes are those of vba_schur_reliability_dyn; a handle without the attitude factor gets VBA_ESTATE (vba_schur_reliability_dyn
 * or vba_schur_reliability is its query; both keep refusing a handle that has the factor).  The query changes nothing: state,
 * last_info, last_ms, debug_fetch 3 .. 9 and last_covariance_dyn_ms read as before, and the following iterates and
 * vba_schur_covariance_dyn queries return the bits they would have returned without it.  No float atomics, every sum has one order:
 * equal problems give equal bits. */
int vba_schur_reliability_att(vba_schur_handle h, double lamda, double* leverage /*[m] or NULL*/, double* wtest /*[m] or NULL*/,
                              double* lm_leverage /*[L] or NULL*/, double* lm_wtest /*[L] or NULL*/, double* lm_stats /*[L][3] or NULL*/,
                              double* pose_stats /*[n][3] or NULL*/, double* edge_leverage /*[n-1] or NULL*/,
                              double* edge_omega /*[n-1] or NULL*/, double* att_leverage /*[n-1] or NULL*/, double* att_wtest /*[n-1] or NULL*/,
                              double* att_omega /*[n-1] or NULL*/, double* fit /*[13] or NULL*/, int* info);
/* HIP-event time of the last vba_schur_reliability_att on this handle (the device part of vba_schur_covariance_dyn and the passes) */
int vba_schur_last_reliability_att_ms(vba_schur_handle h, float* ms);
/* Data snooping on a handle with both factors: the rule of vba_schur_snoop, steps 1 to 3 as they stand, with the same counts,
 * crit_used, min_rows and min_track, fed by the device part of vba_schur_reliability_att(h, lamda, ...); with scaled it uses that
 * query's fit[5], which counts the attitude equations.  Edges of either kind are never rejected: a gyro suspect (att_wtest) is
 * reported by the reliability query, not acted on.  vba_schur_rejected and vba_schur_snoop_restore serve this snoop too.  From the
 * call's return the handle gives, bit for bit, what a fresh handle gives that has the same structure, the same factors, those rows'
 * weights zeroed and the same state (vba_schur_iterate, vba_schur_covariance_dyn, vba_schur_reliability_att).  A call that rejects
 * nothing changes nothing.  Errors: as vba_schur_snoop_dyn, and VBA_ESTATE on a handle without the attitude factor. */
int vba_schur_snoop_att(vba_schur_handle h, double lamda, double crit, int scaled, int min_rows, int min_track, int* counts /*[3] or NULL*/,
                        double* crit_used /*or NULL*/, int* info);
/* HIP-event time of the last vba_schur_snoop_att on this handle */
int vba_schur_last_snoop_att_ms(vba_schur_handle h, float* ms);
/* vba_schur_outlier_power on a handle with both factors: every quantity of vba_schur_outlier_power with the blocks of the Sigma of
 * vba_schur_reliability_att(h, lamda, ...) -- the same row and prior formulas, the same degenerate rules and promises.  fit[17] =
 * the fit[13] of vba_schur_reliability_att with its bits, edges of both kinds included, then the four slots of
 * vba_schur_outlier_power; pose_fit[i][1] has the bits of that query's pose_stats[i][0].  There is no power figure for an edge of
 * either kind: the detectable bias of a gap rotation is not provided.  VBA_ESTATE on a handle without the attitude factor. */
int vba_schur_outlier_power_att(vba_schur_handle h, double lamda, double ncp, double crit, double* mdb /*[m] or NULL*/,
                                double* ext_pos /*[m] or NULL*/, double* ext_att /*[m] or NULL*/, double* ext_lm /*[m] or NULL*/,
                                double* del_pos /*[m] or NULL*/, double* del_lm /*[m] or NULL*/, double* lm_mdb /*[L] or NULL*/,
                                double* lm_ext /*[L] or NULL*/, double* lm_del_pos /*[L] or NULL*/, double* pose_fit /*[n][4] or NULL*/,
                                double* fit /*[17] or NULL*/, int* info);
/* HIP-event time of the last vba_schur_outlier_power_att on this handle */
int vba_schur_last_outlier_power_att_ms(vba_schur_handle h, float* ms);
/* Robust re-weighting of the free-landmark fit: the reference's weights (BA_filtering.py:21-25) at the resident state, written
 * into the handle's weight array in place, on the device.  The reference computes them once per BA() call and holds them through
 * its LM trials; here the caller decides when (vinsat_amd/schur.py: solve(robust=...)).
 *   r_k = uv_k - est_k at the resident state, the projection of the cost kernel of vba_schur_iterate (Z_MIN clamp included).
 *   Keys: |r|, two per row, of ALL rows whatever their weight: a row of weight 0 (rejected, or uploaded so) counts in the median,
 *   as a row of confidence 0 does in the reference (BA_filtering.py:23).
 *   c = *c_obs = the exact lower median, the key of rank (2 m - 1) / 2 (torch.median), by a radix select on the bit patterns: the
 *   bits of the sorted keys' entry of that rank.
 *   q_k = mean over the two components of ((r / c)^2 / |alpha - 2| + 1)^(alpha / 2 - 1) / c^2;  *w_max = q_max = the largest q_k over
 *   all rows, taken before the base weights enter (BA_filtering.py:25);  rho_k = q_k / q_max.
 *   alpha in [1, 2]; anything else, or NaN: VBA_EINVAL.  alpha == 2 is the reference's inf ** 0 == 1: rho_k is exactly 1, no power is
 *   evaluated (q_max = 1 / c^2); c_obs is still computed and returned.
 *   base_k = the weight of row k as vba_schur_upload received it.  A row that is not rejected: row_w[k] = rho_k * base_k, one
 *   product.  A row vba_schur_snoop has rejected keeps 0.0 and its saved weight becomes rho_k * base_k: vba_schur_snoop_restore
 *   then yields the handle that never snooped and was re-weighted at this state.
 * *status = 0: re-weighted.  *status = 1: c_obs is 0 or not finite (a NaN residual among the middle keys, a state that fits
 * exactly), or q_max is not positive and finite (a NaN residual anywhere: numpy's max); then weights and saved values are
 * untouched, *c_obs holds what was found, *w_max is NaN and the call still returns VBA_OK.
 * From the call's return the handle gives, bit for bit, what a fresh handle gives that was uploaded with the same structure, the
 * weights vba_schur_get_weights now returns, and the same state (vba_schur_iterate, vba_schur_covariance, vba_schur_reliability,
 * vba_schur_snoop).  vba_schur_reweight(h, 2.0, ...) puts base back bit for bit on the rows that are not rejected.  State,
 * last_info, last_ms, debug_fetch(0 / 1), last_covariance_ms, last_reliability_ms and last_snoop_ms read as before the call.
 * The feature's state (base weights, keys and raw weights: four doubles per row; the select's histograms) is allocated by the
 * first re-weighting of a handle and lives until vba_schur_upload, which clears it: those are new weights.  A handle that never
 * calls this allocates nothing.  Synchronous.  No float atomics (integer atomics count the select's histograms, which is exact in
 * any order; the maximum has one fixed shape): equal problems give equal bits, across calls and across handles.
 * Errors: VBA_EINVAL (null argument, alpha); VBA_ESTATE before upload or before a state is set; VBA_ENOMEM: no room for the state. */
int vba_schur_reweight(vba_schur_handle h, double alpha, double* c_obs, double* w_max, int* status);
/* The current weights and the base weights (as uploaded), both in sorted row order.  On a handle that never re-weighted base
 * equals w, except that rows the snoop rejected report their saved value.  Either output may be NULL. */
int vba_schur_get_weights(vba_schur_handle h, double* w /*[m] or NULL*/, double* base /*[m] or NULL*/);
/* HIP-event time of the last vba_schur_reweight on this handle (keys, select, raw weights, scaling) */
int vba_schur_last_reweight_ms(vba_schur_handle h, float* ms);
/* The select of vba_schur_reweight on caller keys: *median = the key of rank (count - 1) / 2 among count >= 1 non-negative
 * doubles (+0, denormals and +inf included), bit for bit the entry of that rank of the sorted keys.  It runs the same select
 * kernels (one workgroup up to 8192 keys, eight histogram passes beyond), on a process-wide workspace as vba_prepare_rows does,
 * and restores the caller's HIP device.  VBA_EINVAL: a NaN key, a key with the sign bit set (-0 included), count < 1 or > 2^31. */
int vba_schur_median(int device, const double* keys, int64_t count, double* median);

#ifdef __cplusplus
}
#endif
#endif /* VINSAT_BA_H */
