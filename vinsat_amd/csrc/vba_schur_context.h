// vba_schur_context.h -- the host side of the free-landmark mode shared by its translation units (the map of the units and of
// their kernels heads vba_schur.hip): the view the kernels take, the row geometry three units reproject with, the context behind a
// vba_schur_handle with the state of every feature, error reporting, the scratch helper behind the features, the scaffold of the
// query entries (which kind of handle an entry serves, what runs before its device part, how its outputs reach the host), and the
// functions one unit defines and another calls.  Internal.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/vinsat_ba.h"
#include "vba_math.h"
#include "vba_schur_dyn.h"

using namespace vba;

// (everything below is internal to the library: hidden, as vba_context.h is)
#pragma GCC visibility push(hidden)

typedef double vf4 __attribute__((ext_vector_type(4)));

constexpr int kT = 64;              // tile of the blocked Cholesky
constexpr int kPanel = 4;           // tile columns per panel: the trailing update runs with K = kPanel * kT = 256 (round 4)

struct SchurView {
    int n, L;
    int64_t m;
    int N, Npad, nb;                // reduced system: N = 6 n (9 n with the dynamics factor), padded to a multiple of kT, nb tiles per side
    // rows sorted by landmark: CSR lm_ptr[L+1]
    const int* lm_ptr;
    const int* row_pose;            // [m]
    const int* row_lm;              // [m]
    const double *row_u, *row_v, *row_w;    // [m] measurement, weight
    // rows of a pose: CSR pose_ptr[n+1] -> pose_rows[m] (indices into the landmark-sorted rows)
    const int* pose_ptr;
    const int* pose_rows;
    // blocks (i >= j) of S that receive pair products: CSR blk_ptr[nblk+1] -> (pair_k, pair_k2); blk_i, blk_j
    int nblk;
    const int *blk_i, *blk_j, *blk_ptr, *pair_k, *pair_k2;
    const double* intr;             // [n][4]
    const double* X0;               // [L][3] catalogue positions
    double inv_sigma2;              // 1 / sigma_prior^2
    double lamda;
    // state
    const double* states;           // [n][10]
    const double* X;                // [L][3]
    double* states_new;
    double* X_new;
    // work
    double* Cinv;                   // [L][6] symmetric inverse (00,01,02,11,12,22)
    double* wl;                     // [L][3]
    double* E;                      // [m][18] row major 6x3
    double* Y;                      // [m][18]
    double* S;                      // [Npad][Npad] row major, lower triangle used
    double* g;                      // [Npad] right-hand side, then the step of the poses
    double* ybuf;                   // [Npad] intermediate of the two substitutions
    double* invL;                   // [nb][kT*kT] inverse of the diagonal Cholesky factors
    double* dl;                     // [L][3]
    double* part;                   // cost partials
    int npart;
};

// The reduced system of N unknowns in whole panels of tiles (the padding rows are an identity block): nb tiles per side, Npad rows
inline void schur_padded_size(int N, int& nb, int& Npad) {
    nb = (N + kT * kPanel - 1) / (kT * kPanel) * kPanel;
    Npad = nb * kT;
}

// row k of the landmark-sorted rows: residual, A (d uv / d p_c), camera point, for pose / landmark state given
struct RowGeom {
    double ru, rv, a00, a02, a11, a12, cam[3];
    PoseCam pc;
};

__device__ __forceinline__ void row_geometry(const SchurView& V, const double* states, const double* X, int k, RowGeom& q) {
    const int i = V.row_pose[k], l = V.row_lm[k];
    pose_camera(states + (size_t)i * 10, V.intr + (size_t)i * 4, q.pc);
    double u, v, d;
    project(q.pc, X[3 * l], X[3 * l + 1], X[3 * l + 2], u, v, q.cam, d);
    q.ru = V.row_u[k] - u;
    q.rv = V.row_v[k] - v;
    const double live = q.cam[2] > kZMin ? 1.0 : 0.0;
    q.a00 = q.pc.fx * d;
    q.a11 = q.pc.fy * d;
    q.a02 = -(q.a00 * (q.cam[0] * d * live));
    q.a12 = -(q.a11 * (q.cam[1] * d * live));
}

// J_l = A R^T (2x3): row u -> jl[0..2], row v -> jl[3..5]
__device__ __forceinline__ void landmark_jacobian(const RowGeom& q, double* jl) {
    const double* R = q.pc.R;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        jl[c] = q.a00 * R[3 * c] + q.a02 * R[3 * c + 2];
        jl[3 + c] = q.a11 * R[3 * c + 1] + q.a12 * R[3 * c + 2];
    }
}

// J_c = [-J_l | 2 A hat(p_c)] (2x6): row u -> jc[0..5], row v -> jc[6..11]
__device__ __forceinline__ void pose_jacobian(const RowGeom& q, const double* jl, double* jc) {
    const double x = q.cam[0], y = q.cam[1], z = q.cam[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) { jc[c] = -jl[c]; jc[6 + c] = -jl[3 + c]; }
    jc[3] = 2.0 * (-q.a02 * y);
    jc[4] = 2.0 * (-q.a00 * z + q.a02 * x);
    jc[5] = 2.0 * (q.a00 * y);
    jc[9] = 2.0 * (q.a11 * z - q.a12 * y);
    jc[10] = 2.0 * (q.a12 * x);
    jc[11] = 2.0 * (-q.a11 * x);
}

// ---- error reporting (vba_schur.hip holds the thread-local text that vba_schur_last_error returns)
int sfail(int code, const std::string& msg);
#define SCHK(expr)                                                                                     \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return sfail(VBA_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// ---- scratch of a feature (vba_schur.hip)
// The arrays of one allocation, one after the other, each on a 256-byte boundary: need(b) is the offset of the next one.
struct SchurLayout {
    size_t bytes = 0;
    size_t need(size_t b) { const size_t o = bytes; bytes += (b + 255) & ~size_t(255); return o; }
};

// What every feature allocates on its first call: one zeroed arena, the two events around its timed section, the last reading.
struct SchurScratch {
    char* arena = nullptr;
    hipEvent_t ev[2] = {};
    float ms = 0.0f;
};
// arena (zeroed) and events, or nothing at all; `what` names the scratch in the message of a failure
int schur_scratch_alloc(SchurScratch& Z, size_t bytes, const char* what);
// events and arena go, Z is as it was before its allocation
void schur_scratch_release(SchurScratch& Z);
// End of the timed section on stream s: ev[1], then whatever `copies` enqueues behind it (the copies to the host stay outside the
// reported milliseconds), the wait for the stream, ms = ev[0] .. ev[1].
template <class Copies>
int schur_scratch_finish(SchurScratch& Z, hipStream_t s, Copies copies) {
    SCHK(hipEventRecord(Z.ev[1], s));
    if (int rc = copies()) return rc;
    SCHK(hipStreamSynchronize(s));
    (void)hipEventElapsedTime(&Z.ms, Z.ev[0], Z.ev[1]);
    return VBA_OK;
}
inline int schur_scratch_finish(SchurScratch& Z, hipStream_t s) { return schur_scratch_finish(Z, s, [] { return (int)VBA_OK; }); }

// ---- state of the features
// Scratch of vba_schur_covariance, allocated by the first query of a handle: every array the build and the factorisation write,
// W, the gathered blocks and the landmarks' pair -> block index (built on the host from the uploaded lists, once per upload).
struct SchurQuery {
    SchurScratch sc;
    double *Cinv = nullptr, *wl = nullptr, *E = nullptr, *Y = nullptr, *S = nullptr, *g = nullptr, *ybuf = nullptr, *invL = nullptr, *dl = nullptr;
    double *W = nullptr, *pair = nullptr, *pose = nullptr, *lm = nullptr;
    int *info = nullptr, *lp_ptr = nullptr, *lp_blk = nullptr;
    bool indexed = false;
    // on a handle with the dynamics factor (vba_schur_covariance_dyn): the 9x9 state and edge blocks, the tiles of the selected
    // product (I, J per tile; built with the index, once per upload), and the dynamics arrays of the query's own build -- the
    // handle's r, A, ecost stay those of its last iterate
    double *state = nullptr, *edge = nullptr, *dyn_r = nullptr, *dyn_A = nullptr, *dyn_ecost = nullptr, *dyn_part = nullptr;
    int* tiles = nullptr;
    int ntiles = 0;
};

// What vba_schur_reliability needs beyond that, allocated by the first reliability query of a handle: its outputs on the device,
// the per-row and per-landmark cost terms of the totals, and two timing events of its own.  fit has the thirteen slots of
// vba_schur_reliability_att (the plain query fills and copies eight, vba_schur_reliability_dyn ten); elev [n - 1], the edge
// leverages, exists on a handle with the dynamics factor only; alev, awt [n - 1], leverage and w-test of the attitude edges, on a
// handle with the attitude factor only.
struct SchurRel {
    SchurScratch sc;
    double *lev = nullptr, *wt = nullptr, *om = nullptr, *lmlev = nullptr, *lmwt = nullptr, *lmom = nullptr, *lm_stats = nullptr,
           *pose_stats = nullptr, *fit = nullptr, *elev = nullptr, *alev = nullptr, *awt = nullptr;
};

// What vba_schur_outlier_power needs beyond the reliability scratch, allocated by the first power query of a handle: its outputs on
// the device (six figures per row, three per landmark, pose_fit [n][4], fit with the seventeen slots of vba_schur_outlier_power_att),
// pull [m] = |Sigma_il[0:3,:] z_l| of every row for the landmarks' maxima, and two timing events of its own.
struct SchurPow {
    SchurScratch sc;
    double *mdb = nullptr, *epos = nullptr, *eatt = nullptr, *elm = nullptr, *dpos = nullptr, *dlm = nullptr, *pull = nullptr, *lm_mdb = nullptr,
           *lm_ext = nullptr, *lm_del = nullptr, *pose_fit = nullptr, *fit = nullptr;
};

// State of vba_schur_snoop, allocated by the first snoop of a handle and cleared by vba_schur_upload: the weight a rejected row
// had and a byte per row, a byte per landmark (both cumulative), the per-call decisions of the passes, two timing events.
struct SchurSnoop {
    SchurScratch sc;
    double *saved = nullptr, *crit_used = nullptr;
    unsigned char *row_mask = nullptr, *lm_mask = nullptr;
    int *lm_dec = nullptr, *pose_pick = nullptr, *pose_short = nullptr, *pose_out = nullptr, *lm_out = nullptr;
    int totals[3] = {0, 0, 0};  // rows rejected by their own test, landmarks rejected, rows zeroed through rejected landmarks
};

// State of vba_schur_reweight, allocated by the first re-weighting of a handle and cleared by vba_schur_upload: the weights as
// uploaded, the 2 m keys |r| and the raw weights of the last call, the select's histograms, two timing events.
struct SchurRobust {
    SchurScratch sc;
    double *base = nullptr, *keys = nullptr, *q = nullptr, *part = nullptr, *res = nullptr;
    unsigned long long *hist = nullptr, *state = nullptr;
    bool captured = false;      // base holds the weights of the current upload
    bool have_keys = false;     // keys are those of a re-weighting since the current upload
    int launches = 0;           // kernel launches of the last re-weighting
};

// State of vba_schur_enable_dynamics: the reduced system re-sized for N = 9 n (S, g, ybuf, invL: the view points here from then on),
// the edges' step counts, the factor of the last build and the partials of its cost.
struct SchurDyn {
    char* arena = nullptr;
    bool enabled = false;
    double sigma = 0.0;
    int* steps = nullptr;
    double *r = nullptr, *A = nullptr, *ecost = nullptr, *part = nullptr;
    int npart = 0;              // block partials; the long edges' partials lie behind them (h_part holds both)
    std::vector<double> h_part;
    // long edges of a handle of vba_schur_enable_dynamics_long (vba_schur_dyn_long.h): none on any other handle
    int nlong = 0, par = 0, long_pool_states = 0;
    int *long_idx = nullptr, *long_off = nullptr;
    double* long_pool = nullptr;
    std::vector<int> h_long_idx;
};

// State of vba_schur_enable_attitude: the gap rotations, the factor of the last build and the partials of its cost, and (q_*) the
// arrays vba_schur_covariance_dyn builds into, so that a, J, ecost stay those of the last iterate.  One allocation.
struct SchurAtt {
    char* arena = nullptr;
    bool enabled = false;
    double sigma = 0.0;
    double *cumrot = nullptr, *a = nullptr, *J = nullptr, *ecost = nullptr, *part = nullptr;
    double *q_a = nullptr, *q_J = nullptr, *q_ecost = nullptr, *q_part = nullptr;
    int npart = 0;
    std::vector<double> h_part;
};

// State of vba_schur_enable_state_prior: the priors as uploaded, the terms of the last build and the partials of the cost, and (q_*)
// the arrays vba_schur_covariance_dyn builds into, so that e, J and the shares stay those of the last iterate.  One allocation.
struct SchurPrior {
    char* arena = nullptr;
    bool enabled = false;
    int count = 0, npart = 0;
    int* idx = nullptr;
    double *anchor = nullptr, *info = nullptr;
    double *e = nullptr, *J = nullptr, *LF = nullptr, *Le = nullptr, *share = nullptr, *part = nullptr;
    double *q_e = nullptr, *q_J = nullptr, *q_LF = nullptr, *q_Le = nullptr, *q_share = nullptr;
    std::vector<double> h_part;
};

// Scratch of vba_schur_handoff, allocated by the first hand-off of a handle: the chain slot of a long gap (vba_long_body.h), the
// outputs on the device, two timing events.
struct SchurHandoff {
    SchurScratch sc;
    double *pool = nullptr, *out = nullptr;
};

// why vba_schur_reliability_dyn, vba_schur_snoop_dyn and vba_schur_outlier_power_dyn refuse a handle with the attitude factor
// (vba_schur_reliability_att, vba_schur_snoop_att and vba_schur_outlier_power_att are the queries of such a handle)
constexpr char kAttRefusal[] = " is not available on a handle with the attitude factor: its redundancy counts and edge leverages do not "
                               "know the 3 (n - 1) attitude equations";

// why the plain-named queries refuse a handle with the dynamics factor (vba_schur_covariance_dyn is the covariance query of such a handle)
constexpr char kDynRefusal[] = " is not available on a handle with the dynamics factor: its redundancy counts and gathers assume the "
                               "6 n reduced system of the reprojection rows";

// why the six _dyn / _att reliability, snoop and outlier power entries refuse a handle with the state prior (vba_schur_covariance_dyn
// serves it)
constexpr char kPriorRefusal[] = " is not available on a handle with the state prior: its redundancy counts do not know the 9 equations "
                                 "of every prior";

// which handle an entry serves: the plain one, one with the dynamics factor, one with the attitude factor too
enum SchurKind { kSchurPlain = 0, kSchurDyn = 1, kSchurAtt = 2 };

struct vba_schur_context {
    int device = 0;
    SchurView V{};
    char* arena = nullptr;
    hipStream_t stream = nullptr, aux = nullptr;    // aux: the bulk of a panel's trailing update beside the next panel's factorisation
    hipEvent_t ev[5] = {};
    hipEvent_t ev_chain = nullptr, ev_bulk = nullptr;
    int classic = 0;                // VBA_SCHUR_CLASSIC=1: the round-2 tile-by-tile factorisation (comparison)
    int cov_full = 0;               // VBA_SCHUR_COV_FULL=1: vba_schur_covariance_dyn runs the full W^T W product (comparison)
    int* d_info = nullptr;
    int last_info = 0;              // 0, or 1 + the row at which the last factorisation met a non-positive pivot
    double* S0 = nullptr;       // states buffers
    double* S1 = nullptr;
    double* X0buf = nullptr;
    double* X1buf = nullptr;
    std::vector<double> h_part;
    bool uploaded = false, have_state = false;
    float ms[4] = {0, 0, 0, 0};
    int64_t npairs = 0;
    SchurQuery q;               // vba_schur_covariance's scratch (nothing until the first query)
    SchurRel rel;               // vba_schur_reliability's scratch on top of it (nothing until the first reliability query)
    SchurPow pow;               // vba_schur_outlier_power's scratch on top of both (nothing until the first power query)
    SchurSnoop snoop;           // vba_schur_snoop's state (nothing until the first snoop)
    SchurRobust robust;         // vba_schur_reweight's state (nothing until the first re-weighting)
    SchurDyn dyn;               // vba_schur_enable_dynamics' state (nothing on a handle without the dynamics factor)
    SchurAtt att;               // vba_schur_enable_attitude's state (nothing on a handle without the attitude factor)
    SchurPrior prior;           // vba_schur_enable_state_prior's state (nothing on a handle without the state prior)
    SchurHandoff handoff;       // vba_schur_handoff's scratch (nothing until the first hand-off)
    int bw = 1 << 30;           // tile bandwidth of the reduced system (max |I - J| over its non-zero tiles), from the block list
};

// ---- vba_schur_build.hip
// S, g, Cinv, wl, E, Y of the view's state and damping on stream s (S and g zeroed by the caller): the reprojection blocks, the
// dynamics blocks on a handle with the factor (the attitude blocks behind them on a handle with that factor too), the identity of the
// padding rows.  dyn (if given) replaces the handle's own dynamics arrays: the covariance query of such a handle builds r, A, ecost in
// its scratch and leaves the handle's as the last iterate wrote them; att (if given) does the same for the attitude arrays, prior
// (if given) for those of the state prior, whose blocks go behind every other factor's
void schur_build_launch(vba_schur_handle h, const SchurView& V, hipStream_t s, const SchurDynView* dyn = nullptr, const SchurAttView* att = nullptr,
                        const SchurPriorView* prior = nullptr);

// ---- vba_schur_factor.hip
// S = Lg Lg^T in place and the inverse diagonal factors, on stream s (the bulk of a panel's trailing update beside it on h->aux);
// *d_info (zeroed by the caller) keeps 1 + the first row with a non-positive pivot
int schur_factor_launch(vba_schur_handle h, const SchurView& V, hipStream_t s, int* d_info);

// ---- vba_schur.hip
int schur_build_factor(vba_schur_handle h, const SchurView& V, hipStream_t s, int* d_info, hipEvent_t ev_built, const SchurDynView* dyn = nullptr,
                       const SchurAttView* att = nullptr, const SchurPriorView* prior = nullptr);

// -- the scaffold of the query entries (covariance, reliability, snoop, outlier power)
// VBA_OK, or why an entry of this kind does not serve this handle: the one place that decides it.  `entry` goes in front of the
// refusal: the entry's own name for a plain-named entry (kDynRefusal), the name of the dynamics-only counterpart for a _dyn or an
// _att entry (kAttRefusal); nullptr: a _dyn entry that serves a handle with the attitude factor too (vba_schur_covariance_dyn).
// A plain-named entry asks before it looks at its arguments, the others behind them (schur_query_begin asks for every entry).
int schur_kind_check(SchurKind kind, vba_schur_handle h, const char* entry);
// What every query entry does between its argument checks and the allocations of its own feature: problem and state are there,
// the kind of the handle is the entry's, the device is current, the query scratch and its index exist.
int schur_query_begin(vba_schur_handle h, SchurKind kind, const char* entry);
// One output of a query: where the caller wants it (nullptr: not asked for), where it lies on the device, how many doubles.
struct Out { double* host; const double* dev; size_t count; };
// End of a query whose timed section began at Z.ev[0] (schur_scratch_finish).  bad != 0 (no factor, no covariance, no figure): NaN
// into every output asked for.  Else the copies to the host behind ev[1]: what is asked for decides the copies only.
int schur_outputs_finish(SchurScratch& Z, hipStream_t s, int bad, const Out* outs, size_t count);
// the body of a vba_schur_last_*_ms getter: the last reading of the scratch of one feature (&vba_schur_context::q, ::rel, ...)
template <class Feature>
int schur_last_ms(vba_schur_handle h, Feature vba_schur_context::*feature, float* ms) {
    if (!h || !ms) return sfail(VBA_EINVAL, "null argument");
    *ms = (h->*feature).sc.ms;
    return VBA_OK;
}

// ---- vba_schur_cov.hip
int schur_query_alloc(vba_schur_handle h);
int schur_query_index(vba_schur_handle h);
// the device part of the covariance query of the handle, plain or with the dynamics factor (h->dyn.enabled decides)
int schur_query_device(vba_schur_handle h, double lamda, bool with_lm, hipEvent_t ev_begin, SchurView& V, int* bad);

// ---- vba_schur_rel.hip
int schur_rel_alloc(vba_schur_handle h);
// the device part of the reliability query of a handle of this kind (checked by the caller); pow_ncp > 0: the row pass of the
// outlier power query in the place of k_rel_rows
int schur_rel_device(vba_schur_handle h, SchurKind kind, double lamda, hipEvent_t ev_begin, SchurView& V, int* bad, double pow_ncp = 0.0);

// ---- vba_schur_power.hip
// k_pow_rows on the handle's stream in the place of k_rel_rows (the power scratch is allocated): lev, wt, om of the reliability
// scratch with the bits of k_rel_rows, and the six row figures and the prior pull of vba_schur_outlier_power at this ncp
void schur_pow_rows_launch(vba_schur_handle h, const SchurView& V, double ncp);

// ---- vba_schur_dyn.hip
// the dynamics arrays of a handle with the factor enabled, at the damping of the view
SchurDynView schur_dyn_view(vba_schur_handle h, const SchurView& V);
// the body of vba_schur_enable_dynamics and of vba_schur_enable_dynamics_long (long_gaps: gaps up to VBA_MAX_GAP are accepted)
int schur_dyn_enable(vba_schur_handle h, const int* time_idx, double sigma_dyn, bool long_gaps);

// ---- vba_schur_att.hip
// the attitude arrays of a handle with that factor enabled; query: the arrays of vba_schur_covariance_dyn's build in their place
SchurAttView schur_att_view(vba_schur_handle h, const SchurView& V, bool query = false);

// ---- vba_schur_prior.hip
// the arrays of the state prior of a handle with it enabled; query: the arrays of vba_schur_covariance_dyn's build in their place
SchurPriorView schur_prior_view(vba_schur_handle h, const SchurView& V, bool query = false);
#pragma GCC visibility pop
