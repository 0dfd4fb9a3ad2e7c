// vba_upload.hip -- what goes up to a handle and comes back: observations, pose constants, priors, states.
#include "vba_context.h"

// The states that vba_set_states staged for the first kernel of a chained schedule, sent up with the two stream copies of the other
// handles instead: whoever else is about to read S[par] or the damping -- a single call, a query, the sharded calls, vba_get_states
// -- comes through settle() and finds them on the device.
int flush_states(vba_handle h) {
    if (!h->pend.on) return VBA_OK;
    h->pend.on = false;
    HIPCHK(hipSetDevice(h->device));
    const size_t n10 = (size_t)h->pend.n * 10;
    HIPCHK(hipMemcpyAsync(h->S[h->pend.par], h->h_stage_map, n10 * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(&h->V.sc[0].lam[h->pend.par], h->h_stage_map + n10, 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipEventRecord(h->ev_stage, h->stream));
    h->stage_copy = true;
    return VBA_OK;
}

// The next of the two pinned staging blocks (max(obs_stride, 9 n_max + 160) doubles each), once the copy that last went out of it
// has left it.  *ub: its index -- the caller records ev_up[*ub] behind the copies it enqueues out of the block.
static int next_staging(vba_handle h, int* ub) {
    *ub = h->up_next;
    h->up_next ^= 1;
    HIPCHK(hipEventSynchronize(h->ev_up[*ub]));
    return VBA_OK;
}

int vba_upload_observations(vba_handle h, int window, int n, int64_t m, const double* xyz, const double* uv,
                            const double* conf, const int64_t* ii) {
    if (int rc = check_window(h, window)) return rc;
    if (int rc_settle = settle(h, true)) return rc_settle;
    h->touch();
    if (!xyz || !uv || !conf || !ii) return fail(VBA_EINVAL, "null observation array");
    h->carry_ok = false;
    if (n < 2 || n > h->n_max) return fail(VBA_EINVAL, "n out of range (need 2 <= n <= n_max)");
    if (m < 1 || m > h->m_max) return fail(VBA_EINVAL, "m out of range (need 1 <= m <= m_max)");
    if (h->have_win[window] && h->n[window] != n) { h->have_win[window] = 0; h->have_state[window] = 0; h->have_prior[window] = 0; }   // a new window: re-upload its constants
    HIPCHK(hipSetDevice(h->device));
    // stable counting sort by pose: the reference's segment sums run in input order inside a pose
    std::vector<int> ptr(n + 1, 0);
    for (int64_t k = 0; k < m; ++k) {
        if (ii[k] < 0 || ii[k] >= n) return fail(VBA_EINVAL, "ii[" + std::to_string(k) + "] outside [0, n)");
        ptr[ii[k] + 1]++;
    }
    for (int i = 0; i < n; ++i) ptr[i + 1] += ptr[i];
    std::vector<int64_t>& perm = h->perm[window];
    perm.assign(m, 0);
    if (!h->perm_stale.empty()) h->perm_stale[window] = 1;
    if (!h->snoop_total.empty()) if (int rc = snoop_forget_window(h, window)) return rc;    // new rows: nothing of them is rejected
    {
        std::vector<int> cur(ptr.begin(), ptr.end() - 1);
        for (int64_t k = 0; k < m; ++k) perm[cur[ii[k]]++] = k;
    }
    // the whole block of the window -- six coordinate arrays, pose index, CSR -- is packed into pinned memory and goes up
    // with ONE asynchronous copy on the handle's stream; the pose / row counts follow in a one-thread kernel
    int ub;
    if (int rc = next_staging(h, &ub)) return rc;
    double* blk = h->h_up[ub];
    const size_t mp = (size_t)h->m_pad;
    double *x = blk, *y = x + mp, *z = y + mp, *u = z + mp, *v = u + mp, *c = v + mp;
    int* pose = reinterpret_cast<int*>(c + mp);
    int* cptr = pose + mp;
    for (int64_t s = 0; s < m; ++s) {
        const int64_t k = perm[s];
        x[s] = xyz[3 * k]; y[s] = xyz[3 * k + 1]; z[s] = xyz[3 * k + 2];
        u[s] = uv[2 * k]; v[s] = uv[2 * k + 1];
        c[s] = conf[k];
        pose[s] = (int)ii[k];
    }
    std::memcpy(cptr, ptr.data(), (size_t)(n + 1) * sizeof(int));
    const int mi = (int)m;
    const size_t used = (size_t)(reinterpret_cast<char*>(cptr + n + 1) - reinterpret_cast<char*>(blk));
    HIPCHK(hipMemcpyAsync(h->d_obs + (size_t)window * h->V.obs_stride, blk, used, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipEventRecord(h->ev_up[ub], h->stream));
    launch_set_counts(h->V, window, n, mi, h->stream);
    HIPCHK(hipGetLastError());
    h->n[window] = n;
    h->m[window] = mi;
    h->have_obs[window] = 1;
    h->V.n_min = *std::min_element(h->n.begin(), h->n.end());
    return VBA_OK;
}

int vba_upload_window(vba_handle h, int window, int n, const double* intrinsics, const double* cumrot_last,
                      const int64_t* time_idx) {
    if (int rc = check_window(h, window)) return rc;
    if (int rc_settle = settle(h, true)) return rc_settle;
    h->touch();
    if (!intrinsics || !cumrot_last || !time_idx) return fail(VBA_EINVAL, "null pose-constant array");
    h->carry_ok = false;
    if (n < 2 || n > h->n_max) return fail(VBA_EINVAL, "n out of range (need 2 <= n <= n_max)");
    if (h->have_obs[window] && h->n[window] != n) { h->have_obs[window] = 0; h->have_state[window] = 0; h->have_prior[window] = 0; }   // a new window: re-upload its rows
    HIPCHK(hipSetDevice(h->device));
    std::vector<int> steps(n);
    for (int i = 0; i + 1 < n; ++i) {
        const int64_t d = time_idx[i + 1] - time_idx[i];
        if (d < 1) return fail(VBA_EINVAL, "time_idx must be strictly increasing");
        if (d > VBA_MAX_GAP) return fail(VBA_EINVAL, "time_idx: a gap longer than VBA_MAX_GAP (2^20 s)");
        steps[i] = (int)d;
    }
    steps[n - 1] = 1;   // BA_utils.py:75
    // long gaps (vba_long.hip): the first kLongCap edges of more than kLongGap steps are marked by a NEGATIVE step count and
    // listed; the kernels that walk the chain leave them to k_long_factor / k_long_trial (with the hop integrator the sign is
    // ignored and nothing is long)
    // ... each with room for its chain (header + G sub-chunk start states) in the window's pool; a gap the pool has no room for
    // stays an ordinary edge
    int long_list[2 * kLongCap + 1];
    int nl = 0, pool_used = 0;
    for (int i = 0; i + 1 < n && nl < kLongCap; ++i)
        if (steps[i] > kLongGap) {
            const int need_states = long_pool_states(long_plan(steps[i]));
            if (pool_used + need_states > h->V.long_pool_cap) continue;
            long_list[kLongCap + 1 + nl] = pool_used;
            pool_used += need_states;
            long_list[nl++] = i;
            steps[i] = -steps[i];
        }
    long_list[kLongCap] = nl;
    const size_t pb = (size_t)window * h->n_max;
    int ub;
    if (int rc = next_staging(h, &ub)) return rc;
    double* blk = h->h_up[ub];
    std::memcpy(blk, intrinsics, (size_t)n * 32);
    std::memcpy(blk + (size_t)n * 4, cumrot_last, (size_t)n * 32);
    std::memcpy(blk + (size_t)n * 8, steps.data(), (size_t)n * 4);
    double* lblk = blk + (size_t)n * 8 + (size_t)(n + 1) / 2;      // (8 n + ceil(n / 2) + 65 doubles in all: inside the block's 9 n_max + 160)
    std::memcpy(lblk, long_list, sizeof(long_list));
    HIPCHK(hipMemcpyAsync(h->d_intr + pb * 4, blk, (size_t)n * 32, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_cumrot + pb * 4, blk + (size_t)n * 4, (size_t)n * 32, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_steps + pb, blk + (size_t)n * 8, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    if (nl) {
        HIPCHK(hipMemcpyAsync(h->d_long_idx + (size_t)window * kLongCap, lblk, (size_t)nl * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->d_long_off + (size_t)window * kLongCap, reinterpret_cast<const int*>(lblk) + kLongCap + 1, (size_t)nl * 4,
                              hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(hipMemcpyAsync(h->d_n_long + window, reinterpret_cast<const int*>(lblk) + kLongCap, 4, hipMemcpyHostToDevice, h->stream));
    // (the carried chains of the window's long edges belong to the steps that were just replaced: all ones = NaN start states, which
    // no state ever equals)
    if (nl || h->n_long[window])
        HIPCHK(hipMemsetAsync(h->V.long_pool + (size_t)window * 2 * h->V.long_pool_cap * 6, 0xFF,
                              (size_t)2 * h->V.long_pool_cap * 6 * sizeof(double), h->stream));
    HIPCHK(hipEventRecord(h->ev_up[ub], h->stream));
    h->n_long[window] = nl;
    h->V.nblk_long = h->V.hop ? 0 : *std::max_element(h->n_long.begin(), h->n_long.end());     // (the <= 100 s hops of predict_gpu: no gap is long)
    launch_set_counts(h->V, window, n, -1, h->stream);
    HIPCHK(hipGetLastError());
    h->n[window] = n;
    h->have_win[window] = 1;
    return VBA_OK;
}

int vba_upload_prior(vba_handle h, int window, int n, const double* states_prior, const double* hessian_state) {
    if (int rc = check_window(h, window)) return rc;
    if (int rc_settle = settle(h, true)) return rc_settle;
    h->touch();
    if (!states_prior || !hessian_state) return fail(VBA_EINVAL, "null prior array");
    if (!h->have_obs[window] && !h->have_win[window]) return fail(VBA_ESTATE, "upload the window before its prior");
    if (n != h->n[window]) return fail(VBA_EINVAL, "the prior needs one row per pose of the window");
    HIPCHK(hipSetDevice(h->device));
    std::vector<double> xp((size_t)n * 6);
    for (int i = 0; i < n; ++i) {
        const double* s = states_prior + (size_t)i * 10;
        double* o = xp.data() + (size_t)i * 6;
        o[0] = s[0]; o[1] = s[1]; o[2] = s[2]; o[3] = s[7]; o[4] = s[8]; o[5] = s[9];
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t pb = (size_t)window * h->n_max;
    HIPCHK(hipMemcpy(h->d_prior_x + pb * 6, xp.data(), xp.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_prior_H + pb * 36, hessian_state, (size_t)n * 36 * 8, hipMemcpyHostToDevice));
    h->have_prior[window] = 1;
    return VBA_OK;
}

int vba_set_states(vba_handle h, int window, const double* states, double lamda) {
    if (!h) return fail(VBA_EINVAL, "null handle");
    VBA_ESTAMP(1);
    if (int rc_settle = settle(h, true, true)) return rc_settle;        // (states staged earlier are replaced below, or go up first)
    if (!states) return fail(VBA_EINVAL, "null states");
    h->carry_ok = 0;
    double* S = h->S[h->par];           // the input buffer of the next call
    if (h->h_stage_map && window == 0 && (h->have_obs[0] || h->have_win[0])) {
        // one-window latency-mode handle: staged only; the first kernel of the next chained schedule takes them from there
        // (vba_context::h_stage_map).  States staged before and not sent up yet are simply replaced: nothing has been queued
        // that reads them.
        if (h->stage_kernel) { HIPCHK(hipSetDevice(h->device)); HIPCHK(hipStreamSynchronize(h->stream)); h->stage_kernel = false; }
        if (h->stage_copy) { HIPCHK(hipEventSynchronize(h->ev_stage)); h->stage_copy = false; }
        const int n = h->n[0];
        std::memcpy(h->h_stage_map, states, (size_t)n * 80);
        h->h_stage_map[(size_t)n * 10] = lamda;
        h->pend.on = true; h->pend.par = h->par; h->pend.n = n;
        h->have_state[0] = 1;
        VBA_ESTAMP(2);
        return VBA_OK;
    }
    if (int rc = flush_states(h)) return rc;    // (an error return below leaves the earlier states in place, as before)
    if (window == -1) {     // the same states for every window (all windows must have the same number of poses)
        const int n = h->n[0];
        for (int w = 0; w < h->W; ++w) {
            if (!h->have_obs[w] && !h->have_win[w]) return fail(VBA_ESTATE, "upload the windows before their states");
            if (h->n[w] != n) return fail(VBA_EINVAL, "window = -1 needs equal pose counts");
        }
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipEventSynchronize(h->ev_stage));
        std::memcpy(h->h_stage, states, (size_t)n * 80);
        HIPCHK(hipMemcpyAsync(S, h->h_stage, (size_t)n * 80, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipEventRecord(h->ev_stage, h->stream));
        DevView V = h->V;
        V.states = S;
        V.par = h->par;
        launch_broadcast_states(V, n, lamda, h->stream);
        HIPCHK(hipGetLastError());
        for (int w = 0; w < h->W; ++w) h->have_state[w] = 1;
        return VBA_OK;
    }
    if (int rc = check_window(h, window)) return rc;
    if (!h->have_obs[window] && !h->have_win[window]) return fail(VBA_ESTATE, "upload the window before its states");
    HIPCHK(hipSetDevice(h->device));
    const int n = h->n[window];
    // through a pinned staging buffer and asynchronously on the handle's stream: the call returns as soon as the
    // caller's array has been read, and the next call's kernels queue up behind the copy instead of behind two
    // blocking transfers
    HIPCHK(hipEventSynchronize(h->ev_stage));
    std::memcpy(h->h_stage, states, (size_t)n * 80);
    h->h_stage[(size_t)h->n_max * 10] = lamda;
    HIPCHK(hipMemcpyAsync(S + (size_t)window * h->n_max * 10, h->h_stage, (size_t)n * 80, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(&h->V.sc[window].lam[h->par], h->h_stage + (size_t)h->n_max * 10, 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipEventRecord(h->ev_stage, h->stream));
    h->have_state[window] = 1;
    VBA_ESTAMP(2);
    return VBA_OK;
}

// what a finished call left in the window's scalars, seen from the parity `par` of the NEXT call
void unpack_scalars(const WinScalars* sc, int par, double* lamda, double* last_hessian, int* n_trials, unsigned* flags) {
    if (lamda) *lamda = sc->lam[par];
    if (last_hessian) std::memcpy(last_hessian, sc->last_hessian, 81 * 8);
    if (n_trials) *n_trials = sc->n_trials;
    if (flags) *flags = sc->fl[par ^ 1] & 7u;       // the public bits (vinsat_ba.h)
}

int vba_get_states(vba_handle h, int window, double* states, double* lamda, double* last_hessian, int* n_trials,
                   unsigned* flags) {
    if (int rc = check_window(h, window)) return rc;
    if (int rc_settle = settle(h)) return rc_settle;
    if (!h->have_state[window]) return fail(VBA_ESTATE, "no states uploaded");
    HIPCHK(hipSetDevice(h->device));
    const int n = h->n[window];
    // both pieces through pinned memory behind the queued work, one wait for the lot
    WinScalars* sc = reinterpret_cast<WinScalars*>(h->h_back + (size_t)h->n_max * 10);
    if (states) HIPCHK(hipMemcpyAsync(h->h_back, h->S[h->par] + (size_t)window * h->n_max * 10, (size_t)n * 80, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(sc, h->V.sc + window, sizeof(WinScalars), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (states) std::memcpy(states, h->h_back, (size_t)n * 80);
    unpack_scalars(sc, h->par, lamda, last_hessian, n_trials, flags);
    return VBA_OK;
}

int vba_set_states_all(vba_handle h, const double* states, const double* lamda) {
    if (!h) return fail(VBA_EINVAL, "null handle");
    if (int rc_settle = settle(h, true)) return rc_settle;
    if (!states || !lamda) return fail(VBA_EINVAL, "null states / lamda");
    for (int w = 0; w < h->W; ++w)
        if (!h->have_obs[w] && !h->have_win[w]) return fail(VBA_ESTATE, "upload the windows before their states");
    HIPCHK(hipSetDevice(h->device));
    h->carry_ok = 0;
    const size_t per = (size_t)h->n_max * 10;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(h->S[h->par], states, (size_t)h->W * per * sizeof(double), hipMemcpyHostToDevice));
    std::vector<WinScalars> sc((size_t)h->W);
    HIPCHK(hipMemcpy(sc.data(), h->V.sc, sc.size() * sizeof(WinScalars), hipMemcpyDeviceToHost));
    for (int w = 0; w < h->W; ++w) sc[w].lam[h->par] = lamda[w];
    HIPCHK(hipMemcpy(h->V.sc, sc.data(), sc.size() * sizeof(WinScalars), hipMemcpyHostToDevice));
    for (int w = 0; w < h->W; ++w) h->have_state[w] = 1;
    return VBA_OK;
}

int vba_get_states_all(vba_handle h, double* states, double* lamda, double* last_hessian, int* n_trials, unsigned* flags) {
    if (!h) return fail(VBA_EINVAL, "null handle");
    if (int rc_settle = settle(h)) return rc_settle;
    for (int w = 0; w < h->W; ++w)
        if (!h->have_state[w]) return fail(VBA_ESTATE, "no states uploaded");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t per = (size_t)h->n_max * 10;
    if (states) HIPCHK(hipMemcpy(states, h->S[h->par], (size_t)h->W * per * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<WinScalars> sc((size_t)h->W);
    HIPCHK(hipMemcpy(sc.data(), h->V.sc, sc.size() * sizeof(WinScalars), hipMemcpyDeviceToHost));
    for (int w = 0; w < h->W; ++w)
        unpack_scalars(&sc[w], h->par, lamda ? lamda + w : nullptr, last_hessian ? last_hessian + (size_t)w * 81 : nullptr,
                       n_trials ? n_trials + w : nullptr, flags ? flags + w : nullptr);
    return VBA_OK;
}
