// vba_obs.hip -- the first kernel of a BA call on fresh states, and the housekeeping kernels (gfx950).
//
//   k_obs_residual     A1: reprojection residuals at the input states, |r| keys, sum |r|, digit 0 of the exact select
//   k_debug_project    recompute est / Jacobian at the step's input states for vba_debug_fetch
//   k_broadcast_states, k_set_counts, k_reset_calls, k_clear_hist
//                      states, counts, call counters and histograms between calls
//
// The other stages of the call have units of their own:
//   vba_select.hip     A3a: k_select_pass, k_select_warm, k_select_finish (device bodies: vba_select_body.h)
//   vba_accumulate.hip A2 + A3: k_obs_accumulate
//   vba_trial.hip      A8: k_trial (compiled inside vba_accumulate.hip's unit)
//   vba_shard.hip      sharded mode, carried keys: k_sh_front, k_sh_clear_miss
#include <algorithm>
#include "vba_launch.h"
#include "vba_select_body.h"

namespace vba {


// ---------------------------------------------------------------------------------------------- A1
// HIST0: also histogram the top radix digit (the 10 exponent bits) of the keys this block produced.
template <bool HIST0>
__global__ __launch_bounds__(kObsBlock) void k_obs_residual(DevView V, double* abs_out /*null: V.absr*/) {
    __shared__ double red[kObsBlock / 64];
    __shared__ unsigned lh[HIST0 ? 1024 : 1];
    const int w = blockIdx.y;
    VBA_SKIP_CALL(V, w);
    const int m = V.m[w];
    const size_t ob = (size_t)w * V.obs_stride;     // observation block of the window
    const size_t mb = (size_t)w * V.m_max;          // per-observation work arrays
    const int k = blockIdx.x * kObsBlock + threadIdx.x;
    if (HIST0) {
        for (int b = threadIdx.x; b < 1024; b += kObsBlock) lh[b] = 0u;
        __syncthreads();
    }
    double s = 0.0;
    if (k < m) {
        const int pose = V.opose[2 * ob + k];
        const size_t pb = (size_t)w * V.n_max + pose;
        PoseCam pc;
        pose_camera(V.states + pb * 10, V.intr + pb * 4, pc);
        double u, v, cam[3], d;
        project(pc, V.ox[ob + k], V.oy[ob + k], V.oz[ob + k], u, v, cam, d);
        const double ru = fabs(V.ou[ob + k] - u), rv = fabs(V.ov[ob + k] - v);
        double* ab = abs_out ? abs_out : V.absr + 2 * mb;
        reinterpret_cast<double2*>(ab)[k] = make_double2(ru, rv);
        s = ru + rv;
        if (HIST0) {
            atomicAdd(&lh[(unsigned)(f64_bits(ru) >> 53) & 1023u], 1u);
            atomicAdd(&lh[(unsigned)(f64_bits(rv) >> 53) & 1023u], 1u);
        }
    }
    const double t = block_sum<kObsBlock>(s, red);
    if (threadIdx.x == 0) V.part_init[(size_t)w * V.nblk_obs + blockIdx.x] = t;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        begin_call_scalars(V.sc[w], V.par);
        V.sc[w].sel_cnt = 0u;
    }
    if (HIST0) {
        unsigned* hist = hist0_of(V, w, V.par);
        for (int b = threadIdx.x; b < 1024; b += kObsBlock) {
            const unsigned c = lh[b];
            if (c) atomicAdd(&hist[b], c);
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            V.sc[w].sel_prefix[0] = 0ull;
            V.sc[w].sel_rank[0] = (2 * (long long)m - 1) / 2;
        }
    }
}

void launch_obs_residual(const DevView& V, double* abs_out, hipStream_t s) {
    // the exponent histogram is fused only when the keys of this launch are the whole key set (not sharded)
    if (abs_out) hipLaunchKernelGGL(k_obs_residual<false>, dim3(V.nblk_obs, V.W), dim3(kObsBlock), 0, s, V, abs_out);
    else hipLaunchKernelGGL(k_obs_residual<true>, dim3(V.nblk_obs, V.W), dim3(kObsBlock), 0, s, V, abs_out);
}

// ---------------------------------------------------------------------------------------------- debug
__global__ __launch_bounds__(kObsBlock) void k_debug_project(DevView V, int w, double* est, double* J, double* wt) {
    const int m = V.m[w];
    const int k = blockIdx.x * kObsBlock + threadIdx.x;
    if (k >= m) return;
    const size_t ob = (size_t)w * V.obs_stride, mb = (size_t)w * V.m_max;
    const int pose = V.opose[2 * ob + k];
    const size_t pb = (size_t)w * V.n_max + pose;
    PoseCam pc;
    pose_camera(V.states_prev + pb * 10, V.intr + pb * 4, pc);
    double u, v, cam[3], d;
    project(pc, V.ox[ob + k], V.oy[ob + k], V.oz[ob + k], u, v, cam, d);
    est[2 * k] = u;
    est[2 * k + 1] = v;
    if (V.jac_f32) project_jacobian_f32(pc, cam, d, J + 12 * (size_t)k);      // the Jacobian the fp32 accumulation used
    else project_jacobian(pc, cam, d, J + 12 * (size_t)k);
    wt[k] = (V.wraw[mb + k] / bits_f64(V.sc[w].wmax_bits[V.par])) * V.oconf[ob + k];
}

void launch_debug_project(const DevView& V, int w, int m, double* est, double* J, double* wt, hipStream_t s) {
    hipLaunchKernelGGL(k_debug_project, dim3((m + kObsBlock - 1) / kObsBlock), dim3(kObsBlock), 0, s, V, w, est, J, wt);
}

// ---------------------------------------------------------------------------------------------- housekeeping
// window 0's states and damping copied to every other window (vba_set_states with window == -1)
__global__ __launch_bounds__(256) void k_broadcast_states(DevView V, int n, double lamda) {
    const int w = blockIdx.y;
    const double* src = V.states;
    double* dst = V.states + (size_t)w * V.n_max * 10;
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (w > 0 && k < n * 10) dst[k] = src[k];
    if (k == 0) V.sc[w].lam[V.par] = lamda;
}

void launch_broadcast_states(const DevView& V, int n, double lamda, hipStream_t s) {
    hipLaunchKernelGGL(k_broadcast_states, dim3((n * 10 + 255) / 256, V.W), dim3(256), 0, s, V, n, lamda);
}

// pose / row counts of a freshly uploaded window (m < 0: keep)
__global__ void k_set_counts(int* n_arr, int* m_arr, int w, int n, int m) {
    n_arr[w] = n;
    if (m >= 0) m_arr[w] = m;
}

void launch_set_counts(const DevView& V, int w, int n, int m, hipStream_t s) {
    hipLaunchKernelGGL(k_set_counts, dim3(1), dim3(1), 0, s, const_cast<int*>(V.n), const_cast<int*>(V.m), w, n, m);
}

// The kernel in front of a chain of calls: every window back at call 0.  In front of a chained schedule (vba_run_schedule) it also
// does what else the entry needs, so that the whole entry is one launch inside the schedule's graph:
//   stage != nullptr   the states and the damping that vba_set_states left in mapped host memory go into window 0's S[V.par] /
//                      sc.lam[V.par] (one-window handles; n10 = poses * 10 doubles, an even count: one double2 per thread, the
//                      caller's exact bits).  The kernels of the call read them behind the kernel boundary.
//   clear0             the digit-0 histogram of parity V.par is cleared (k_clear_hist, which == 0)
__global__ __launch_bounds__(256) void k_reset_calls(DevView V, const double* stage, int n10, int clear0) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int stride = gridDim.x * 256;
    for (int w = t; w < V.W; w += stride) {
        V.sc[w].call_idx = 0;
        V.sc[w].pending = -1;
        V.sc[w].miss = 0;       // (a speculated call that was dropped may have recorded a missed warm select: nobody will repeat it)
    }
    if (stage) {
        const double2* src = reinterpret_cast<const double2*>(stage);
        double2* dst = reinterpret_cast<double2*>(V.states);
        for (int k = t; k < n10 / 2; k += stride) dst[k] = src[k];
        if (t == 0) V.sc[0].lam[V.par] = stage[n10];
    }
    if (clear0) {
        for (int64_t k = t; k < (int64_t)V.W * kSelBins; k += stride) hist0_of(V, (int)(k / kSelBins), V.par)[k % kSelBins] = 0u;
    }
}

void launch_reset_calls(const DevView& V, hipStream_t s, const double* stage, int n10, int clear0) {
    int64_t items = V.W;
    if (stage) items = std::max<int64_t>(items, n10 / 2);
    if (clear0) items = std::max<int64_t>(items, (int64_t)V.W * kSelBins);
    const int nb = (int)std::min<int64_t>((items + 255) / 256, 1024);       // (grid-stride loops: a longer list is walked)
    hipLaunchKernelGGL(k_reset_calls, dim3(nb), dim3(256), 0, s, V, stage, n10, clear0);
}

// Digit-0 histogram of parity V.par (a warm histogram left by a trial whose states were then replaced, or one that a
// repeated select is about to rebuild by exponent) and, which == 1, digits 1 and 2 as well (an exact select that no
// trial followed).  which == 2: only the windows whose warm select missed.
__global__ __launch_bounds__(1024) void k_clear_hist(DevView V, int which) {
    const int w = blockIdx.x;
    if (which == 2 && !V.sc[w].miss) return;
    unsigned* h0 = hist0_of(V, w, V.par);
    for (int b = threadIdx.x; b < kSelBins; b += 1024) h0[b] = 0u;
    if (which == 1) {
        unsigned* h12 = histd_of(V, w, 1);
        for (int b = threadIdx.x; b < 2 * kSelBins; b += 1024) h12[b] = 0u;
    }
}

void launch_clear_hist(const DevView& V, int which, hipStream_t s) {
    hipLaunchKernelGGL(k_clear_hist, dim3(V.W), dim3(1024), 0, s, V, which);
}

}  // namespace vba
