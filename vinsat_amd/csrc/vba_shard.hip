// vba_shard.hip -- glue kernels of the observation-sharded multi-GPU mode.
//
// Every rank owns a contiguous slice of the observation rows.  Per BA() call three small device buffers are
// exchanged with all-gathers (RCCL, issued by the host side on the same stream) and reduced in rank order, so
// all ranks hold bit-identical normal equations and take the same LM decisions:
//   |r| keys (2 m_local doubles)  ->  exact global lower median
//   partial = [sum w J^T J (21 n) | sum w J^T r (6 n) | max raw weight | sum |r_obs|]
//   trial   = [sum |w r_obs'| local, sqrt(Sigma) sum |r_pred'|]
// Carried keys (vba_sh_run_schedule) exchange bin buckets and block sums instead: k_sh_front, k_sh_clear_miss below.
#include "vba_device.h"
#include "vba_launch.h"
#include "vba_select_body.h"

namespace vba {

__global__ __launch_bounds__(256) void k_shard_pack(DevView V, double* out) {
    __shared__ double red[4];
    const int n = V.n[0];
    const int cnt = 27 * n;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < cnt; e += gridDim.x * 256)
        out[e] = e < 21 * n ? V.Hraw[e] : V.braw[e - 21 * n];
    if (blockIdx.x == 0) {
        double s = 0.0;
        for (int b = threadIdx.x; b < V.nblk_obs; b += 256) s += V.part_init[b];
        const double t = block_sum<256>(s, red);
        if (threadIdx.x == 0) {
            out[cnt] = bits_f64(V.sc[0].wmax_bits[V.par]);
            out[cnt + 1] = t;
        }
    }
}

// with_sum == 0: the slot of sum |r_obs| is not in use (carried keys: the sum came with the trial's exchange)
__global__ __launch_bounds__(256) void k_shard_reduce(DevView V, const double* all, int ranks, int with_sum) {
    const int n = V.n[0];
    const int cnt = 27 * n;
    const int64_t stride = cnt + 2;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < cnt; e += gridDim.x * 256) {
        double s = 0.0;
        for (int q = 0; q < ranks; ++q) s += all[q * stride + e];   // fixed rank order
        if (e < 21 * n) V.Hraw[e] = s; else V.braw[e - 21 * n] = s;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double mx = 0.0, sa = 0.0;
        for (int q = 0; q < ranks; ++q) {
            mx = fmax(mx, all[q * stride + cnt]);
            sa += all[q * stride + cnt + 1];
        }
        V.sc[0].wmax_bits[V.par] = f64_bits(mx);
        if (with_sum) V.sc[0].sum_in[V.par] = sa;
    }
}

__global__ __launch_bounds__(64) void k_shard_trial_sum(DevView V, double* out) {
    const int lane = threadIdx.x;
    double so = 0.0, sd = 0.0;
    for (int b = lane; b < V.nblk_obs; b += 64) so += V.part_trial[b];
    for (int b = lane; b < V.nblk_dyn + (V.prm.initialize ? 0 : V.nblk_long); b += 64) sd += V.part_trial[V.nblk_obs + b];
    so = wave_sum(so);
    sd = wave_sum(sd);
    if (lane == 0) { out[0] = so; out[1] = sd; }
}

void launch_shard_pack(const DevView& V, double* out, hipStream_t s) {
    hipLaunchKernelGGL(k_shard_pack, dim3(64), dim3(256), 0, s, V, out);
}
void launch_shard_reduce(const DevView& V, const double* all, int ranks, hipStream_t s, int with_sum) {
    hipLaunchKernelGGL(k_shard_reduce, dim3(64), dim3(256), 0, s, V, all, ranks, with_sum);
}
void launch_shard_trial_sum(const DevView& V, double* out, hipStream_t s) {
    hipLaunchKernelGGL(k_shard_trial_sum, dim3(1), dim3(64), 0, s, V, out);
}

// ---------------------------------------------------------------------------------------------- sharded mode: front of a carried call
// Observation-sharded window, carried-keys protocol (vba_sh_run_schedule).  The trial kernel of every rank has left the keys of
// ITS rows in bin buckets, their warm histogram and its block sums in the rank's exchange buffer; `gathered` holds those of
// all R ranks (one all-gather of ~10 kB per rank instead of 16 B per observation).  One block, the same arithmetic on the same
// data on every rank, so every rank decides alike:
//   fold     the accept test of the call in front on the gathered block sums (observation part: every rank's; pose-chain
//            part: rank 0's -- all ranks computed the same); a first trial that is not cleanly accepted leaves everything
//            untouched and the window stalls there for the host's LM loop;
//   resolve  the R histograms are added up (integers), the bin of the global lower median is found, and this rank's bucket
//            of that bin goes into `bucket_out` = [count, keys ...] for the second (and last key-sized) exchange; a rank whose
//            bucket overflowed, a bin longer than 1024 keys over all ranks or a rank outside the binned range is a MISS: the
//            call takes the exact select over all keys instead (rank-consistent: the decision uses gathered data only).
// Layout of a rank's slot of `gathered` (doubles): [hist: 1024 (2048 u32) | part_next: nblk_obs | part_trial: nblk_obs + nblk_dyn].
__global__ __launch_bounds__(256) void k_sh_front(DevView V, const double* gathered, int ranks, int slot_len, double* bucket_out, int do_fold,
                                                  int do_resolve) {
    __shared__ unsigned lds_u[260];
    __shared__ double red[5][4];
    __shared__ unsigned over;
    const int w = 0, t = threadIdx.x;
    WinScalars& sc = V.sc[w];
    const int off_next = 1024, off_trial = 1024 + V.nblk_obs;
    // Everything this kernel reads is requested FIRST (the addresses depend on nothing it learns later): the scalars of the
    // window, the block sums and histograms of all ranks, this rank's own histogram, the inputs of the accept test -- one
    // round trip to memory instead of a chain of five (one block: nobody hides a latency here).
    const int seen_call = sc.call_idx, seen_pending = sc.pending, seen_miss = sc.miss;
    const int pc = V.par ^ 1;
    const double lam_in = sc.lam[pc], so_in = sc.sum_in[pc];
    const unsigned fl_in = sc.fl[pc];
    const unsigned long long lo = sc.warm_lo[V.par];
    double s_next = 0.0, s_trial = 0.0, s_pred = 0.0;
    for (int q = 0; q < ranks; ++q) {
        const double* slot = gathered + (size_t)q * slot_len;
        for (int b = t; b < V.nblk_obs; b += 256) { s_next += slot[off_next + b]; s_trial += slot[off_trial + b]; }
    }
    for (int b = t; b < V.nblk_dyn + (V.prev.initialize ? 0 : V.nblk_long); b += 256) s_trial += gathered[off_trial + V.nblk_obs + b];
    if (do_fold && !V.prev.initialize) {
        const double* pp = V.part_pred + ((size_t)w * 2 + pc) * V.pred_stride;
        for (int b = t; b < V.nblk_pred + V.nblk_long; b += 256) s_pred += pp[b];
    }
    unsigned hl[8], mine[8];
    if (do_resolve) {
        const uint4* own4 = reinterpret_cast<const uint4*>(hist0_of(V, w, V.par)) + 2 * t;
        const uint4 o0 = own4[0], o1 = own4[1];
        mine[0] = o0.x; mine[1] = o0.y; mine[2] = o0.z; mine[3] = o0.w; mine[4] = o1.x; mine[5] = o1.y; mine[6] = o1.z; mine[7] = o1.w;
#pragma unroll
        for (int j = 0; j < 8; ++j) hl[j] = 0u;
        for (int q = 0; q < ranks; ++q) {
            const uint4* g4 = reinterpret_cast<const uint4*>(gathered + (size_t)q * slot_len) + 2 * t;
            const uint4 g0 = g4[0], g1 = g4[1];
            hl[0] += g0.x; hl[1] += g0.y; hl[2] += g0.z; hl[3] += g0.w; hl[4] += g1.x; hl[5] += g1.y; hl[6] += g1.z; hl[7] += g1.w;
        }
    }
    if (do_fold) {
        if (!(V.call >= 0 && seen_pending == V.call - 1 && seen_call == V.call - 1)) return;
    } else {
        if (!((V.call < 0 || seen_call == V.call) && (V.redo == 2 || (seen_miss != 0) == (V.redo != 0)))) return;     // VBA_SKIP_CALL on the snapshot
    }
    if (do_fold) {
        DecideIn in;
        in.s_pred = s_pred;
        in.s_prior = 0.0;
        in.s_trial = s_trial;
        in.s_next = s_next;
        in.lam_in = lam_in;
        in.so = so_in;
        in.flags = fl_in;
        const DecideOut d = decide_finish(V, w, in, V.prev, 0, 0.0, nullptr, 0, red);
        if (!(d.accept && !(d.flags & (2u | 8u | 32u)))) return;        // not clean: no trace
        fold_commit(V, w, d);
        if (!do_resolve && t == 0) {                    // the last call of a schedule: decided, nothing begins
            sc.pending = -1;
            sc.n_trials = 1;                            // (vba_get_states reports the decided call's)
            sc.done = 1;
        }
    } else if (do_resolve) {
        // (the call in front was decided by k_decide, which knows this rank's part only)
        const double v = wave_sum(s_next);
        __syncthreads();
        if ((t & 63) == 0) red[0][t >> 6] = v;
        __syncthreads();
        if (t == 0) sc.sum_in[V.par] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    }
    if (!do_resolve) return;
    if (t == 0) over = 0u;
    __syncthreads();
    const int64_t count = 2 * V.m_total;
    unsigned long long prefix;
    long long rank;
    unsigned in_bin;
    select_resolve_loaded(hl, kSelBins, 11, 0ull, (count - 1) / 2, prefix, rank, lds_u, &in_bin);
    const unsigned bin = (unsigned)prefix;
    // every rank's bucket of that bin must be complete
    if ((unsigned)(t * 8) <= bin && bin < (unsigned)(t * 8 + 8)) {
        for (int q = 0; q < ranks; ++q)
            if (reinterpret_cast<const unsigned*>(gathered + (size_t)q * slot_len)[bin] > (unsigned)V.bucket_cap) over = 1u;
    }
    __syncthreads();
    const bool hit = lo != ~0ull && bin >= 1u && bin <= 2046u && in_bin <= 1024u && !over && !V.warm_force_miss;
    if (t == 0) {
        front_commit(V, w, hit, bin, rank, in_bin, false);
        if (hit) sc.sel_cnt = in_bin;
        if (V.wmax_ext) *V.wmax_ext = 0ull;
    }
    if (!hit) return;
    // this rank's bucket of the bin: [count, keys ...]
    unsigned my_cnt = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) if ((unsigned)(t * 8 + j) == bin) my_cnt = mine[j];
    __syncthreads();
    if ((unsigned)(t * 8) <= bin && bin < (unsigned)(t * 8 + 8)) lds_u[20] = my_cnt;
    __syncthreads();
    const unsigned cnt = lds_u[20];
    const double* bucket = V.wbucket + (((size_t)w * 2 + V.par) * kSelBins + bin) * (size_t)V.bucket_cap;
    if (t == 0) bucket_out[0] = (double)cnt;
    for (unsigned q = t; q < cnt; q += 256) bucket_out[1 + q] = bucket[q];
}
void launch_sh_front(const DevView& V, const double* gathered, int ranks, int slot_len, double* bucket_out, int do_fold, int do_resolve, hipStream_t s) {
    hipLaunchKernelGGL(k_sh_front, dim3(1), dim3(256), 0, s, V, gathered, ranks, slot_len, bucket_out, do_fold, do_resolve);
}

// a call that missed its warm select is repeated with the exact select over all keys: the window takes part again
__global__ void k_sh_clear_miss(DevView V) {
    V.sc[0].miss = 0;
    V.sc[0].fl[V.par] = 0u;
    V.host_head[0].flags = 0u;
}
void launch_sh_clear_miss(const DevView& V, hipStream_t s) { hipLaunchKernelGGL(k_sh_clear_miss, dim3(1), dim3(1), 0, s, V); }

}  // namespace vba
