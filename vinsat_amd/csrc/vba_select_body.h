// vba_select_body.h -- device bodies of the median select that more than one unit needs (gfx950).
//
//   begin_call_scalars                    the scalars a call starts from (k_obs_residual, k_select_pass<1>, front_commit)
//   fold_decide / fold_load / fold_decide_loaded / fold_commit
//                                         the accept test of the call in front, folded into the kernel that starts the next
//                                         call (k_select_warm, k_obs_accumulate, k_sh_front)
//   front_resolve / front_commit / warm_front
//                                         the warm histogram resolved to the bin of the wanted rank, and what that leaves
//   select_finish_list / select_finish    the select finished on a short list (k_select_finish, k_obs_accumulate)
//
// The kernels: vba_select.hip (k_select_pass, k_select_warm, k_select_finish), vba_accumulate.hip, vba_shard.hip.
#pragma once
#include "vba_decide.h"
#include "vba_device.h"

namespace vba {

// Per-call state that must be clean before the first kernel touches it:
//   * digit-0 histogram of the call's parity: zeroed by k_obs_accumulate / k_select_finish of the call that consumed it last
//     -- with the inline select by that call's k_trial, the accumulation's blocks are still reading it -- (and by the
//     allocation); digits 1, 2: zeroed by k_trial;
//   * scalars (done, n_trials, flags, max weight): reset by thread 0 of block 0 of the call's first kernel
//     (k_obs_residual, k_select_warm, k_select_pass<1> of a repeated select, or -- inline select -- k_obs_accumulate at its
//     end, except the max weight: per parity, cleared by the previous call's k_trial); no other block of that kernel reads them;
//   * the length of the compacted list: reset by the kernel in FRONT of the one that appends (k_obs_residual /
//     k_select_pass<1>, or the previous call's k_trial for k_select_warm).
// keep_wmax: the caller is a block of the accumulation itself (inline select): other blocks of the same kernel may
// already have entered their maximum, the slot was cleared by the previous call's trial kernel instead
__device__ __forceinline__ void begin_call_scalars(WinScalars& sc, int par, bool keep_wmax = false) {
    sc.done = 0;
    sc.n_trials = 0;
    sc.fl[par] = 0u;
    if (!keep_wmax) sc.wmax_bits[par] = 0ull;
    sc.sum_abs_rpred = 0.0;
}

// ---------------------------------------------------------------------------------------------- A3a: front of a call on carried keys
// Evaluated by the kernel that starts the call: every block of k_select_warm (warm_front), or, with the bin buckets (inline
// select), k_obs_accumulate itself, whose extra block takes the accept test and the record off the other blocks.  Chained schedule (V.fold, fold_here): first the accept test of the call in front
// (vba_decide.h); a first trial that was cleanly accepted lets the window move on to this call at once, one that was not
// leaves everything untouched (kWarmSkip).  Then the warm histogram the trial left behind is resolved to the bin of the
// wanted rank, and one thread records the outcome.  A rank outside the binned range, or a bin longer than `list_cap`, is a
// miss: the window waits (sc.miss) until the host has repeated this call's select with the exact digits.
enum { kWarmSkip = 0, kWarmHit = 1, kWarmMiss = 2 };

// the accept test of the call in front (all threads); clean = its first trial was accepted with nothing to repair
__device__ __forceinline__ bool fold_decide(const DevView& V, int w, double (*red)[4], DecideOut& d) {
    d = decide_eval(V, w, V.par ^ 1, V.prev, 0, 0.0, nullptr, 0, red);
    return d.accept && !(d.flags & (2u | 8u | 32u));
}
// ... with its inputs loaded earlier (fold_load)
__device__ __forceinline__ DecideIn fold_load(const DevView& V, int w) { return decide_load(V, w, V.par ^ 1, V.prev, 0); }
__device__ __forceinline__ bool fold_decide_loaded(const DevView& V, int w, const DecideIn& in, double (*red)[4], DecideOut& d) {
    d = decide_finish(V, w, in, V.prev, 0, 0.0, nullptr, 0, red);
    return d.accept && !(d.flags & (2u | 8u | 32u));
}
// ... and what a clean one leaves behind (block 0 only): the window moves on to this call
__device__ __forceinline__ void fold_commit(const DevView& V, int w, const DecideOut& d) {
    WinScalars& sc = V.sc[w];
    const int t = threadIdx.x, par = V.par;
    const double lam32 = sc.lam32;      // of the decided call's solve
    if (t < 81) {
        const double hv = V.lastD[(size_t)w * 81 + t] + ((t / 9 == t % 9) ? lam32 : 0.0);
        sc.last_hessian[t] = hv;
        if (V.host_states) V.host_head[w].last_hessian[t] = hv;     // (a pipelined call reads its result from host memory)
    }
    if (t == 0) {
        sc.lam[par] = d.lam_out;
        sc.sum_in[par] = d.sum_next;
        sc.init_residual = d.init_residual;
        sc.trial_residual = d.residual;
        sc.call_idx = V.call;
        WinHead& hh = V.host_head[w];
        hh.lamda = d.lam_out;
        hh.trial_residual = d.residual;
        hh.n_trials = 1;
        hh.flags = d.flags;
        hh.done = 1;
        hh.call_idx = V.call;
    }
}
// the scalars of the call that begins (one thread): the selected bin, or the miss
__device__ __forceinline__ void front_commit(const DevView& V, int w, bool hit, unsigned bin, long long rank, unsigned in_bin, bool inline_select) {
    WinScalars& sc = V.sc[w];
    const int par = V.par;
    begin_call_scalars(sc, par, inline_select);
    if (hit) {
        sc.sel_mode = 1;
        sc.sel_rank[2] = rank;
        sc.warm_base = sc.warm_lo[par] + ((unsigned long long)(bin - 1u) << V.warm_shift);
        if (inline_select) sc.sel_cnt = in_bin;
    } else {
        sc.miss = 1;
        sc.fl[par] = 32u;
        V.host_head[w].flags = 32u;
        V.host_head[w].done = 0;
    }
}
// the warm histogram resolved to the bin of the wanted rank (all threads; hloc: select_load of hist0[par])
__device__ __forceinline__ bool front_resolve(const DevView& V, int w, const unsigned (&hloc)[8], long long list_cap, unsigned* lds_u,
                                              unsigned& bin, long long& rank, unsigned& in_bin) {
    const int64_t count = 2 * (int64_t)V.m[w];
    const unsigned long long lo = V.sc[w].warm_lo[V.par];
    unsigned long long prefix;
    select_resolve_loaded(hloc, kSelBins, 11, 0ull, (count - 1) / 2, prefix, rank, lds_u, &in_bin);
    bin = (unsigned)prefix;
    return lo != ~0ull && bin >= 1u && bin <= 2046u && (int64_t)in_bin <= list_cap && !V.warm_force_miss;
}

// in order: accept test, then this call's select (k_select_warm)
__device__ __forceinline__ int warm_front(const DevView& V, int w, bool fold_here, long long list_cap, double (*red)[4],
                                          unsigned* lds_u, unsigned& bin_out, long long& rank_out, unsigned& in_bin_out) {
    unsigned hloc[8];
    select_load(hist0_of(V, w, V.par), kSelBins, hloc);        // in flight while the accept test is evaluated
    if (fold_here) {
        DecideOut d;
        if (!fold_decide(V, w, red, d)) return kWarmSkip;      // not a clean first trial: the host finishes that call
        if (blockIdx.x == 0) fold_commit(V, w, d);
    }
    const bool hit = front_resolve(V, w, hloc, list_cap, lds_u, bin_out, rank_out, in_bin_out);
    if (blockIdx.x == 0 && threadIdx.x == 0) front_commit(V, w, hit, bin_out, rank_out, in_bin_out, false);
    return hit ? kWarmHit : kWarmMiss;
}

// Finishes the select on the compacted list (the keys that k_select_pass<2, true> found to match digits 0 and 1, key >> 42;
// digit 2 of the wanted key is known from that pass's histogram): returns the lower median c_obs to every thread of the
// (256-thread) block.  It is the prologue of k_obs_accumulate -- every block of a window redoes it (a handful of keys:
// rank by counting) instead of one more single-block kernel on the critical path; long lists (massive ties) take digits
// 3, 4, 5 with a block-local histogram each, the full key array if the list overflowed -- at any length: in sharded mode
// the list has room for this rank's rows and is filled from the gathered keys of all ranks, so a list of a few hundred
// keys can have overflowed (tests/test_gpu_sharded_stages.py).  A list made by k_select_warm (one warm bin) is ranked by
// counting while short, by radix digits of the offset inside the bin otherwise.
// ck: the list (capacity `cap` entries, cnt of them valid -- cnt > cap: it overflowed), want: the rank wanted among them,
// mode 0: keys sharing digits 0 and 1 of an exact select, 1: the keys of one warm bin starting at warm_base.
// speculate: load the first 1024 entries before cnt is known to the caller's satisfaction (one round trip instead of two).
__device__ __forceinline__ double select_finish_list(const DevView& V, int w, const double* ck, int64_t cap, unsigned cnt, long long want,
                                                     int mode, unsigned long long warm_base, bool speculate, unsigned* lh /*[kSelBins]*/,
                                                     unsigned* lds_u /*[260]*/, unsigned long long* skeys /*[1024] + 1*/) {
    const WinScalars& sc = V.sc[w];
    // latency mode loads the first 1024 entries speculatively together with the length (one round trip instead of two);
    // with many windows per launch every block of every window would drag 8 KB through the caches for a handful of keys
    unsigned long long pre[4];
    if (V.sel_nslots > 0 && ck == V.sel_slots) {
        // sharded mode: the list is the concatenation of the ranks' buckets of one warm bin, slot r = [count_r, keys ...];
        // entry q of the list lives in the slot whose running count covers it (cnt <= 1024 is guaranteed by the front)
        unsigned lo_q = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) pre[j] = 0ull;
        for (int r = 0; r < V.sel_nslots; ++r) {
            const double* slot = ck + (size_t)r * V.sel_slot_stride;
            const unsigned c_r = (unsigned)slot[0];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned q = threadIdx.x + 256u * j;
                if (q >= lo_q && q < lo_q + c_r && q < cnt) pre[j] = f64_bits(slot[1 + (q - lo_q)]);
            }
            lo_q += c_r;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned q = threadIdx.x + 256u * j;
            pre[j] = ((int64_t)q < cap && (speculate || q < cnt)) ? f64_bits(ck[q]) : 0ull;
        }
    }
    if (mode == 1 && cnt <= 1024u && V.warm_shift >= 8) {
        // One warm bin: every key is warm_base + rel, rel < 2^warm_shift.  Ranking ~130 keys by counting is a serial loop of
        // ~130 LDS reads per thread on the critical path of every call; instead the top 8 bits of rel split the list over 256
        // sub-bins (one LDS atomic per key, one sub-bin per thread for the scan), and only the handful of keys in the sub-bin
        // of the wanted rank is ranked by counting.  Exact either way: the same key comes out.
        const int t = threadIdx.x;
        const int sh = V.warm_shift - 8;
        lh[t] = 0u;
        if (t == 0) { lds_u[16] = 0u; lds_u[17] = 0u; lds_u[18] = 0u; }
        __syncthreads();
        unsigned sb4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned q = t + 256u * j;
            sb4[j] = (unsigned)((pre[j] - warm_base) >> sh) & 255u;
            if (q < cnt) atomicAdd(&lh[sb4[j]], 1u);
        }
        __syncthreads();
        const unsigned c = lh[t];
        const unsigned inc = wave_inclusive_scan_u32(c);
        if ((t & 63) == 63) lds_u[t >> 6] = inc;
        __syncthreads();
        unsigned base = 0;
        for (int q = 0; q < (t >> 6); ++q) base += lds_u[q];
        const long long excl = (long long)base + inc - c;
        if (want >= excl && want < excl + (long long)c) { lds_u[16] = (unsigned)t; lds_u[17] = (unsigned)(want - excl); }
        __syncthreads();
        const unsigned tb = lds_u[16], r = lds_u[17];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned q = t + 256u * j;
            if (q < cnt && sb4[j] == tb) {
                const unsigned slot = atomicAdd(&lds_u[18], 1u);
                skeys[slot] = pre[j];       // (the order inside the list does not matter: equal keys are the same value)
            }
        }
        __syncthreads();
        const unsigned k = lds_u[18];
        for (unsigned q = t; q < k; q += 256) {
            const unsigned long long key = skeys[q];
            unsigned below = 0;
            for (unsigned j = 0; j < k; ++j) {
                const unsigned long long o = skeys[j];
                below += (o < key) || (o == key && j < q);
            }
            if (below == r) skeys[1024] = key;
        }
        __syncthreads();
        return bits_f64(skeys[1024]);
    }
    // (an exact-mode list that overflowed -- cnt > cap, sharded mode: the list is sized for this rank's rows and filled from the
    // keys of all ranks -- holds only its first `cap` entries, however short it is: it goes to the fallback below)
    if (cnt <= (mode ? (unsigned)kWarmCount : 1024u) && (mode != 0 || (int64_t)cnt <= cap)) {
        // the wanted key is the one of rank `want` among the list -- rank each key by counting (ties broken by position)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned q = threadIdx.x + 256u * j;
            if (q < cnt) skeys[q] = pre[j];
        }
        __syncthreads();
        for (unsigned q = threadIdx.x; q < cnt; q += 256) {
            const unsigned long long key = skeys[q];
            long long below = 0;
            for (unsigned j = 0; j < cnt; ++j) {
                const unsigned long long o = skeys[j];
                below += (o < key) || (o == key && j < q);
            }
            if (below == want) skeys[1024] = key;
        }
        __syncthreads();
        return bits_f64(skeys[1024]);
    }
    if (mode == 1) {
        // a long warm bin: every key is warm_base + rel with rel < 2^warm_shift; radix digits of rel from the top, 11 bits at
        // a time, with a block-local histogram each
        unsigned long long prefix = 0ull;
        long long rank = want;
        int remaining = V.warm_shift;
        if (remaining > 11) {
            // first digit, then -- the usual case: thousands of keys spread over 2048 sub-bins -- the handful of keys of the
            // wanted sub-bin is gathered in LDS and ranked by counting: two passes over the list instead of one per digit
            remaining -= 11;
            for (int b = threadIdx.x; b < kSelBins; b += 256) lh[b] = 0u;
            if (threadIdx.x == 0) lds_u[18] = 0u;
            __syncthreads();
            for (unsigned q = threadIdx.x; q < cnt; q += 256) {
                const unsigned long long rel = f64_bits(ck[q]) - warm_base;
                atomicAdd(&lh[(unsigned)(rel >> remaining) & 2047u], 1u);
            }
            __syncthreads();
            unsigned sub_cnt;
            {
                unsigned loc[8];
                select_load(lh, kSelBins, loc);
                select_resolve_loaded(loc, kSelBins, 11, 0ull, rank, prefix, rank, lds_u, &sub_cnt);
            }
            if (sub_cnt <= 1024u) {
                for (unsigned q = threadIdx.x; q < cnt; q += 256) {
                    const unsigned long long key = f64_bits(ck[q]);
                    if (((key - warm_base) >> remaining) == prefix) skeys[atomicAdd(&lds_u[18], 1u)] = key;
                }
                __syncthreads();
                for (unsigned q = threadIdx.x; q < sub_cnt; q += 256) {
                    const unsigned long long key = skeys[q];
                    long long below = 0;
                    for (unsigned j = 0; j < sub_cnt; ++j) {
                        const unsigned long long o = skeys[j];
                        below += (o < key) || (o == key && j < q);
                    }
                    if (below == rank) skeys[1024] = key;
                }
                __syncthreads();
                return bits_f64(skeys[1024]);
            }
        }
        while (remaining > 0) {
            const int width = remaining < 11 ? remaining : 11;
            remaining -= width;
            const int nbins = 1 << width;
            for (int b = threadIdx.x; b < kSelBins; b += 256) lh[b] = 0u;
            __syncthreads();
            for (unsigned q = threadIdx.x; q < cnt; q += 256) {
                const unsigned long long rel = f64_bits(ck[q]) - warm_base;
                if ((rel >> (remaining + width)) == prefix) atomicAdd(&lh[(unsigned)(rel >> remaining) & (nbins - 1)], 1u);
            }
            __syncthreads();
            unsigned long long np;
            long long nr;
            select_resolve(lh, nbins, width, prefix, rank, np, nr, lds_u);
            prefix = np;
            rank = nr;
        }
        return bits_f64(warm_base + prefix);
    }
    if ((int64_t)cnt > 2 * V.m_max) {       // list overflowed: fall back to the full key array
        ck = V.abs_all ? V.abs_all : V.absr + 2 * (size_t)w * V.m_max;
        cnt = (unsigned)(V.abs_all ? V.abs_all_count : 2 * (int64_t)V.m[w]);
    }
    unsigned long long prefix;
    long long rank;
    select_resolve(histd_of(V, w, 2), 1 << sel_width(2), sel_width(2), sc.sel_prefix[2], sc.sel_rank[2], prefix, rank, lds_u);
#pragma unroll
    for (int P = 3; P < 6; ++P) {
        const int nbins = 1 << sel_width(P);
        for (int b = threadIdx.x; b < kSelBins; b += 256) lh[b] = 0u;
        __syncthreads();
        for (unsigned q = threadIdx.x; q < cnt; q += 256) {
            const unsigned long long key = f64_bits(ck[q]);
            if ((key >> sel_shift(P - 1)) == prefix) atomicAdd(&lh[(unsigned)(key >> sel_shift(P)) & (nbins - 1)], 1u);
        }
        __syncthreads();
        unsigned long long np;
        long long nr;
        select_resolve(lh, nbins, sel_width(P), prefix, rank, np, nr, lds_u);
        prefix = np;
        rank = nr;
    }
    return bits_f64(prefix);
}

// The list the select kernels of this call left (k_select_pass<2> / k_select_warm): its length, the wanted rank and the
// first entries are loaded together.
__device__ __forceinline__ double select_finish(const DevView& V, int w, unsigned* lh /*[kSelBins]*/, unsigned* lds_u /*[260]*/,
                                                unsigned long long* skeys /*[1024] + 1*/) {
    const WinScalars& sc = V.sc[w];
    if (V.sel_nslots > 0)       // sharded mode, carried keys: the ranks' buckets of the median's bin as gathered
        return select_finish_list(V, w, V.sel_slots, 1024, sc.sel_cnt, sc.sel_rank[2], 1, sc.warm_base, false, lh, lds_u, skeys);
    return select_finish_list(V, w, V.ckeys + 2 * (size_t)w * V.m_max, 2 * V.m_max, sc.sel_cnt, sc.sel_rank[2], sc.sel_mode, sc.warm_base,
                              V.lat != 0, lh, lds_u, skeys);
}

}  // namespace vba
