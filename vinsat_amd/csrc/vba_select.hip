// vba_select.hip -- A3a, the exact lower median of the 2m |r| keys of a window (gfx950).
//
//   k_select_pass<P>   exact select by most-significant-digit radix select: digit 0 (exponent) is histogrammed inside
//                      k_obs_residual (vba_obs.hip), digits 1 and 2 read the keys once each, the second of them compacting
//                      the (few) keys that match digits 0 and 1 (key >> 42), and select_finish finishes digits 3..5 on that short list
//   k_select_warm      on carried keys: the trial that produced the keys binned them around the median of its own call
//                      (warm_bin, vba_device.h), so ONE pass compacts the bin of the wanted rank; in a chained schedule its
//                      prologue is the accept test of the call in front (vba_decide.h).  Batched handles; latency mode keeps
//                      the keys in per-bin buckets instead and selects inside the accumulation (vba_accumulate.hip)
//   k_select_finish    many windows: the select finished once per window (one block each) instead of in every
//                      accumulation block
//
// The device bodies these share with the accumulation and the sharded front: vba_select_body.h.
#include "vba_launch.h"
#include "vba_select_body.h"

namespace vba {

// ---------------------------------------------------------------------------------------------- exact select
// COMPACT: additionally append the keys that match the digits known so far to the short list V.ckeys.
// ITEMS keys per thread: 8 keeps a single window spread over many blocks (latency), 32 amortises the per-block
// prologue (histogram scan, LDS clear, flush) when many windows are batched.
template <int P, bool COMPACT, int ITEMS>
__global__ __launch_bounds__(256) void k_select_pass(DevView V) {
    __shared__ unsigned lh[kSelBins];
    __shared__ unsigned lds_u[260];
    __shared__ double red[kObsBlock / 64];
    const int w = blockIdx.y;
    VBA_SKIP_CALL(V, w);
    const double* keys = V.abs_all ? V.abs_all : V.absr + 2 * (size_t)w * V.m_max;
    const int64_t count = V.abs_all ? V.abs_all_count : 2 * (int64_t)V.m[w];
    // carried keys (a select repeated with the exact digits): k_obs_residual did not run, this kernel owns the resets
    if (P == 1 && V.carry && blockIdx.x == 0 && threadIdx.x == 0) {
        begin_call_scalars(V.sc[w], V.par);
        V.sc[w].sel_cnt = 0u;
    }
    // sum |r_obs| at the input states for the accept test: fixed-order sum of k_obs_residual's block partials
    // (carried keys bring it along; sharded mode gets the sum over all ranks from k_shard_reduce)
    if (P == 1 && !V.carry && V.m_total == 0 && blockIdx.x == 0) {
        const double* pi = V.part_init + (size_t)w * V.nblk_obs;
        double s_init = 0.0;
        for (int b = threadIdx.x; b < V.nblk_obs; b += 256) s_init += pi[b];
        const double tot = block_sum<256>(s_init, red);
        if (threadIdx.x == 0) V.sc[w].sum_in[V.par] = tot;
    }
    if ((int64_t)blockIdx.x * 256 * ITEMS >= count) return;
    auto digit_hist = [&](int d) { return d == 0 ? hist0_of(V, w, V.par) : histd_of(V, w, d); };
    constexpr int nbins = 1 << sel_width(P);
    for (int b = threadIdx.x; b < nbins; b += 256) lh[b] = 0u;
    // few keys per thread (single window, latency matters): their loads are issued before the histogram of the
    // previous digit is resolved, not after
    // keys are read two at a time (16 bytes per lane: 8-byte accesses stream at little more than half that rate); the
    // number of keys is even (two per observation row)
    constexpr bool PRELOAD = ITEMS <= 8;
    constexpr int PAIRS = ITEMS / 2;
    const double2* keys2 = reinterpret_cast<const double2*>(keys);
    const int64_t npair = count / 2;
    double2 pk[PRELOAD ? PAIRS : 1];
    if (PRELOAD) {
#pragma unroll
        for (int it = 0; it < PAIRS; ++it) {
            const int64_t idx = ((int64_t)blockIdx.x * PAIRS + it) * 256 + threadIdx.x;
            pk[it] = idx < npair ? keys2[idx] : make_double2(0.0, 0.0);
        }
    }
    unsigned long long prefix = 0ull;
    // torch.median = lower median (BA_filtering.py:23); in sharded mode the gathered buffer may end in +inf padding
    long long rank = ((V.m_total ? 2 * V.m_total : count) - 1) / 2;
    if (P > 0) {
        constexpr int Q = P > 0 ? P - 1 : 0;
        select_resolve(digit_hist(Q), 1 << sel_width(Q), sel_width(Q), V.sc[w].sel_prefix[Q], V.sc[w].sel_rank[Q],
                       prefix, rank, lds_u);
    } else {
        __syncthreads();
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        V.sc[w].sel_prefix[P] = prefix;
        V.sc[w].sel_rank[P] = rank;
        if (COMPACT) V.sc[w].sel_mode = 0;
    }
    auto take = [&](unsigned long long key, bool have) {
        bool match = have;
        if (P > 0) match = have && (key >> sel_shift(P > 0 ? P - 1 : 0)) == prefix;
        if (match) atomicAdd(&lh[(unsigned)(key >> sel_shift(P)) & (nbins - 1)], 1u);
        if (COMPACT) {
            // wave-aggregated append: one atomic per wave instruction
            const unsigned long long mask = __ballot(match);
            if (mask) {
                const int lane = threadIdx.x & 63;
                const int leader = __ffsll((long long)mask) - 1;
                unsigned base = 0;
                if (lane == leader) base = atomicAdd(&V.sc[w].sel_cnt, (unsigned)__popcll(mask));
                base = (unsigned)__builtin_amdgcn_readlane((int)base, leader);      // (leader is uniform: one v_readlane, not a crossbar shuffle)
                if (match) {
                    const unsigned off = (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
                    // the list has room for 2 m_max keys; if more match (massive ties) select_finish sees
                    // sel_cnt > capacity and rescans the full key array instead
                    if ((int64_t)base + off < 2 * V.m_max) V.ckeys[2 * (size_t)w * V.m_max + base + off] = bits_f64(key);
                }
            }
        }
    };
#pragma unroll 8
    for (int it = 0; it < PAIRS; ++it) {
        const int64_t idx = ((int64_t)blockIdx.x * PAIRS + it) * 256 + threadIdx.x;
        const bool have = idx < npair;
        const double2 kk = PRELOAD ? pk[it] : (have ? keys2[idx] : make_double2(0.0, 0.0));
        take(f64_bits(kk.x), have);
        take(f64_bits(kk.y), have);
    }
    __syncthreads();
    unsigned* hist_out = digit_hist(P);
    for (int b = threadIdx.x; b < nbins; b += 256) {
        const unsigned c = lh[b];
        if (c) atomicAdd(&hist_out[b], c);
    }
}

// digits 1 and 2 over the keys; digit 0 comes from k_obs_residual, or -- with_digit0 -- from a pass of its own: sharded
// mode's gathered keys, a select repeated after a warm miss
void launch_select(const DevView& V, bool with_digit0, hipStream_t s) {
    const int64_t count = V.abs_all ? V.abs_all_count : 2 * V.m_max;
    const dim3 b(256);
    if (!V.lat) {
        const int nb = (int)((count + 256 * 32 - 1) / (256 * 32));
        const dim3 g(nb > 0 ? nb : 1, V.W);
        if (with_digit0) hipLaunchKernelGGL((k_select_pass<0, false, 32>), g, b, 0, s, V);
        hipLaunchKernelGGL((k_select_pass<1, false, 32>), g, b, 0, s, V);
        hipLaunchKernelGGL((k_select_pass<2, true, 32>), g, b, 0, s, V);
    } else {
        const int nb = (int)((count + 256 * kSelItems - 1) / (256 * kSelItems));
        const dim3 g(nb > 0 ? nb : 1, V.W);
        if (with_digit0) hipLaunchKernelGGL((k_select_pass<0, false, kSelItems>), g, b, 0, s, V);
        hipLaunchKernelGGL((k_select_pass<1, false, kSelItems>), g, b, 0, s, V);
        hipLaunchKernelGGL((k_select_pass<2, true, kSelItems>), g, b, 0, s, V);
    }
}

// ---------------------------------------------------------------------------------------------- warm select
// One pass over carried keys: warm_front (accept test of the call in front, then the bin of the wanted rank), and the keys
// of that bin are compacted for select_finish.
#ifndef VBA_SELW_ITEMS
#define VBA_SELW_ITEMS 32       // keys per thread with many windows per launch (latency mode: kSelItems)
#endif
template <int ITEMS>
__global__ __launch_bounds__(256) void k_select_warm(DevView V) {
    __shared__ unsigned lds_u[260];
    __shared__ double red[5][4];
    const int w = blockIdx.y;
    WinScalars& sc = V.sc[w];
    const int t = threadIdx.x;
    const bool fold_here = V.call >= 0 && V.fold && sc.pending == V.call - 1 && sc.call_idx == V.call - 1;
    if (!fold_here) VBA_SKIP_CALL(V, w);
    const double* keys = V.absr + 2 * (size_t)w * V.m_max;
    const int64_t count = 2 * (int64_t)V.m[w];
    if ((int64_t)blockIdx.x * 256 * ITEMS >= count) return;         // (never block 0)
    // the keys of a short block are loaded before anything is decided (latency)
    constexpr bool PRELOAD = ITEMS <= 8;
    constexpr int PAIRS = ITEMS / 2;        // two keys (16 bytes) per load
    const double2* keys2 = reinterpret_cast<const double2*>(keys);
    const int64_t npair = count / 2;
    // (both forms request their keys before the histogram is resolved: the resolve is a dependent round trip plus a scan)
    double2 pk[PAIRS];
#pragma unroll
    for (int it = 0; it < PAIRS; ++it) {
        const int64_t idx = ((int64_t)blockIdx.x * PAIRS + it) * 256 + t;
        pk[it] = idx < npair ? keys2[idx] : make_double2(0.0, 0.0);
    }
    const unsigned long long lo = sc.warm_lo[V.par];
    unsigned bin, in_bin;
    long long rank;
    if (warm_front(V, w, fold_here, 2 * V.m_max, red, lds_u, bin, rank, in_bin) != kWarmHit) return;
    if constexpr (!PRELOAD) {
        // Many windows per launch, coarse warm bins (1/8 binade: a few per cent of the keys match).  A returning atomic per
        // wave instruction would be a chain of ITEMS dependent round trips; instead the block counts its matches first,
        // reserves its share of the list with ONE atomic and then writes.  The keys stay in registers in between.
        double2 (&kk)[PAIRS] = pk;
        unsigned long long mbits = 0ull;        // bit 2 it: kk[it].x matches, bit 2 it + 1: kk[it].y
#pragma unroll
        for (int it = 0; it < PAIRS; ++it) {
            const int64_t idx = ((int64_t)blockIdx.x * PAIRS + it) * 256 + t;
            const bool have = idx < npair;
            if (have && warm_bin(f64_bits(kk[it].x), lo, V.warm_shift) == bin) mbits |= 1ull << (2 * it);
            if (have && warm_bin(f64_bits(kk[it].y), lo, V.warm_shift) == bin) mbits |= 2ull << (2 * it);
        }
        const unsigned mine = (unsigned)__popcll(mbits);
        const unsigned inc = wave_inclusive_scan_u32(mine);
        __syncthreads();            // lds_u was read by the resolve above
        if ((t & 63) == 63) lds_u[t >> 6] = inc;
        __syncthreads();
        if (t == 0) {
            const unsigned total = lds_u[0] + lds_u[1] + lds_u[2] + lds_u[3];
            lds_u[4] = total ? atomicAdd(&sc.sel_cnt, total) : 0u;
        }
        __syncthreads();
        unsigned at = lds_u[4] + inc - mine;
        for (int q = 0; q < (t >> 6); ++q) at += lds_u[q];
        double* list = V.ckeys + 2 * (size_t)w * V.m_max;
#pragma unroll
        for (int it = 0; it < PAIRS; ++it) {
            if (mbits & (1ull << (2 * it))) list[at++] = kk[it].x;
            if (mbits & (2ull << (2 * it))) list[at++] = kk[it].y;
        }
        return;
    }
    auto take = [&](unsigned long long key, bool have) {
        const bool match = have && warm_bin(key, lo, V.warm_shift) == bin;
        const unsigned long long mask = __ballot(match);
        if (mask) {     // wave-aggregated append: one atomic per wave instruction
            const int lane = t & 63;
            const int leader = __ffsll((long long)mask) - 1;
            unsigned base = 0;
            if (lane == leader) base = atomicAdd(&sc.sel_cnt, (unsigned)__popcll(mask));
            base = (unsigned)__builtin_amdgcn_readlane((int)base, leader);      // (leader is uniform: one v_readlane, not a crossbar shuffle)
            if (match) V.ckeys[2 * (size_t)w * V.m_max + base + (unsigned)__popcll(mask & ((1ull << lane) - 1ull))] = bits_f64(key);
        }
    };
    if constexpr (PRELOAD) {
#pragma unroll 8
        for (int it = 0; it < PAIRS; ++it) {
            const int64_t idx = ((int64_t)blockIdx.x * PAIRS + it) * 256 + t;
            const bool have = idx < npair;
            take(f64_bits(pk[it].x), have);
            take(f64_bits(pk[it].y), have);
        }
    }
}

// (plus, V.fold, the accept test of the call in front)
void launch_select_warm(const DevView& V, hipStream_t s) {
    const int64_t count = 2 * V.m_max;
    if (!V.lat) {
        const int nb = (int)((count + 256 * VBA_SELW_ITEMS - 1) / (256 * VBA_SELW_ITEMS));
        hipLaunchKernelGGL((k_select_warm<VBA_SELW_ITEMS>), dim3(nb > 0 ? nb : 1, V.W), dim3(256), 0, s, V);
    } else {
        const int nb = (int)((count + 256 * kSelItems - 1) / (256 * kSelItems));
        hipLaunchKernelGGL((k_select_warm<kSelItems>), dim3(nb > 0 ? nb : 1, V.W), dim3(256), 0, s, V);
    }
}

// ---------------------------------------------------------------------------------------------- finish
// Many windows per launch: the select is finished ONCE per window by a launch of its own (one block per window, ~20 us for
// 4096 windows) instead of by every accumulation block in its prologue -- there the two dependent round trips and the
// barriers of the finish were a third of a block's life at two blocks per CU, with nothing to overlap them.
__global__ __launch_bounds__(256) void k_select_finish(DevView V) {
    __shared__ unsigned sel_lh[kSelBins];
    __shared__ unsigned sel_u[260];
    __shared__ unsigned long long sel_keys[1025];
    const int w = blockIdx.x;
    VBA_SKIP_CALL(V, w);
    const double c = select_finish(V, w, sel_lh, sel_u, sel_keys);
    if (threadIdx.x == 0) V.sc[w].c_obs = c;
    unsigned* h0 = hist0_of(V, w, V.par);       // (see k_obs_accumulate: clean for the call after next)
    for (int b = threadIdx.x; b < kSelBins; b += 256) h0[b] = 0u;
}

void launch_select_finish(const DevView& V, hipStream_t s) {
    hipLaunchKernelGGL(k_select_finish, dim3(V.W), dim3(256), 0, s, V);
}

}  // namespace vba
