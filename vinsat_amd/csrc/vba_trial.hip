// vba_trial.hip -- A8 of the BA iteration (gfx950).
//
//   k_trial            step + retraction (latency mode), weighted trial residuals and dynamics residuals at the trial
//                      states, next call's keys: histogram + bin buckets
//
// The observation blocks stream the observation arrays once, coalesced (SoA, 8 B per lane per array); the pose state is
// gathered through L1/L2 (observations are pose sorted, so a wave touches one or two poses).
// Not a unit of the Makefile: vba_accumulate.hip includes this file at its end (the reason is given there).
#include "vba_device.h"
#include "vba_launch.h"
#include "vba_step.h"

namespace vba {

// Diagnostic builds (-DVBA_RESIDENT_STAMPS; tools/attic/trial_stamps.py): 100 MHz wall-clock stamps of thread 0 of observation
// block 100 along k_trial, fetched with vba_debug_fetch(h, 0, 102, ...): 64 words, 0 .. 15 from here, 16 .. 63 the stamps
// along k_obs_accumulate (vba_accumulate.hip).
#ifdef VBA_RESIDENT_STAMPS
__device__ unsigned long long g_ostamps[16];
#define VBA_OSTAMP(slot) do { if (threadIdx.x == 0 && blockIdx.x == 100 && blockIdx.y == 0) g_ostamps[slot] = wall_clock64(); } while (0)
void fetch_ostamps(unsigned long long* out) {
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ostamps), sizeof(g_ostamps));
    fetch_astamps(out + 16);
}
#else
#define VBA_OSTAMP(slot) do {} while (0)
#endif

// ---------------------------------------------------------------------------------------------- A8: trial residuals
// blocks [0, nblk_obs): sum |w (uv - est')| over the observations (BA_filtering.py:61, 66);
// blocks [nblk_obs, nblk_obs + nblk_dyn): sqrt(sigma) sum |r_pred'| over the pose edges (BA_filtering.py:65, 67).
// EMIT: the observation blocks also write the |r| keys, their histogram (digit-0 slot of the NEXT call's parity) and the
// block sums of |r| at the trial states -- the input of the next call if this trial is accepted (k_decide clears the
// histogram again if it is not).  EMIT 2: warm histogram (bins around this call's median: the next call selects in one
// pass); EMIT 1: the 10 exponent bits = digit 0 of the exact select (many windows per launch: the ~1 global atomic per
// key that a 2048-bin histogram costs is dearer there than the second pass over the keys it saves).
// FUSED (latency mode, VBA_OPT_FUSION bit 0): 0 = the trial states are in memory, pose-chain blocks of 256 edges;
// 1 / 2 = the trial states do not exist yet and are formed here (vba_step.h: 1 landmark-only 6x6 solve, 2 recovery of the
// partitioned solve), 16 lanes per pose: an observation block for the poses its rows belong to (a handful), a pose-chain
// block for 16 poses = 15 edges, which also writes states_new / dpose for everybody after this kernel; 3 = the geometry
// of 1 / 2 with the trial states read from memory (a call of such a handle that cannot fuse: pivoted landmark-only solve).
constexpr int kEdgesPerBlock16 = 15;

// PART (many windows per launch, FUSED 0): 0 = one grid does both kinds of block; 1 = the observation blocks only, 2 = the
// pose-chain blocks only, as two launches -- the orbit propagation of the chain blocks costs the streaming blocks half
// their occupancy when both are one kernel (96 registers against 40).
// TILES (plain geometry, one grid, latency mode): an observation block takes TILES consecutive tiles of 256 rows.  The
// block's keys share ONE pass of bin reservations -- a window of 10^6 keys is ~2000 tiles, every one of which hits the few
// hundred central bins with a returning atomic of its own, and the same-address atomics queue up (block 100 of C5 waited
// 6 .. 8 of its 15 us for its bases, C3: 0.4 .. 1.8) -- and the grid fits the chip in one round.  Block sums stay per TILE
// (the slots and the bits of TILES = 1), the histogram is integers, a bucket is a set: the results do not depend on TILES.
template <int EMIT, int FUSED, int PART = 0, int TILES = 1>
__global__ __launch_bounds__(kObsBlock) void k_trial(DevView V) {
    static_assert(PART == 0 || FUSED == 0, "split launches exist for the plain geometry only");
    static_assert(TILES == 1 || (PART == 0 && FUSED == 0), "tiled observation blocks exist for the plain one-grid geometry only");
    constexpr bool FORM = FUSED == 1 || FUSED == 2;
    __shared__ double red[kObsBlock / 64];
    __shared__ double redt[TILES > 1 ? 2 * TILES * (kObsBlock / 64) : 1];
    __shared__ unsigned lh[EMIT == 2 ? kSelBins : (EMIT == 1 ? 1024 : 1)];
    __shared__ double snew[FORM ? (kObsBlock + 1) * 10 : 1];
    __shared__ int lpose[FORM ? kObsBlock : 1];
    __shared__ unsigned wlead[FORM ? 4 : 1];
    const int w = blockIdx.y;
    // The pose of this thread's row (and of the row in front of it), requested FIRST of all: the address needs the block and
    // thread index only (clamped into the window's rows), and everything an observation block does hangs on it -- this way
    // the round trip runs beside the one of the call counter instead of behind it.
    int early_pose = 0, early_prev = 0;
    constexpr bool kEarlyPose = FUSED == 1 || FUSED == 2;      // (the streaming blocks of the batched mode keep their load where it was)
    if (kEarlyPose && PART != 2) {
        const int64_t ke = min((int64_t)blockIdx.x * kObsBlock + threadIdx.x, V.m_max - 1);
        const int* op = V.opose + 2 * (size_t)w * V.obs_stride;
        early_pose = op[ke];
        early_prev = op[ke > 0 ? ke - 1 : 0];
    }
    VBA_SKIP_CALL(V, w);
    WinScalars& sc = V.sc[w];
    if (sc.done) return;
    VBA_OSTAMP(0);
    const int n = V.n[w], m = V.m[w];
    const StepParams& prm = V.prm;
    const int par = V.par;
    const int tid = threadIdx.x;
    double s = 0.0, s_raw = 0.0;
    const size_t sb = (size_t)w * V.n_max;
    const int nfat = (V.nblk_obs + TILES - 1) / TILES;     // observation blocks of this grid
    const bool obs_block = PART == 1 || (PART == 0 && (int)blockIdx.x < nfat);
    // this block's place in part_trial (an observation block of several tiles: its first tile's)
    const int part_slot = PART == 2 ? V.nblk_obs + (int)blockIdx.x : (obs_block ? (int)blockIdx.x * TILES : V.nblk_obs + ((int)blockIdx.x - nfat));
    const double lam32 = (double)(float)sc.lam[par];      // torch.eye() is float32 (BA_filtering.py:54)
    // a window that has fallen back to the pivoted kernels (landmark-only phase) reads the trial states they wrote
    const bool fz = FUSED == 2 || (FUSED == 1 && !(sc.fl[par] & 16u));
    const double wmax = bits_f64(sc.wmax_bits[par]);
    const double inv_wmax = 1.0 / wmax;
    const int l16 = tid & 15, grp = tid >> 4, gbase = (tid & 63) & ~15;
    unsigned long long wlo = 0ull;
    constexpr int kEmitBins = EMIT == 2 ? kSelBins : 1024;     // warm bins, or the 10 exponent bits (digit 0 of the exact select)
    if (EMIT == 2) wlo = warm_range_start(f64_bits(sc.c_obs), V.warm_shift);
    if (EMIT && PART != 2 && obs_block) {
        for (int b = tid; b < kEmitBins; b += kObsBlock) lh[b] = 0u;
        __syncthreads();
    }
    if (PART != 2 && blockIdx.x == 0) {
        // digits 1, 2 of an exact select are dead since the accumulation; the list of the next warm select starts empty
        unsigned* h12 = histd_of(V, w, 1);
        for (int b = tid; b < 2 * kSelBins; b += kObsBlock) h12[b] = 0u;
        if (V.wbucket) {    // inline select: nobody clears these in front of the next accumulation
            unsigned* h0 = hist0_of(V, w, par);     // this call's histogram: its last readers were the accumulation's prologues
            for (int b = tid; b < kSelBins; b += kObsBlock) h0[b] = 0u;
            if (tid == 0) sc.wmax_bits[par ^ 1] = 0ull;
        }
        if (tid == 0) {
            sc.sel_cnt = 0u;
            sc.pending = V.call;
            if (EMIT == 2) sc.warm_lo[par ^ 1] = wlo;
            if (EMIT == 1) {        // digit 0 of the next call's exact select is the histogram this kernel leaves
                sc.sel_prefix[0] = 0ull;
                sc.sel_rank[0] = (2 * (long long)m - 1) / 2;
            }
            if (FUSED == 1 && fz) sc.lam32 = lam32;
        }
    }
    VBA_OSTAMP(1);
    unsigned bad = 0u;
    unsigned kbin[2 * TILES] = {}, kslot[2 * TILES] = {};      // EMIT 2: warm bin of this thread's keys and their place in the block's share
    double kkey[2 * TILES] = {};
    bool kvalid[TILES] = {};
    double s_tile[TILES] = {}, sraw_tile[TILES] = {};          // (TILES > 1: the sums of the tiles, reduced together below)
    if (PART != 2 && obs_block) {
    // (the loop over this block's tiles; its body keeps the indentation of the one tile it was)
#pragma unroll
    for (int tl = 0; tl < TILES; ++tl) {
        const int k = (blockIdx.x * TILES + tl) * kObsBlock + tid;
        const size_t ob = (size_t)w * V.obs_stride, mb = (size_t)w * V.m_max;
        const bool have = k < m;
        const int pose = have ? (kEarlyPose ? early_pose : V.opose[2 * ob + k]) : -1;
        const double* stp = V.states_new + (sb + (have ? pose : 0)) * 10;
        if (FORM && fz) {
            // the poses of this block's rows (rows are pose sorted): the first row of every pose inside the block leads,
            // leaders are numbered in row order and 16 lanes form the trial state of each
            const int prev = (have && tid > 0) ? early_prev : -2;
            const bool lead = have && (tid == 0 || prev != pose);
            const unsigned long long lm = __ballot(lead);
            const int lane = tid & 63, wv = tid >> 6;
            if (lane == 0) wlead[wv] = (unsigned)__popcll(lm);
            __syncthreads();
            unsigned before = 0, nlead = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                before += q < wv ? wlead[q] : 0u;
                nlead += wlead[q];
            }
            const int slot = (int)(before + (unsigned)__popcll(lm & ((2ull << lane) - 1ull))) - 1;   // leaders up to and including me
            if (lead) lpose[slot] = pose;
            __syncthreads();
            VBA_OSTAMP(2);
            for (unsigned base = 0; base < nlead; base += 16) {
                const unsigned idx = base + (unsigned)grp;
                const bool live = idx < nlead;
                double o[10], d9[9];
                unsigned b2 = 0u;
                pose_trial_state_group<FORM ? FUSED : 1>(V, w, live ? lpose[idx] : 0, live, l16, gbase, inv_wmax, lam32, o, d9, b2);
                if (live && l16 == 0) {
#pragma unroll
                    for (int r = 0; r < 10; ++r) snew[(size_t)idx * 10 + r] = o[r];
                }
            }
            __syncthreads();
            VBA_OSTAMP(3);
            stp = snew + (size_t)(slot < 0 ? 0 : slot) * 10;
        }
        if (have) {
            PoseCam pc;
            pose_camera(stp, V.intr + (sb + pose) * 4, pc);
            double u, v, cam[3], d;
            project(pc, V.ox[ob + k], V.oy[ob + k], V.oz[ob + k], u, v, cam, d);
            const double wk = (V.wraw[mb + k] / wmax) * V.oconf[ob + k];
            const double du = V.ou[ob + k] - u, dv = V.ov[ob + k] - v;
            s = fabs(du * wk) + fabs(dv * wk);
            s_tile[tl] = s;
            if (EMIT) {
                const double ru = fabs(du), rv = fabs(dv);
                reinterpret_cast<double2*>(V.absr + 2 * mb)[k] = make_double2(ru, rv);
                s_raw = ru + rv;
                sraw_tile[tl] = s_raw;
                if (EMIT == 2) {
                    kbin[2 * tl] = warm_bin(f64_bits(ru), wlo, V.warm_shift);
                    kbin[2 * tl + 1] = warm_bin(f64_bits(rv), wlo, V.warm_shift);
                    if (V.wbucket) {        // the place inside the block's share of the bin: a returning atomic
                        kslot[2 * tl] = atomicAdd(&lh[kbin[2 * tl]], 1u);
                        kslot[2 * tl + 1] = atomicAdd(&lh[kbin[2 * tl + 1]], 1u);
                        kkey[2 * tl] = ru;
                        kkey[2 * tl + 1] = rv;
                        kvalid[tl] = true;
                    } else {
                        atomicAdd(&lh[kbin[2 * tl]], 1u);
                        atomicAdd(&lh[kbin[2 * tl + 1]], 1u);
                    }
                } else {
                    atomicAdd(&lh[(unsigned)(f64_bits(ru) >> 53) & 1023u], 1u);
                    atomicAdd(&lh[(unsigned)(f64_bits(rv) >> 53) & 1023u], 1u);
                }
            }
        }
    }   // tiles
    } else if (PART != 1) {
        const int db = part_slot - V.nblk_obs;
        const bool reg = V.reg && !prm.initialize;
        // which pose / edge this thread evaluates, and where its two states are
        int i;                      // pose; edge i -> i + 1
        bool edge_thread;           // this thread evaluates the edge i -> i + 1
        bool pose_thread;           // this thread accounts for pose i (prior residual; FORM: writes its trial state)
        const double* st;
        const double* sn;
        if (FUSED == 0) {
            i = db * kObsBlock + tid;
            edge_thread = pose_thread = true;
            st = V.states_new + (sb + i) * 10;
            sn = st + 10;
        } else {
            const int i0 = db * kEdgesPerBlock16;
            const int j = i0 + grp;                     // the pose of this 16-lane group
            i = j;
            edge_thread = l16 == 0 && grp < kEdgesPerBlock16;
            // the block's 16th pose is the next block's first -- unless there is no next block
            pose_thread = l16 == 0 && (grp < kEdgesPerBlock16 || j / kEdgesPerBlock16 >= V.nblk_dyn);
            if (FORM && fz) {
                const bool live = j < n;
                double o[10], d9[9];
                unsigned b2 = 0u;
                pose_trial_state_group<FORM ? FUSED : 1>(V, w, j, live, l16, gbase, inv_wmax, lam32, o, d9, b2);
                bad = b2;
                if (live && l16 == 0) {
#pragma unroll
                    for (int r = 0; r < 10; ++r) snew[(size_t)grp * 10 + r] = o[r];
                    if (pose_thread) {
#pragma unroll
                        for (int r = 0; r < 10; ++r) V.states_new[(sb + j) * 10 + r] = o[r];
#pragma unroll
                        for (int r = 0; r < 9; ++r) V.dpose[(sb + j) * 9 + r] = d9[r];
                        if (V.host_states) {        // (one-window handles: sb == 0)
#pragma unroll
                            for (int r = 0; r < 10; ++r) V.host_states[((size_t)par * V.n_max + j) * 10 + r] = o[r];
                        }
                    }
                }
                if (FUSED == 1 && live && j == n - 1) {     // last_hessian of a landmark-only call: H / w_max on the 6x6, zeros elsewhere
                    const double* H = V.Hraw + (sb + j) * 21;
                    for (int e = l16; e < 81; e += 16) {
                        const int a = e / 9, c = e % 9;
                        V.lastD[(size_t)w * 81 + e] = (a < 6 && c < 6) ? H[sym6(a, c)] * inv_wmax : 0.0;
                    }
                }
                __syncthreads();
                st = snew + (size_t)grp * 10;
                sn = st + 10;
            } else {
                st = V.states_new + (sb + j) * 10;
                sn = st + 10;
            }
        }
        if (edge_thread && !prm.initialize && i < n - 1) {
            double x[6] = {st[0], st[1], st[2], st[7], st[8], st[9]};
            const int steps = V.steps[sb + i];
            if (steps > 0 || V.hop) {       // (a long edge's orbit residual is k_long_trial's, in a slot of its own)
                propagate_gap<false>(x, nullptr, abs(steps), V.hop);
                s = fabs(x[0] - sn[0]) + fabs(x[1] - sn[1]) + fabs(x[2] - sn[2]) +
                    fabs((x[3] - sn[7]) * kVelCoeff) + fabs((x[4] - sn[8]) * kVelCoeff) + fabs((x[5] - sn[9]) * kVelCoeff);
            }
            double att = fabs(attitude_residual(st + 3, V.cumrot + (sb + i) * 4, sn + 3));
            // BA_reg evaluates the trial's dynamics residual with quat_coeff_prior = 1 where BA passes quat_coeff = 100
            // (BA_filtering.py:172, 174 vs :63, 65): reproduced as written
            if (reg) att *= 1.0 / kQuatCoeff;
            s += att;
            s *= prm.sqrt_sigma;
        }
        if (reg && pose_thread && i < n) {     // sum |r_prior| at the trial states (BA_filtering.py:175, 178), not scaled by sigma
            double r6[6];
            prior_residual(V.prior_H + (sb + i) * 36, V.prior_x + (sb + i) * 6, st, r6);
            s += fabs(r6[0]) + fabs(r6[1]) + fabs(r6[2]) + fabs(r6[3]) + fabs(r6[4]) + fabs(r6[5]);
        }
    }
    // bin buckets: the block reserves its share of every bin it touched with one returning atomic per bin -- requested
    // here, in flight while the block sums below are formed
    VBA_OSTAMP(4);
    constexpr int kBinsPerThread = kSelBins / kObsBlock;
    static_assert(kSelBins % kObsBlock == 0, "bins per thread");
    unsigned bb[kBinsPerThread] = {};
    const bool bucketing = EMIT == 2 && PART == 0 && obs_block && V.wbucket;
    if (bucketing) {
        __syncthreads();        // the block's counts are complete
        unsigned* hist = hist0_of(V, w, par ^ 1);
#pragma unroll
        for (int q = 0; q < kBinsPerThread; ++q) {
            const unsigned c = lh[tid + q * kObsBlock];
            bb[q] = c ? atomicAdd(&hist[tid + q * kObsBlock], c) : 0u;
        }
    }
    VBA_OSTAMP(5);
    if (TILES > 1 && obs_block) {
        // the 2 TILES sums of the tiles in ONE round of barriers; per sum the order of block_sum (waves 0 .. 3 onto 0.0)
#pragma unroll
        for (int tl = 0; tl < TILES; ++tl) {
            const double a = wave_sum(s_tile[tl]), r2 = wave_sum(sraw_tile[tl]);
            if ((tid & 63) == 0) {
                redt[(2 * tl) * (kObsBlock / 64) + (tid >> 6)] = a;
                redt[(2 * tl + 1) * (kObsBlock / 64) + (tid >> 6)] = r2;
            }
        }
        __syncthreads();
        if (tid < 2 * TILES && part_slot + tid / 2 < V.nblk_obs) {
            double t = 0.0;
#pragma unroll
            for (int i = 0; i < kObsBlock / 64; ++i) t += redt[tid * (kObsBlock / 64) + i];
            if (tid & 1) { if (EMIT) V.part_next[(size_t)w * V.nblk_obs + part_slot + tid / 2] = t; }
            else V.part_trial[(size_t)w * V.trial_stride + part_slot + tid / 2] = t;
        }
    } else {
        const double t = block_sum<kObsBlock>(s, red);
        if (tid == 0) V.part_trial[(size_t)w * V.trial_stride + part_slot] = t;
    }
    VBA_OSTAMP(6);
    if (FORM && !obs_block) {
        const unsigned long long bp = __ballot(bad & 1u), bn = __ballot(bad & 2u);
        if ((tid & 63) == 0 && (bp || bn)) atomicOr(&sc.fl[par], (bp ? (8u | 16u) : 0u) | (bn ? 2u : 0u));
    }
    if (EMIT && PART != 2 && obs_block) {
        if (TILES == 1) {
            const double t_raw = block_sum<kObsBlock>(s_raw, red);
            if (tid == 0) V.part_next[(size_t)w * V.nblk_obs + part_slot] = t_raw;
        }
        unsigned* hist = hist0_of(V, w, par ^ 1);
        if (bucketing) {
            // ... and each key goes to its place: the next call finds the keys of the wanted bin together, no pass over all keys
            // (k_select_warm) is needed
#pragma unroll
            for (int q = 0; q < kBinsPerThread; ++q) lh[tid + q * kObsBlock] = bb[q];
            __syncthreads();
            VBA_OSTAMP(7);
            double* pool = V.wbucket + ((size_t)w * 2 + (par ^ 1)) * kSelBins * (size_t)V.bucket_cap;
#pragma unroll
            for (int q = 0; q < 2 * TILES; ++q) {
                if (kvalid[q / 2]) {
                    const unsigned slot = lh[kbin[q]] + kslot[q];
                    if (kbin[q] >= 1u && kbin[q] <= 2046u && slot < (unsigned)V.bucket_cap) pool[(size_t)kbin[q] * V.bucket_cap + slot] = kkey[q];
                }
            }
            VBA_OSTAMP(8);
        } else {
            for (int b = tid; b < kEmitBins; b += kObsBlock) {
                const unsigned c = lh[b];
                if (c) atomicAdd(&hist[b], c);
            }
        }
    }
}

template <int EMIT>
static void launch_trial_emit(const DevView& V, hipStream_t s) {
    const dim3 g(V.nblk_obs + V.nblk_dyn, V.W), b(kObsBlock);
    const int f = V.fused_trial;        // 0..3, see k_trial; V.nblk_dyn is the pose-chain block count of that geometry
    if (f == 0 && !V.lat && !V.wbucket) {        // many windows: the two kinds of block as two launches
        hipLaunchKernelGGL((k_trial<EMIT, 0, 2>), dim3(V.nblk_dyn, V.W), b, 0, s, V);
        hipLaunchKernelGGL((k_trial<EMIT, 0, 1>), dim3(V.nblk_obs, V.W), b, 0, s, V);
        return;
    }
    if (f == 1) hipLaunchKernelGGL((k_trial<EMIT, 1>), g, b, 0, s, V);
    else if (f == 2) hipLaunchKernelGGL((k_trial<EMIT, 2>), g, b, 0, s, V);
    else if (f == 3) hipLaunchKernelGGL((k_trial<EMIT, 3>), g, b, 0, s, V);
    else if (EMIT == 2 && V.trial_tiles == 8) hipLaunchKernelGGL((k_trial<EMIT, 0, 0, EMIT == 2 ? 8 : 1>), dim3((V.nblk_obs + 7) / 8 + V.nblk_dyn, V.W), b, 0, s, V);
    else if (EMIT == 2 && V.trial_tiles == 4) hipLaunchKernelGGL((k_trial<EMIT, 0, 0, EMIT == 2 ? 4 : 1>), dim3((V.nblk_obs + 3) / 4 + V.nblk_dyn, V.W), b, 0, s, V);
    else if (EMIT == 2 && V.trial_tiles == 2) hipLaunchKernelGGL((k_trial<EMIT, 0, 0, EMIT == 2 ? 2 : 1>), dim3((V.nblk_obs + 1) / 2 + V.nblk_dyn, V.W), b, 0, s, V);
    else hipLaunchKernelGGL((k_trial<EMIT, 0>), g, b, 0, s, V);
}

void launch_trial(const DevView& V, hipStream_t s) {
    if (V.emit == 2) launch_trial_emit<2>(V, s);
    else if (V.emit == 1) launch_trial_emit<1>(V, s);
    else launch_trial_emit<0>(V, s);
    launch_long_trial(V, s);        // the orbit residual of the long edges at the trial states (vba_long.hip)
}

}  // namespace vba
