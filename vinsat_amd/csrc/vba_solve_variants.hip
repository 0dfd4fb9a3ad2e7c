// vba_solve_variants.hip -- comparison builds only (make VARIANTS=1, -DVBA_VARIANTS): the solvers that were measured slower than
// what the default library launches and are kept as a record that can still be run (tests/test_gpu_variants.py):
//   k_solve_forming, k_solve_packed   sequential walks (one window per wave forming its blocks; three windows per wave)
//   k_cr_level0, k_cr_level012        one or three cyclic-reduction levels in front of the one-workgroup kernel instead of two
//   k_solve_resident                  the latency-mode solve as one grid of producer and waiting consumer blocks
// They are built from the production units' device bodies (vba_solve_step.h, vba_solve_chunk_body.h, vba_solve_cr_body.h); where
// a comparison path launches a production KERNEL it goes through that unit's launcher (vba_solve_units.h).
#ifndef VBA_VARIANTS
#error "vba_solve_variants.hip belongs to the comparison build (make VARIANTS=1)"
#endif
#include <atomic>

#include "vba_launch.h"
#include "vba_solve_chunk_body.h"
#include "vba_solve_cr_body.h"

namespace vba {

#ifdef VBA_RESIDENT_STAMPS
VBA_KSTAMP_FETCH(fetch_kstamps_variants)
#endif

// measured dead ends kept for comparison builds (make VARIANTS=1): k_solve_forming, k_solve_packed
// Batched windows, full phase (VBA_OPT_FUSION bit 2): the walk forms the blocks itself.  The assembly kernel wrote 2 kB
// per pose that this kernel read straight back -- 8 GB per call at 4096 windows of 500 poses; here the wave keeps the
// inputs of three consecutive poses (141 doubles each, BA_reg 183) in an LDS ring, loads the next pose's while it
// eliminates, and every lane forms the four entries of the next block it used to load.  Same band_entry / rhs_entry,
// so the same system to the bit; ~200 more instructions per block step in a kernel that is issue-bound at four waves
// per SIMD, against a whole launch and its traffic.
template <bool REG>
struct RawSource {
    static constexpr int kIn = kAsmBase + (REG ? kAsmPrior : 0);
    static constexpr int kPer = (kIn + 63) / 64;
    static constexpr bool kLateFetch = true;
    const DevView& V;
    size_t sb;
    int n, lane;
    double sigma, inv_wmax;
    double* ring;               // [3][kIn]: pose i lives in slot i % 3
    AsmLanes lanes;
    mutable double hold[kPer];
    __device__ void prefetch(int i) const {
        if (i >= n) return;
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const int q = lane + 64 * k;
            hold[k] = q < kIn ? asm_input<REG>(V, sb + i, q, true) : 0.0;
        }
    }
    __device__ void commit(int i) const {
        if (i >= n) return;
        double* slot = ring + (i % 3) * kIn;
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const int q = lane + 64 * k;
            if (q < kIn) slot[q] = hold[k];
        }
    }
    __device__ double operator()(int i, int e) const {
        const AsmRow R = asm_row<REG>(ring + (i % 3) * kIn, ring + ((i + 2) % 3) * kIn, i, n, true, sigma, inv_wmax);
        if (e >= 243) return rhs_entry(R, e - 243);
        return band_entry(R, e / 81, (e % 81) / 9, e % 9);
    }
    // all 252 entries of block i into out (LDS), seven uniform passes of the wave (vba_asm_fast.h)
    __device__ void form(int i, double* out) const {
        asm_form_row<REG>(lanes, ring + (i % 3) * kIn, ring + ((i + 2) % 3) * kIn, i < n - 1, i > 0, sigma, inv_wmax, lane,
                          [&](int e, double v) { out[e] = v; });
    }
};

template <bool PIVOT, bool REG>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_solve_forming(DevView V) {
    __shared__ double blk[2][256];
    __shared__ double ring[3 * RawSource<REG>::kIn];
    const int w = blockIdx.x;
    VBA_SKIP_CALL(V, w);
    WinScalars& sc = V.sc[w];
    if (sc.done || !solver_mine<PIVOT>(V, sc)) return;
    const int n = V.n[w];
    const int lane = threadIdx.x;
    const size_t sb = (size_t)w * V.n_max;
    const double lam32 = (double)(float)sc.lam[V.par];      // torch.eye() is float32 (BA_filtering.py:54)
    if (lane == 0) {
        sc.lam32 = lam32;
        if (PIVOT) atomicAnd(&sc.fl[V.par], ~8u);
    }
    bool badp = false;
    const RawSource<REG> src{V, sb, n, lane, V.prm.sigma, 1.0 / bits_f64(sc.wmax_bits[V.par]), ring, asm_lanes(lane), {}};
    src.prefetch(0); src.commit(0);
    src.prefetch(1); src.commit(1);
    for (int e = lane; e < 512; e += 64) (&blk[0][0])[e] = 0.0;     // (entries 252 .. 255 of a buffer are never formed)
    __syncthreads();
    chain_solve<PIVOT, true>(src, n, lam32, V.Xs + sb * 81, V.zs + sb * 9, V.dpose + sb * 9, blk, lane, badp);
    // the ring still holds poses n-3 .. n-1: the last diagonal block leaves for last_hessian (BA_filtering.py:97)
    for (int e = 81 + lane; e < 162; e += 64) V.lastD[(size_t)w * 81 + (e - 81)] = src(n - 1, e);
    report_pivot<PIVOT>(badp, sc, lane, V.par);
    const bool bad = retract_range(V, sb, n, lane, 64);
    const unsigned long long anybad = __ballot(bad);
    if (lane == 0 && anybad) atomicOr(&sc.fl[V.par], 2u);
}

// ---------------------------------------------------------------------------------------------- packed
// Many batched windows: three chains per wavefront (19 lanes each: 9 D' + 9 U + 1 right-hand side), so the ~550
// instructions of a block step serve three windows.  All windows of the handle must have the same pose count
// (checked by the host); windows that are already done ride along without storing.
constexpr int kPack = 3;

template <bool PIVOT>
__global__ __launch_bounds__(64) void k_solve_packed(DevView V) {
    __shared__ double blk[2][kPack][256];
    const int lane = threadIdx.x;
    const int g = lane / 19 < kPack ? lane / 19 : kPack - 1;
    const bool lane_ok = lane < 19 * kPack;
    const int ll = lane_ok ? lane - 19 * g : 19;          // 19 = no role
    const int gbase = 19 * g;
    const int w0 = blockIdx.x * kPack;
    const int wg = min(w0 + g, V.W - 1);
    const bool w_ok = w0 + g < V.W;
    const int n = V.n[w0];
    WinScalars& sc = V.sc[wg];
    const bool active = lane_ok && w_ok && !sc.done && VBA_WINDOW_RUNS(V, wg) && solver_mine<PIVOT>(V, sc);
    const size_t sb = (size_t)wg * V.n_max;
    const double lam32 = (double)(float)sc.lam[V.par];
    if (active && ll == 0) {
        sc.lam32 = lam32;
        if (PIVOT) atomicAnd(&sc.fl[V.par], ~8u);
    }
    double a[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) a[j] = 0.0;
    bool badp = false;
    double pre[kPack][4];
    auto fetch = [&](int i) {
#pragma unroll
        for (int q3 = 0; q3 < kPack; ++q3) {
            const size_t s3 = (size_t)min(w0 + q3, V.W - 1) * V.n_max + i;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = lane + 64 * q;
                pre[q3][q] = e < 243 ? V.bands[s3 * 243 + e] : (e < 252 ? V.rhs[s3 * 9 + (e - 243)] : 0.0);
            }
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int q3 = 0; q3 < kPack; ++q3)
#pragma unroll
            for (int q = 0; q < 4; ++q) blk[buf][q3][lane + 64 * q] = pre[q3][q];
    };
    auto load_base = [&](const double* b, int db, double (&base)[9]) {
        const int ub = 9 - db;
        const bool isD = ll >= db && ll < db + 9, isU = ll >= ub && ll < ub + 9, isY = ll == 18;
        const int cc = isD ? ll - db : (isU ? ll - ub : 0);
        const double* p = isD ? b + 81 + cc : (isU ? b + 162 + cc : b + 243);
        const int stride = isY ? 1 : 9;
#pragma unroll
        for (int r = 0; r < 9; ++r) {
            double v = (isD || isU || isY) ? p[r * stride] : 0.0;
            if (isD && r == cc) v += lam32;
            base[r] = v;
        }
    };
    fetch(0);
    stash(0);
    __syncthreads();
    for (int i = 0; i < n; ++i) {
        const int buf = i & 1;
        if (i + 1 < n) fetch(i + 1);
        double base[9];
        const double* mine = blk[buf][g];
        if (buf == 0) {
            load_base(mine, 0, base);
            forward_step<0, 1, PIVOT, true, true>(i > 0 ? mine : nullptr, base, a, ll, badp, gbase);
        } else {
            load_base(mine, 9, base);
            forward_step<9, 1, PIVOT, true, true>(mine, base, a, ll, badp, gbase);
        }
        const int ub = buf == 0 ? 9 : 0;
        if (active) {
            if (ll >= ub && ll < ub + 9) {
                double* X = V.Xs + (sb + i) * 81 + (ll - ub);
#pragma unroll
                for (int r = 0; r < 9; ++r) X[r * 9] = a[r];
            } else if (ll == 18) {
                double* z = V.zs + (sb + i) * 9;
#pragma unroll
                for (int r = 0; r < 9; ++r) z[r] = a[r];
            }
        }
        if (i + 1 < n) stash(buf ^ 1);
        __syncthreads();
    }
    __threadfence_block();
    __syncthreads();
    // backward sweep: lane ll < 9 of each group owns row ll
    const int r = ll < 9 ? ll : 0;
    double x = V.zs[(sb + n - 1) * 9 + r];
    if (active && ll < 9) V.dpose[(sb + n - 1) * 9 + r] = x;
    double Xrow[9], zr = 0.0;
    auto fetch_row = [&](int i) {
        const double* X = V.Xs + (sb + i) * 81 + r * 9;
#pragma unroll
        for (int j = 0; j < 9; ++j) Xrow[j] = X[j];
        zr = V.zs[(sb + i) * 9 + r];
    };
    if (n > 1) fetch_row(n - 2);
    for (int i = n - 2; i >= 0; --i) {
        double cur[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) cur[j] = Xrow[j];
        double v = zr;
        if (i > 0) fetch_row(i - 1);
#pragma unroll
        for (int j = 0; j < 9; ++j) v -= cur[j] * __shfl(x, gbase + j, kWave);
        x = v;
        if (active && ll < 9) V.dpose[(sb + i) * 9 + r] = x;
    }
    __threadfence_block();
    __syncthreads();
    // flags + retraction, one window after the other with the whole wave
    const unsigned long long badmask = __ballot(badp && active);
#pragma unroll
    for (int q3 = 0; q3 < kPack; ++q3) {
        const int w = w0 + q3;
        if (w >= V.W) break;
        WinScalars& s3 = V.sc[w];
        if (s3.done || !VBA_WINDOW_RUNS(V, w) || !solver_mine<PIVOT>(V, s3)) continue;
        const unsigned long long gm = ((1ull << 19) - 1ull) << (19 * q3);
        // (as report_pivot: 8 asks the host for the pivoted repeat, 16 hands the window to the pivoted kernels -- without it
        // solver_mine<true> turned the window away and the repeat never reported an outcome)
        if (lane == 0 && (badmask & gm)) atomicOr(&s3.fl[V.par], PIVOT ? 4u : (8u | 16u));
        const bool bad = retract_range(V, (size_t)w * V.n_max, n, lane, 64);
        const unsigned long long anybad = __ballot(bad);
        if (lane == 0 && anybad) atomicOr(&s3.fl[V.par], 2u);
    }
}


// ================================================================================================== cyclic reduction
// one cyclic-reduction level in front instead of two (VBA_OPT_FUSION bit 4): 0.9 us per call slower, comparison builds
// First level of the cyclic reduction as its own kernel, one wave (one CU) per pair of separators: wave t builds the
// blocks 2t, 2t+1, 2t+2, eliminates the two even ones (each even block is eliminated by both of its odd neighbours'
// waves: redundant work instead of communication), folds them into block 2t+1 and leaves
//   red[t] = the folded block 2t+1 (252 doubles) and  P[2t] = [PL | PU | Pg] of block 2t (for the back substitution)
// in global memory.  The 31 eliminations + folds of a 62-separator system then run on 31 CUs instead of sharing the
// four SIMDs of one.
// Two waves: the two eliminations are independent, so wave 1 builds and eliminates block 2t+2 beside wave 0's 2t.
template <bool PIVOT>
__global__ __launch_bounds__(128) void k_cr_level0(DevView V, int s) {
    __shared__ __attribute__((aligned(16))) double blk[3 * 252];
    const int w = blockIdx.y, t = blockIdx.x;
    VBA_SKIP_CALL(V, w);
    WinScalars& sc = V.sc[w];
    if (sc.done || !solver_mine<PIVOT>(V, sc)) return;
    const int n1 = n_separators(V.n[w], s);
    if (n1 < kCrSplitMin || n1 > 2 * kCrMax || 2 * t >= n1) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t rb = (size_t)w * V.p_max;
    const double lam32 = (double)(float)sc.lam[V.par];
    CrLanes g;
    if (wv == 0) cr_fill<2>(V, w, s, n1, lam32, 2 * t, 1, blk, 1, lane, [&]() { g = cr_lanes(lane); });
    else cr_fill<1>(V, w, s, n1, lam32, 2 * t + 2, 1, blk + 504, 1, lane, [&]() { g = cr_lanes(lane); });
    __syncthreads();
    bool bad = false;
    const bool has_j = 2 * t + 1 < n1, has_p = 2 * t + 2 < n1;
    if (wv == 0) cr_eliminate<PIVOT>(blk, g, lane, bad);
    else if (has_p) cr_eliminate<PIVOT>(blk + 504, g, lane, bad);
    __syncthreads();
    if (wv == 0) {
        double* P = V.csol2 + (rb + 2 * t) * 171;           // scratch of the two-level driver, unused in this mode
        for (int e = lane; e < 171; e += 64) P[e] = e < 81 ? blk[e] : blk[81 + e];       // PL | PU | Pg
        if (has_j) {
            cr_fold(blk + 252, blk, blk + 504, has_p, g);
            double* R = V.cL2 + rb * 171 + (size_t)t * 252;
            for (int e = lane; e < 252; e += 64) R[e] = blk[252 + e];
        }
    }
    report_pivot<PIVOT>(bad, sc, lane, V.par);
}

// three levels in front (VBA_CR_LEVELS=3): measured 0.45 us per call SLOWER than two, comparison builds
// The first THREE levels on their own CUs (round 4): eight waves per group of eight separators.  Group t builds the fifteen
// blocks 8t .. 8t+14, eliminates the even ones (eight waves side by side), folds them into the odd ones, eliminates 8t+1, 8t+5,
// 8t+9, 8t+13 and folds those into 8t+3, 8t+7, 8t+11, eliminates 8t+3 and 8t+11 and folds them into 8t+7.  It leaves
//   red3[t] = the three times folded block 8t+7 (252 doubles),  P[8t], P[8t+2], P[8t+4], P[8t+6] (level 0), P[8t+1], P[8t+5]
//   (level 1) and P[8t+3] (level 2) = [PL | PU | Pg]
// in global memory; what it shares with the next group (blocks 8t+8 .. 8t+14) is computed by both.  The one-workgroup kernel then
// starts from n / 8 blocks (7 instead of 15 at 62 separators): its fill shrinks and its first level of eight eliminations, two
// per SIMD, is gone.  Same eliminations and folds in another place: the bits of two levels in front.
template <bool PIVOT>
__device__ __forceinline__ void cr_level012_body(const DevView& V, int s, int w, int t, double* blk) {
    VBA_SKIP_CALL(V, w);
    WinScalars& sc = V.sc[w];
    if (sc.done || !solver_mine<PIVOT>(V, sc)) return;
    const int n1 = n_separators(V.n[w], s);
    if (n1 < kCrSplitMin || n1 > 8 * kCrMax || 8 * t >= n1) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;     // 8 waves
    const size_t rb = (size_t)w * V.p_max;
    const double lam32 = (double)(float)sc.lam[V.par];
    const int q0 = 8 * t;
    CrLanes g;
    cr_fill<2>(V, w, s, n1, lam32, q0 + wv, 8, blk + (size_t)wv * 252, 8, lane, [&]() { g = cr_lanes(lane); });     // blocks wv, wv + 8
    __syncthreads();
    bool bad = false;
    auto store_P = [&](int u) {         // [PL | PU | Pg] of block q0 + u
        double* P = V.csol2 + (rb + q0 + u) * 171;
        const double* B = blk + (size_t)u * 252;
        for (int e = lane; e < 171; e += 64) P[e] = e < 81 ? B[e] : B[81 + e];
    };
    auto fold = [&](int u, int h) {     // the eliminated blocks u - h and u + h into block u
        if (q0 + u < n1) cr_fold(blk + (size_t)u * 252, blk + (size_t)(u - h) * 252, blk + (size_t)(u + h) * 252, q0 + u + h < n1, g);
    };
    // level 0: the even blocks 0, 2, ..., 14
    if (q0 + 2 * wv < n1) cr_eliminate<PIVOT>(blk + (size_t)(2 * wv) * 252, g, lane, bad);
    __syncthreads();
    if (wv < 7) fold(2 * wv + 1, 1);
    else {
        for (int u = 0; u < 8; u += 2) if (q0 + u < n1) store_P(u);
    }
    __syncthreads();
    // level 1: blocks 1, 5, 9, 13
    if (wv < 4 && q0 + 4 * wv + 1 < n1) cr_eliminate<PIVOT>(blk + (size_t)(4 * wv + 1) * 252, g, lane, bad);
    __syncthreads();
    if (wv < 3) fold(4 * wv + 3, 2);
    else if (wv == 3) { if (q0 + 1 < n1) store_P(1); }
    else if (wv == 4) { if (q0 + 5 < n1) store_P(5); }
    __syncthreads();
    // level 2: blocks 3 and 11
    if (wv < 2 && q0 + 8 * wv + 3 < n1) cr_eliminate<PIVOT>(blk + (size_t)(8 * wv + 3) * 252, g, lane, bad);
    __syncthreads();
    if (wv == 0) {
        if (q0 + 7 < n1) {
            fold(7, 4);
            wave_sync_lds();
            double* R = V.cL2 + rb * 171 + (size_t)t * 252;
            for (int e = lane; e < 252; e += 64) R[e] = blk[7 * 252 + e];
        }
    } else if (wv == 1) {
        if (q0 + 3 < n1) store_P(3);
    }
    report_pivot<PIVOT>(bad, sc, lane, V.par);
}

template <bool PIVOT>
__global__ __launch_bounds__(512) void k_cr_level012(DevView V, int s) {
    __shared__ __attribute__((aligned(16))) double blk[16 * 252];
    cr_level012_body<PIVOT>(V, s, blockIdx.y, blockIdx.x, blk);
}

// the solve as ONE grid of producer and waiting consumer blocks (VBA_OPT_FUSION bits 5, 6): measured slower, comparison builds
// ------------------------------------------------------------------------------------------------ resident solve
// The three launches of the latency-mode solve (chunk elimination -> cyclic-reduction levels 0 + 1 -> the remaining levels
// in one workgroup) as ONE grid whose consumer blocks are resident from the start and wait for their producers on flags
// (VBA_OPT_FUSION bit 5).  Block x of window y is
//   x <  P          : chunk x                        (produces flag x)
//   x <  P + G      : cyclic-reduction group x - P   (waits for chunks 4t .. 4t + 7, produces flag x)
//   x == P + G      : the one-workgroup tail         (TAIL; waits for all groups)
// The grid (at C3: 63 + 16 + 1 blocks) is far below what the 256 CUs hold at once and blocks are dispatched in index order, so
// every producer is running or done when a consumer starts to wait.  A flag holds the EPOCH of the launch that wrote it
// (a counter the host increments per launch, so nothing is ever reset) and is stored by the last wave of the block to get
// there, EVERY wave passing through resident_publish whatever path it took through its role (windows that skip the call,
// short windows, a failed pivot check) -- a consumer can therefore never wait for a block that has nothing to say.  The
// wait is bounded all the same: kResidentSpins polls (> 100 ms) and the window is flagged (fl bit 64 -> VBA_ESTATE).
// Same bodies, same operations, same bits as the three launches.
constexpr int kResidentSpins = 1 << 18;      // polls; one is a round trip to memory, ~1 us

__device__ __forceinline__ void resident_publish(unsigned* flag, unsigned epoch, unsigned* lds_count, int nwaves) {
    __threadfence();            // this wave's stores are visible device-wide before it is counted
    if ((threadIdx.x & 63) == 0) {
        const unsigned before = atomicAdd(lds_count, 1u);
        // (relaxed: the fences above have released every wave's stores; a release store would write the L2 back once more)
        if (before == (unsigned)nwaves - 1u) __hip_atomic_store(flag, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// every wave waits by itself: lane l < count watches flags[first + l]; false when the bound was hit
__device__ __forceinline__ bool resident_wait(const unsigned* flags, int first, int count, unsigned epoch) {
    const int lane = threadIdx.x & 63;
    bool ok = true;
    for (int base = 0; base < count; base += 64) {
        const bool mine = base + lane < count;
        const unsigned* f = flags + first + (mine ? base + lane : 0);
        int spins = 0;
        for (;;) {
            const unsigned v = __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const bool there = !mine || (int)(v - epoch) >= 0;
            if (__all(there)) break;
            if (++spins > kResidentSpins) { ok = false; break; }
        }
        if (!ok) break;
    }
    __threadfence();            // acquire: nothing read below is older than the flags
    return ok;
}

template <bool PIVOT, bool REG, bool TAIL>
__global__ __launch_bounds__(TAIL ? 512 : 256) void k_solve_resident(DevView V, int s, int P, int G, unsigned epoch) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    __shared__ unsigned arrived;
    constexpr int kThreads = TAIL ? 512 : 256;
    const int w = blockIdx.y, x = blockIdx.x, tid = threadIdx.x;
    unsigned* flags = V.res_flags + (size_t)w * V.res_stride;
    if (tid == 0) arrived = 0u;
#ifdef VBA_RESIDENT_STAMPS
    // diagnostic build: 100 MHz wall clock at entry / after the wait / after the body / after the publish, wave 0 of every block
    unsigned long long* stamp = reinterpret_cast<unsigned long long*>(V.cR2) + ((size_t)w * V.res_stride + x) * 4;
#define VBA_RSTAMP(k) do { if (tid == 0) stamp[k] = wall_clock64(); } while (0)
#else
#define VBA_RSTAMP(k) do {} while (0)
#endif
    VBA_RSTAMP(0);
    __syncthreads();
    if (x < P) {
        VBA_RSTAMP(1);
        if (tid < 256) chunks_ts_fused_body<PIVOT, REG>(V, s, w, x, smem);
    } else if (x < P + G) {
        const int t = x - P;
        if (tid < 256) {
            const int first = 4 * t, last = 4 * t + 7 < P - 1 ? 4 * t + 7 : P - 1;
            if (!resident_wait(flags, first, last - first + 1, epoch) && (tid & 63) == 0) atomicOr(&V.sc[w].fl[V.par], 2u | 64u);
            VBA_RSTAMP(1);
            cr_level01_body<PIVOT>(V, s, w, t, smem);
        }
    } else if (TAIL) {
        if (!resident_wait(flags, P, G, epoch) && (tid & 63) == 0) atomicOr(&V.sc[w].fl[V.par], 2u | 64u);
        VBA_RSTAMP(1);
        reduced_cr_body<PIVOT, 2, kThreads>(V, s, w, smem);
    }
    VBA_RSTAMP(2);
    resident_publish(flags + x, epoch, &arrived, kThreads / 64);
    VBA_RSTAMP(3);
#undef VBA_RSTAMP
}

static std::atomic<unsigned> g_resident_epoch{0u};    // flags of k_solve_resident: one value per launch, process wide

// ================================================================================================== dispatch
template <bool PIVOT>
static bool launch_comparison_t(const DevView& V, hipStream_t s) {
    if (V.chunk <= 0) {
        if (V.pack == 2) return false;      // four windows per wavefront: the production walk
        if (V.pack) {       // equal pose counts: three windows per wavefront
            hipLaunchKernelGGL(k_solve_packed<PIVOT>, dim3((V.W + kPack - 1) / kPack), dim3(64), 0, s, V);
            return true;
        }
        if (!walk_forms_blocks(V)) return false;
        // (V.pack == 0: one window per wavefront)
        if (V.reg) hipLaunchKernelGGL((k_solve_forming<PIVOT, true>), dim3(V.W), dim3(64), 0, s, V);
        else hipLaunchKernelGGL((k_solve_forming<PIVOT, false>), dim3(V.W), dim3(64), 0, s, V);
        return true;
    }
    const int cs = V.chunk, cs2 = V.chunk2;
    const int P = (V.n_max + cs - 1) / cs;
    const int n0_all = P - 1;
    const bool resident = V.resident && solve_forms_blocks(V) && V.chunk_waves == 2 && cs >= 4 && cs2 < 0 && V.cr_levels == 2 &&
                          n0_all >= kCrSplitMin && n0_all <= 4 * kCrMax;
    if (resident) {
        // one grid: chunks, cyclic-reduction groups and (V.resident == 2) the one-workgroup tail, see k_solve_resident
        const bool reg = V.reg != 0, tail = V.resident == 2;
        const int G = (n0_all + 3) / 4;
        size_t lds_all = (size_t)twosided_fused_lds_doubles(cs, reg) * sizeof(double);
        if (lds_all < 7 * 252 * sizeof(double)) lds_all = 7 * 252 * sizeof(double);
        if (tail && lds_all < cr_tail2_lds_bytes(n0_all)) lds_all = cr_tail2_lds_bytes(n0_all);
        const unsigned epoch = ++g_resident_epoch;
        const dim3 grid(P + G + (tail ? 1 : 0), V.W);
        if (tail) {
            if (reg) hipLaunchKernelGGL((k_solve_resident<PIVOT, true, true>), grid, dim3(512), lds_all, s, V, cs, P, G, epoch);
            else hipLaunchKernelGGL((k_solve_resident<PIVOT, false, true>), grid, dim3(512), lds_all, s, V, cs, P, G, epoch);
        } else {
            if (reg) hipLaunchKernelGGL((k_solve_resident<PIVOT, true, false>), grid, dim3(256), lds_all, s, V, cs, P, G, epoch);
            else hipLaunchKernelGGL((k_solve_resident<PIVOT, false, false>), grid, dim3(256), lds_all, s, V, cs, P, G, epoch);
            launch_cr_tail2(V, PIVOT, s);
        }
        launch_cr_short(V, PIVOT, s);       // short windows of the handle: the one-workgroup variant as before
        return true;
    }
    if (cs2 < 0 && V.cr_levels != 2) {      // another number of cyclic-reduction levels in front of the one-workgroup kernel
        launch_solve_chunks(V, PIVOT, solve_forms_blocks(V), s);
        const int n0_max = n0_all;
        if (n0_max >= kCrSplitMin) {
            if (V.cr_levels == 3) {
                hipLaunchKernelGGL(k_cr_level012<PIVOT>, dim3((n0_max + 7) / 8, V.W), dim3(512), 0, s, V, cs);
                hipLaunchKernelGGL((k_solve_reduced_cr<PIVOT, 3>), dim3(V.W), dim3(kCrThreads),
                                   ((size_t)(n0_max / 8) * 252 + (size_t)((n0_max + 7) / 8) * 9 + (size_t)((n0_max + 3) / 4) * 9) * sizeof(double), s, V, cs);
            } else {
                hipLaunchKernelGGL(k_cr_level0<PIVOT>, dim3((n0_max + 1) / 2, V.W), dim3(128), 0, s, V, cs);
                hipLaunchKernelGGL((k_solve_reduced_cr<PIVOT, 1>), dim3(V.W), dim3(kCrThreads), (size_t)(n0_max / 2) * 252 * sizeof(double), s, V, cs);
            }
        }
        launch_cr_short(V, PIVOT, s);
        return true;
    }
    return false;
}
bool launch_solve_comparison(const DevView& V, bool pivot, hipStream_t s) {
    return pivot ? launch_comparison_t<true>(V, s) : launch_comparison_t<false>(V, s);
}

hipError_t configure_variants_device() {
    const int cap_ts = twosided_fused_lds_doubles(kFusedChunkMax, true) * 8;
    const int cap_res = cap_ts > kCrTail2LdsCap ? cap_ts : kCrTail2LdsCap;
    const LdsLimit set[] = {
        {reinterpret_cast<const void*>(k_solve_reduced_cr<false, 3>), kCrLdsCap + 200 * 9 * 8}, {reinterpret_cast<const void*>(k_solve_reduced_cr<true, 3>), kCrLdsCap + 200 * 9 * 8},
        {reinterpret_cast<const void*>(k_solve_reduced_cr<false, 1>), kCrLdsCap}, {reinterpret_cast<const void*>(k_solve_reduced_cr<true, 1>), kCrLdsCap},
        {reinterpret_cast<const void*>(k_solve_resident<false, false, false>), cap_res}, {reinterpret_cast<const void*>(k_solve_resident<true, false, false>), cap_res},
        {reinterpret_cast<const void*>(k_solve_resident<false, true, false>), cap_res}, {reinterpret_cast<const void*>(k_solve_resident<true, true, false>), cap_res},
        {reinterpret_cast<const void*>(k_solve_resident<false, false, true>), cap_res}, {reinterpret_cast<const void*>(k_solve_resident<true, false, true>), cap_res},
        {reinterpret_cast<const void*>(k_solve_resident<false, true, true>), cap_res}, {reinterpret_cast<const void*>(k_solve_resident<true, true, true>), cap_res}};
    return set_lds_limits(set);
}

}  // namespace vba
