// vba_solve_step.h -- what every unit of the block-tridiagonal solve (A7) shares: the wave-level pivot step, the walk of
// one chain built on it, the per-window choice of the pivoted / unpivoted kernels and the retraction (A8).
//
// The reference forms the (9n)^2 matrix densely and calls LU (BA_filtering.py:54-55).  The matrix is exactly
// block tridiagonal in 9x9 blocks and not symmetric, so the solve here is a block elimination along the
// pose chain with partial pivoting inside each 9x9 diagonal block:
//
//   forward :  D'_i = D_i + fp32(lamda) I - L_i X_{i-1},  y_i = g_i - L_i z_{i-1},
//              [X_i | z_i] = D'_i^{-1} [U_i | y_i]           (Gauss-Jordan, row pivoting)
//   backward:  x_{n-1} = z_{n-1},  x_i = z_i - X_i x_{i+1}
//
// A wavefront walks a chain.  Lane c owns COLUMN c of the working matrix [D' | U | right-hand sides] in 9
// registers, so the pivot search is lane-local and a pivot step is 8 broadcasts (v_readlane) plus 8 FMAs
// per lane; extra right-hand-side columns ride along in otherwise idle lanes.  The lanes that end a step
// holding X_i are the ones that need it as the D' columns of step i+1, so the two column groups swap roles
// every step and nothing is shuffled.
//
// Two drivers share that step:
//   * k_solve          one wave per window walks all n blocks (work-optimal; used when many windows are
//                      batched, the windows supply the parallelism) -- vba_solve_seq.hip;
//   * k_solve_chunks / k_solve_reduced / k_solve_recover   (vba_solve_chunks.hip, vba_solve_cr.hip)
//                      the chain is cut into P chunks separated by single "separator" blocks.  Every chunk is
//                      eliminated by its own wave with 19 right-hand sides (g and the couplings to its two
//                      separators), a reduced block-tridiagonal system over the P-1 separators is solved by one
//                      wave, and the interiors are recovered in parallel: ~ n/P + P sequential block steps
//                      instead of n.  Default of the latency mode: k_solve_chunks_ts (two waves per chunk, meeting in the
//                      middle), the reduced system by block cyclic reduction -- k_cr_level01 (first two levels, one
//                      workgroup per four separators) and k_solve_reduced_cr (the rest in one workgroup) -- and the
//                      recovery inside the trial kernel (vba_step.h).
//
// Files: vba_solve_step.h (this), vba_solve_seq.hip (sequential walks), vba_solve_chunk_body.h + vba_solve_chunks.hip
// (partitioned chain), vba_solve_cr_body.h + vba_solve_cr.hip (block cyclic reduction of the reduced system), vba_solve.hip (accept
// test and the host dispatch), vba_solve_variants.hip (comparison builds only: the measured dead ends).  The build has no
// relocatable device code, so device functions that two units need live in the headers.
#pragma once

#include "vba_device.h"

namespace vba {

typedef double vf4 __attribute__((ext_vector_type(4)));     // accumulator of v_mfma_f64_16x16x4

// Diagnostic builds (-DVBA_RESIDENT_STAMPS; tools/attic/tail_stamps.py): 100 MHz wall-clock stamps of one thread along the
// single-window solve kernels, fetched with vba_debug_fetch(h, 0, 101, ...).  A device global does not link across
// translation units, so every solver unit that stamps has its own copy of the array (VBA_KSTAMP_FETCH defines the unit's
// reader) and fetch_kstamps (vba_solve.hip) returns, per slot, the latest value of all copies: the stamps are wall-clock
// readings, so that is the unit whose kernel ran last.
#ifdef VBA_RESIDENT_STAMPS
[[maybe_unused]] static __device__ unsigned long long g_kstamps[128];
#define VBA_KSTAMP(on, slot) do { if (on) g_kstamps[slot] = wall_clock64(); } while (0)
#define VBA_KSTAMP_FETCH(name) \
    void name(unsigned long long* out) { (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_kstamps), sizeof(g_kstamps)); }
#else
#define VBA_KSTAMP(on, slot) do {} while (0)
#endif

// Lane roles of a forward step.  DB = first lane of the D' group (0 or 9), the U group starts at 9 - DB,
// right-hand-side columns sit in lanes [18, 18 + NRHS).
template <int DB, int NRHS>
struct Roles {
    static constexpr int UB = 9 - DB;
    __device__ static bool isD(int lane) { return lane >= DB && lane < DB + 9; }
    __device__ static bool isU(int lane) { return lane >= UB && lane < UB + 9; }
    __device__ static bool isR(int lane) { return lane >= 18 && lane < 18 + NRHS; }
};

// a[] enters holding this lane's column of [X_{i-1} | z_{i-1}] (or zeros), base[] this lane's column of
// [D_i + lam I | U_i | rhs_i]; on exit a[] holds the column of [I | X_i | z_i].  Lmat (LDS, row major 9x9) is
// L_i, or null for the first block of a chain.
//
// Per pivot the dependent chain is: lane-local tree search for the largest |entry| of the pivot column ->
// reciprocal of that entry (computed by every lane on its own candidate, only the pivot lane's is used) ->
// two broadcasts (row index, reciprocal) -> scale -> rank-1 update.  The row swap and the broadcasts of the
// eight multipliers run beside the reciprocal.
// PIVOT = false is the fast path: the damped normal equations are symmetric positive definite up to a ~1e-6
// relative non-symmetric term, for which elimination without row exchanges is as stable as Cholesky; every
// pivot is checked against the diagonal entry it started from and a failed check (`bad`) makes the host repeat
// the solve with PIVOT = true (row pivoting inside the 9x9 block).
// SPARSE_L: L_i of the assembled system has the pattern [pp 0 pv; 0 rr 0; vp 0 vv] over (position, rotation,
// velocity) (the orbit factor does not touch the rotation slots and the attitude term touches nothing else),
// so 45 instead of 81 multiply-adds; not valid for the reduced system.
// GROUPED: the wave holds several independent chains side by side (19 lanes each, `lane` is the lane inside the
// group, `gbase` the group's first lane); broadcasts then come from the group's own pivot lane through the LDS
// crossbar (ds_bpermute) instead of v_readlane, and the pivot row index is a per-lane value.
template <bool GROUPED>
__device__ __forceinline__ double bcast_f64(double v, int src) {
    if (GROUPED) return __shfl(v, src, kWave);
    return readlane_f64(v, src);
}
template <bool GROUPED>
__device__ __forceinline__ int bcast_i32(int v, int src) {
    if (GROUPED) return __shfl(v, src, kWave);
    return __builtin_amdgcn_readlane(v, src);
}

template <int DB, int NRHS, bool PIVOT, bool SPARSE_L, bool GROUPED = false>
__device__ __forceinline__ void forward_step(const double* Lmat, const double (&base)[9], double (&a)[9], int lane,
                                             bool& bad, int gbase = 0) {
    using R = Roles<DB, NRHS>;
    const bool carry = R::isD(lane) || R::isR(lane);
    double xp[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) xp[j] = carry ? a[j] : 0.0;
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        double v = base[r];
        if (Lmat) {
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                const bool rot_r = (r >= 3 && r < 6), rot_j = (j >= 3 && j < 6);
                if (!SPARSE_L || rot_r == rot_j) v = fma(-Lmat[r * 9 + j], xp[j], v);   // broadcast LDS read
            }
        }
        a[r] = v;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int pl = DB + k;
        double inv;
        if (PIVOT) {
            // lane-local tree search for the largest |entry| of the pivot column, reciprocal of that entry
            // computed by every lane on its own candidate, then two broadcasts (row index, reciprocal)
            const int cnt = 9 - k;
            double cv[9], cs[9];
            int ci[9];
#pragma unroll
            for (int r = 0; r < 9; ++r) {
                if (r < cnt) { cs[r] = a[k + r]; cv[r] = fabs(cs[r]); ci[r] = k + r; }
            }
#pragma unroll
            for (int step = 1; step < 9; step *= 2) {
#pragma unroll
                for (int r = 0; r < 9; r += 2 * step) {
                    if (r + step < cnt) {
                        const bool take = cv[r + step] > cv[r];       // strict: the lowest row wins a tie
                        cv[r] = take ? cv[r + step] : cv[r];
                        cs[r] = take ? cs[r + step] : cs[r];
                        ci[r] = take ? ci[r + step] : ci[r];
                    }
                }
            }
            const double inv_l = fast_rcp(cs[0]);
            const int p = bcast_i32<GROUPED>(ci[0], gbase + pl);
            inv = bcast_f64<GROUPED>(inv_l, gbase + pl);
            if (!(fabs(inv) <= 1.79e308)) bad = true;
            const double ak = a[k];
            double nk = ak;
#pragma unroll
            for (int r = k + 1; r < 9; ++r) {     // row swap k <-> p (p is wave uniform), branch free
                const bool sel = (p == r);
                const double ar = a[r];
                nk = sel ? ar : nk;
                a[r] = sel ? ak : ar;
            }
            a[k] = nk;
        } else {
            // pivot on the diagonal; it must stay a healthy fraction of the diagonal entry it started from
            if (lane == pl && !(a[k] > 1e-10 * base[k])) bad = true;
            inv = bcast_f64<GROUPED>(fast_rcp(a[k]), gbase + pl);
        }
        double f[9];
#pragma unroll
        for (int r = 0; r < 9; ++r) f[r] = (r != k) ? bcast_f64<GROUPED>(a[r], gbase + pl) : 0.0;
        a[k] = a[k] * inv;
#pragma unroll
        for (int r = 0; r < 9; ++r) {
            if (r != k) a[r] = fma(-f[r], a[k], a[r]);
        }
    }
}

// The unpivoted elimination with row broadcasts (DPP) instead of v_readlane: every ROW of 16 lanes holds the nine columns of
// D in its lanes 0..8 (the same values in all rows: each row pivots its own copy) and seven of the nineteen columns of
// [L | U | g] in lanes 9..15 (rows 0..2; row 3 idles).  A pivot is then reciprocal -> one v_mov_b64_dpp -> scale -> eight
// v_fmac_f64_dpp (dpp_rank1_9) per lane instead of twenty v_readlane through scalar registers + nine multiply-adds -- the
// same operations per entry in the same order as forward_step<0, 10, false, false>, so the same bits.
template <int K = 0>
__device__ __forceinline__ void cr_pivots_dpp(const double (&base)[9], double (&a)[9], int c, bool& bad) {
    if constexpr (K < 9) {
        bad = bad | ((c == K) & !(a[K] > 1e-10 * base[K]));
        const double inv = bcast_row16<K>(fast_rcp(a[K]));
        a[K] = a[K] * inv;
        dpp_rank1_9<K>(a);
        cr_pivots_dpp<K + 1>(base, a, c, bad);
    }
}

// A failed pivot check: with row pivoting it is a numerically singular block (flag 4, result kept as in the
// reference); without it the host is asked to repeat this solve with pivoting (internal flag 8) and the window
// stays on the pivoted kernels for the rest of the call (internal flag 16).  The choice is per window, so what one
// window of a batch needs never changes the arithmetic of another.
// V.pivot: 0 = only the unpivoted kernels are launched, 1 = only the pivoted ones and they take every window,
// 2 = both are launched and each takes the windows whose sticky bit matches.
template <bool PIVOT>
__device__ __forceinline__ bool solver_mine(const DevView& V, const WinScalars& sc) {
    if (V.pivot == 1) return PIVOT;
    return ((sc.fl[V.par] & 16u) != 0) == PIVOT;
}

template <bool PIVOT>
__device__ __forceinline__ void report_pivot(bool bad, WinScalars& sc, int lane, int par) {
    const unsigned long long any = __ballot(bad);
    if (lane == 0 && any) atomicOr(&sc.fl[par], PIVOT ? 4u : (8u | 16u));
}

// LDS written by one wave of a workgroup is there for the other waves' later reads: fence, no s_barrier (the waves meet at
// __syncthreads() where they have to)
__device__ __forceinline__ void wave_sync_lds() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// number of separators of a chain of n blocks cut into chunks of s
__device__ __forceinline__ int n_separators(int n, int s) { return (n + s - 1) / s - 1; }

// ================================================================================================== sequential
// Walks blocks [0, n) of a block-tridiagonal system stored as bands[n][3][81], rhs[n][9]; damping lam32 is
// added to the diagonal.  Writes the solution to x[n][9].  Xs/zs: scratch [n][81], [n][9] in global memory.
// block sources: entry e of block i, e in [0,243) = sub|diag|super row major, [243,252) = right-hand side
struct BandSource {
    const double* bands;
    const double* rhs;
    __device__ double operator()(int i, int e) const { return e < 243 ? bands[(size_t)i * 243 + e] : rhs[(size_t)i * 9 + (e - 243)]; }
};

// A source may stage its own inputs beside the walk (RawSource): prefetch(i) starts the loads of what block i needs,
// commit(i) puts them where operator() finds them; the barrier of the walk's step orders the two.  No-ops otherwise.
template <class S> __device__ __forceinline__ auto src_prefetch(const S& s, int i, int) -> decltype(s.prefetch(i), void()) { s.prefetch(i); }
template <class S> __device__ __forceinline__ void src_prefetch(const S&, int, long) {}
template <class S> __device__ __forceinline__ auto src_commit(const S& s, int i, int) -> decltype(s.commit(i), void()) { s.commit(i); }
template <class S> __device__ __forceinline__ void src_commit(const S&, int, long) {}
// a source that COMPUTES its entries takes them behind the elimination step (nothing of it is live across the step)
template <class S> constexpr auto src_late(int) -> decltype(S::kLateFetch) { return S::kLateFetch; }
template <class S> constexpr bool src_late(long) { return false; }

template <bool PIVOT, bool SPARSE_L, class Src>
__device__ __forceinline__ void chain_solve(const Src& src, int n, double lam32, double* Xs, double* zs, double* x_out,
                                            double (*blk)[256], int lane, bool& zero_pivot) {
    double a[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) a[j] = 0.0;
    double pre[4];
    auto fetch = [&](int i) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = lane + 64 * q;
            pre[q] = e < 252 ? src(i, e) : 0.0;
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int q = 0; q < 4; ++q) blk[buf][lane + 64 * q] = pre[q];
    };
    auto load_base = [&](const double* b, int db, double (&base)[9]) {
        const int ub = 9 - db;
        const bool isD = lane >= db && lane < db + 9, isU = lane >= ub && lane < ub + 9, isY = lane == 18;
        const int cc = isD ? lane - db : (isU ? lane - ub : 0);
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
        constexpr bool late = src_late<Src>(0);
        src_prefetch(src, i + 2, 0);
        if (!late && i + 1 < n) fetch(i + 1);
        double base[9];
        if (buf == 0) {
            load_base(blk[0], 0, base);
            forward_step<0, 1, PIVOT, SPARSE_L>(i > 0 ? blk[0] : nullptr, base, a, lane, zero_pivot);
        } else {
            load_base(blk[1], 9, base);
            forward_step<9, 1, PIVOT, SPARSE_L>(blk[1], base, a, lane, zero_pivot);
        }
        const int ub = buf == 0 ? 9 : 0;    // X_i sits in the U group of this step, z_i in lane 18
        if (lane >= ub && lane < ub + 9) {
            double* X = Xs + (size_t)i * 81 + (lane - ub);
#pragma unroll
            for (int r = 0; r < 9; ++r) X[r * 9] = a[r];
        } else if (lane == 18) {
            double* z = zs + (size_t)i * 9;
#pragma unroll
            for (int r = 0; r < 9; ++r) z[r] = a[r];
        }
        if constexpr (late) {
            if (i + 1 < n) src.form(i + 1, blk[buf ^ 1]);       // the whole block in uniform passes, straight into the other buffer
        } else {
            if (i + 1 < n) stash(buf ^ 1);
        }
        src_commit(src, i + 2, 0);
        __syncthreads();
    }
    __threadfence_block();
    __syncthreads();
    // backward sweep, lane r = row r
    const int r = lane < 9 ? lane : 0;
    double x = zs[(size_t)(n - 1) * 9 + r];
    if (lane < 9) x_out[(size_t)(n - 1) * 9 + r] = x;
    double Xrow[9], zr = 0.0;
    auto fetch_row = [&](int i) {
        const double* X = Xs + (size_t)i * 81 + r * 9;
#pragma unroll
        for (int j = 0; j < 9; ++j) Xrow[j] = X[j];
        zr = zs[(size_t)i * 9 + r];
    };
    if (n > 1) fetch_row(n - 2);
    for (int i = n - 2; i >= 0; --i) {
        double cur[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) cur[j] = Xrow[j];
        double v = zr;
        if (i > 0) fetch_row(i - 1);
#pragma unroll
        for (int j = 0; j < 9; ++j) v -= cur[j] * readlane_f64(x, j);
        x = v;
        if (lane < 9) x_out[(size_t)i * 9 + r] = x;
    }
    __threadfence_block();
    __syncthreads();
}

// retraction of poses [lane, lane+64, ...) (BA_filtering.py:56-60); returns true if a non-finite step was seen
__device__ __forceinline__ bool retract_range(const DevView& V, size_t sb, int n, int first, int stride) {
    bool bad = false;
    for (int i = first; i < n; i += stride) {
        const double* dp = V.dpose + (sb + i) * 9;
        double d9[9], o[10];
#pragma unroll
        for (int j = 0; j < 9; ++j) { d9[j] = dp[j]; bad |= !(fabs(d9[j]) <= 1.79e308); }
        retract(V.states + (sb + i) * 10, d9, o);
        double* sn = V.states_new + (sb + i) * 10;
#pragma unroll
        for (int j = 0; j < 10; ++j) sn[j] = o[j];
    }
    return bad;
}

}  // namespace vba
