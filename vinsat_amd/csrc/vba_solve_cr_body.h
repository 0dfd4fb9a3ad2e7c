// vba_solve_cr_body.h -- device bodies of the block cyclic reduction of the reduced system: the two block operations
// (eliminate, fold), the fill of the blocks from what the chunk waves left, the two levels in front (cr_level01_body) and the
// one-workgroup kernel (reduced_cr_body, k_solve_reduced_cr).  Included by vba_solve_cr.hip (the production kernels) and by the
// comparison unit (other numbers of levels in front, the resident solve).
#pragma once

#include "vba_solve_step.h"
#include "vba_solve_units.h"

namespace vba {

// The reduced system over the separators by block cyclic reduction inside ONE workgroup (16 waves, the whole system
// in LDS): log2(n1) levels of "every other block eliminated in parallel" instead of n1 sequential block steps.
//   level with stride h, active blocks k = r h - 1 (r = 1, 2, ...):
//     A  odd r:   [PL | PU | Pg]_k = D_k^{-1} [L_k | U_k | g_k]                   (one Gauss-Jordan per wave, in place)
//     B  even r:  D_j -= L_j PU_{j-h} + U_j PL_{j+h},  g_j -= L_j Pg_{j-h} + U_j Pg_{j+h},
//                 L_j  = -L_j PL_{j-h},  U_j = -U_j PU_{j+h}                        (couples j to j -+ 2h from now on)
//   back substitution, coarsest level first:  x_k = Pg_k - PL_k x_{k-h} - PU_k x_{k+h}.
// Schur complements of the (damped, near-SPD) system stay near-SPD, so the unpivoted path applies with the same
// per-pivot check; PIVOT exchanges rows inside a block as everywhere else.
// LDS: n1 blocks of 252 doubles [L | D | U | g]; x overwrites g.  n1 <= kCrMax.

// Per-lane geometry of the two block operations (depends on the lane only, built once per kernel).
struct CrLanes {
    // elimination (A): lane -> column of [D | L | U | g]; one address per lane and role (selecting among loaded
    // VALUES would make every lane load every alternative)
    int grp, own, ownst;
    // fold (B) on the matrix cores:
    //   out (9 x 28: new D | L | U | g) = init - [L_j | U_j] (9 x 18) * Bm (18 x 28),
    //   Bm rows 0..8  = [PU | PL | 0  | Pg] of the left neighbour,  rows 9..17 = [PL | 0 | PU | Pg] of the right one.
    // v_mfma_f64_16x16x4: lane l feeds A[l & 15][4 s + (l >> 4)] and B[4 s + (l >> 4)][l & 15] of k-step s and owns
    // C[(l >> 4) + 4 i][l & 15], i = 0..3; two column tiles, five k-steps.  One LDS read per operand element instead
    // of 162 broadcast reads per lane (the VALU form was LDS-bandwidth-bound).
    int lr, lk;
    int offA[5], offB0[5], offB1[5];    // -1: structural zero
    bool hiB[5];                        // the B element comes from the right neighbour
};

__device__ __forceinline__ CrLanes cr_lanes(int lane) {
    CrLanes g;
    g.grp = lane < 9 ? 0 : (lane < 18 ? 1 : (lane < 27 ? 2 : (lane == 27 ? 3 : 4)));
    const int c = g.grp < 3 ? lane - 9 * g.grp : 0;
    g.own = g.grp == 0 ? 81 + c : (g.grp == 1 ? c : (g.grp == 2 ? 162 + c : 243));
    g.ownst = g.grp == 3 ? 1 : 9;
    g.lr = lane & 15;
    g.lk = lane >> 4;
#pragma unroll
    for (int st = 0; st < 5; ++st) {
        const int k = 4 * st + g.lk;
        g.offA[st] = (g.lr < 9 && k < 18) ? (k < 9 ? g.lr * 9 + k : 162 + g.lr * 9 + (k - 9)) : -1;
        const bool lo = k < 9;
        const int q = lo ? k : k - 9;
        g.hiB[st] = !lo;
        auto bm = [&](int col) -> int {
            if (k >= 18) return -1;
            if (col < 9) return lo ? 162 + q * 9 + col : q * 9 + col;
            if (col < 18) return lo ? q * 9 + col - 9 : -1;
            if (col < 27) return lo ? -1 : 162 + q * 9 + col - 18;
            if (col == 27) return 243 + q;
            return -1;
        };
        g.offB0[st] = bm(g.lr);
        g.offB1[st] = bm(16 + g.lr);
    }
    return g;
}

// (cr_pivots_dpp, above forward_step's users: D replicated per row of 16 lanes, seven other columns per row)
__device__ __forceinline__ void cr_eliminate_dpp(double* B, int lane, bool& bad) {
    const int row = lane >> 4, c = lane & 15;
    const int o = row * 7 + (c - 9);                    // column of [L | U | g] of a lane with c >= 9
    const bool isD = c < 9, isX = !isD && o < 19;
    const int off = isD ? 81 + c : (o < 9 ? o : (o < 18 ? 162 + (o - 9) : 243));
    const int st = (isX && o == 18) ? 1 : 9;
    const double* p = B + ((isD || isX) ? off : 0);
    double a[9], base[9];
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        const double v = p[r * st];
        a[r] = (isD || isX) ? v : 0.0;
        base[r] = a[r];
    }
    bool mybad = false;
    cr_pivots_dpp<0>(base, a, c, mybad);
    bad = bad | (isD & mybad);
    if (isX) {
        double* q = B + off;
#pragma unroll
        for (int r = 0; r < 9; ++r) q[r * st] = a[r];
    }
}

// A: [PL | PU | Pg] = D^{-1} [L | U | g] of block B (LDS, 252 doubles), in place; one wave.
template <bool PIVOT>
__device__ __forceinline__ void cr_eliminate(double* B, const CrLanes& g, int lane, bool& bad) {
#ifndef VBA_CR_READLANE
    if constexpr (!PIVOT) {
        cr_eliminate_dpp(B, lane, bad);
        return;
    }
#endif
    double base[9], a[9];
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        const double v = B[g.own + r * g.ownst];
        base[r] = g.grp < 4 ? v : 0.0;
        a[r] = 0.0;
    }
    forward_step<0, 10, PIVOT, false>(nullptr, base, a, lane, bad);
    if (g.grp >= 1 && g.grp <= 3) {
#pragma unroll
        for (int r = 0; r < 9; ++r) B[g.own + r * g.ownst] = a[r];
    }
}

// B: fold the eliminated neighbours Pm (left) and Pp (right, if has_p) into block Bj, in place; one wave.
__device__ __forceinline__ void cr_fold(double* Bj, const double* Pm, const double* Pp, bool has_p, const CrLanes& g) {
    vf4 acc0, acc1;
    VBA_KSTAMP(threadIdx.x == 0 && gridDim.y == 1 && blockDim.x == 1024, 79);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = g.lk + 4 * i;
        const bool rv = row < 9;
        const double d0 = Bj[(rv && g.lr < 9) ? 81 + row * 9 + g.lr : 0];
        const double g0 = Bj[(rv && g.lr == 11) ? 243 + row : 0];
        acc0[i] = (rv && g.lr < 9) ? d0 : 0.0;
        acc1[i] = (rv && g.lr == 11) ? g0 : 0.0;      // column 27 = 16 + 11
    }
    // every LDS operand first (15 reads in flight together), then the chain of matrix operations: left to itself the
    // compiler reads each k-step's operands right in front of its two MFMAs -- five LDS round trips one after the other
    double am[5], b0[5], b1[5];
#pragma unroll
    for (int st = 0; st < 5; ++st) {
        const double a0 = Bj[g.offA[st] >= 0 ? g.offA[st] : 0];
        am[st] = g.offA[st] >= 0 ? -a0 : 0.0;
        const double* P = g.hiB[st] ? Pp : Pm;
        const bool okp = !g.hiB[st] || has_p;
        const double v0 = P[g.offB0[st] >= 0 ? g.offB0[st] : 0], v1 = P[g.offB1[st] >= 0 ? g.offB1[st] : 0];
        b0[st] = (okp && g.offB0[st] >= 0) ? v0 : 0.0;
        b1[st] = (okp && g.offB1[st] >= 0) ? v1 : 0.0;
    }
#ifndef VBA_FOLD_INTERLEAVED
    __builtin_amdgcn_sched_barrier(0);
#endif
#ifdef VBA_RESIDENT_STAMPS
    const bool fson = threadIdx.x == 0 && gridDim.y == 1 && blockDim.x == 1024;
    VBA_KSTAMP(fson, 80);
    if (fson) g_kstamps[81] = (unsigned long long)(am[0] + b0[0] + b1[4] + am[4] != 12345.0);   // (forces the operands)
    VBA_KSTAMP(fson, 82);
#endif
#pragma unroll
    for (int st = 0; st < 5; ++st) {
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(am[st], b0[st], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(am[st], b1[st], acc1, 0, 0, 0);
    }
#ifdef VBA_RESIDENT_STAMPS
    if (fson) g_kstamps[83] = (unsigned long long)(acc0[0] + acc1[3] != 12345.0);               // (forces the results)
    VBA_KSTAMP(fson, 84);
#endif
    // every operand has been read (the LDS operations of a wave execute in order): replace the block.  One destination per
    // lane and tile, decided by arithmetic -- as nested branches this tail was twenty basic blocks
    const int c1 = 16 + g.lr;
    const int col0 = g.lr < 9 ? 81 + g.lr : g.lr - 9;                                              // D | L columns 0..6
    const int col1 = c1 < 18 ? c1 - 9 : (c1 < 27 ? 162 + (c1 - 18) : 243);                         // L columns 7, 8 | U | g
    const int st1 = c1 == 27 ? 1 : 9;
    const bool has1 = c1 <= 27;
    // ... and every lane stores every time: a lane without an entry repeats its own first one (row g.lk < 4 of tile 0 always
    // exists) -- a predicated store is a branch region of its own
    const int home = col0 + g.lk * 9;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = g.lk + 4 * i;
        const bool ok0 = row < 9, ok1 = ok0 && has1;
        Bj[ok0 ? col0 + row * 9 : home] = ok0 ? acc0[i] : acc0[0];
        Bj[ok1 ? col1 + row * st1 : home] = ok1 ? acc1[i] : acc0[0];
    }
#ifdef VBA_RESIDENT_STAMPS
    VBA_KSTAMP(fson, 85);
#endif
}

// Blocks q0 + u * stride (u < NB) of the reduced system (see ReducedSource) into LDS at dst + u * dst_stride * 252.  A wave takes
// whole blocks and a lane the same (row, column) of L, D and U, so the index arithmetic is done once per three
// entries and nothing diverges (walking the 252 entries of a block through the generic source costs more in integer
// divisions and branches than in loads); all loads are issued before the first store.
// between(): called when the loads have been issued and before the first store waits for them (lane geometry and the like)
template <int NB, class Between>
__device__ __forceinline__ void cr_fill(const DevView& V, int w, int s, int n1, double lam32, int q0, int stride, double* dst, int dst_stride, int lane,
                                        Between&& between) {
    const size_t sb = (size_t)w * V.n_max, rb = (size_t)w * V.p_max;
    const double* bands = V.bands + sb * 243;
    const double* rhs = V.rhs + sb * 9;
    const double* cL = V.cL + rb * 171;
    const double* cR = V.cR + rb * 171;
    const int r0 = lane / 9, c0 = lane % 9, r1 = (lane + 64) / 9, c1 = (lane + 64) % 9;
    double lv[NB][2], lw[NB][2], rv[NB][2], rw[NB][2], dv[NB][2], gv[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        const int q = q0 + u * stride;
        const bool in = q >= 0 && q < n1;
        const size_t j = in ? (size_t)(q + 1) * s - 1 : 0;
        const double* l = cL + (size_t)(in ? q : 0) * 171;
        const double* r_ = cR + (size_t)(in ? q : 0) * 171;
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int r = it ? r1 : r0, cc = it ? c1 : c0;
            const bool ok = in && lane + 64 * it < 81;
            lv[u][it] = ok ? l[r * 19 + 1 + cc] : 0.0;
            lw[u][it] = ok ? l[r * 19 + 10 + cc] : 0.0;
            rv[u][it] = ok ? r_[r * 19 + 1 + cc] : 0.0;
            rw[u][it] = ok ? r_[r * 19 + 10 + cc] : 0.0;
            dv[u][it] = ok ? bands[j * 243 + 81 + lane + 64 * it] : 0.0;
        }
        gv[u] = (in && lane < 9) ? rhs[j * 9 + lane] - l[lane * 19] - r_[lane * 19] : 0.0;
    }
    between();
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        const int q = q0 + u * stride;
        if (q >= 0 && q < n1) {
            double* B = dst + (size_t)u * dst_stride * 252;
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const int i = lane + 64 * it;
                if (i < 81) {
                    const int r = it ? r1 : r0, cc = it ? c1 : c0;
                    B[i] = q == 0 ? 0.0 : -lv[u][it];                       // no neighbour on that side
                    B[81 + i] = dv[u][it] - lw[u][it] - rv[u][it] + (r == cc ? lam32 : 0.0);
                    B[162 + i] = q == n1 - 1 ? 0.0 : -rw[u][it];
                }
            }
            if (lane < 9) B[243 + lane] = gv[u];
        }
    }
}

// The first TWO levels on their own CUs: four waves per group of four separators.  Group t builds the seven blocks
// 4t .. 4t+6, eliminates the even ones (four waves side by side), folds them into 4t+1, 4t+3, 4t+5, eliminates 4t+1 and
// 4t+5 (level 1: every other odd block) and folds those into 4t+3.  It leaves
//   red2[t] = the twice-folded block 4t+3 (252 doubles),  P[4t], P[4t+2] (level 0) and P[4t+1] (level 1) = [PL | PU | Pg]
// in global memory; what it shares with its neighbour groups (blocks 4t+4 .. 4t+6) is computed by both: redundant work
// instead of communication.  In the one-workgroup kernel the first level ran 16 eliminations on the four SIMDs of one CU
// (5.8 us, issue-bound at four waves per SIMD) -- here they are spread over 16 CUs and that kernel starts from 15 blocks.
template <bool PIVOT>
__device__ __forceinline__ void cr_level01_body(const DevView& V, int s, int w, int t, double* blk) {
    VBA_SKIP_CALL(V, w);
    WinScalars& sc = V.sc[w];
    if (sc.done || !solver_mine<PIVOT>(V, sc)) return;
    const int n1 = n_separators(V.n[w], s);
    if (n1 < kCrSplitMin || n1 > 4 * kCrMax || 4 * t >= n1) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t rb = (size_t)w * V.p_max;
    const double lam32 = (double)(float)sc.lam[V.par];
    const int q0 = 4 * t;
    CrLanes g;
    cr_fill<2>(V, w, s, n1, lam32, q0 + wv, 4, blk + (size_t)wv * 252, 4, lane, [&]() { g = cr_lanes(lane); });     // blocks wv, wv + 4
    __syncthreads();
    bool bad = false;
    auto store_P = [&](int u) {         // [PL | PU | Pg] of block q0 + u
        double* P = V.csol2 + (rb + q0 + u) * 171;
        const double* B = blk + (size_t)u * 252;
        for (int e = lane; e < 171; e += 64) P[e] = e < 81 ? B[e] : B[81 + e];
    };
    // level 0: the even blocks
    if (q0 + 2 * wv < n1) cr_eliminate<PIVOT>(blk + (size_t)(2 * wv) * 252, g, lane, bad);
    __syncthreads();
    if (wv < 3) {
        const int u = 2 * wv + 1;
        if (q0 + u < n1) cr_fold(blk + (size_t)u * 252, blk + (size_t)(u - 1) * 252, blk + (size_t)(u + 1) * 252, q0 + u + 1 < n1, g);
    } else {
        store_P(0);
        if (q0 + 2 < n1) store_P(2);
    }
    __syncthreads();
    // level 1: blocks 4t+1 and 4t+5
    if (wv < 2) {
        const int u = 4 * wv + 1;
        if (q0 + u < n1) cr_eliminate<PIVOT>(blk + (size_t)u * 252, g, lane, bad);
    }
    __syncthreads();
    if (wv == 0) {
        if (q0 + 3 < n1) {
            cr_fold(blk + 3 * 252, blk + 1 * 252, blk + 5 * 252, q0 + 5 < n1, g);
            wave_sync_lds();
            double* R = V.cL2 + rb * 171 + (size_t)t * 252;
            for (int e = lane; e < 252; e += 64) R[e] = blk[3 * 252 + e];
        }
    } else if (wv == 1) {
        if (q0 + 1 < n1) store_P(1);
    }
    report_pivot<PIVOT>(bad, sc, lane, V.par);
}

// PRE: the first level has been done by k_cr_level0; this kernel continues with the n1 / 2 folded blocks and finishes
// with the back substitution of the level-0 blocks.
// PRE 2: the first two levels have been done by k_cr_level01; the system solved here is over the separators 4b + 3.
template <bool PIVOT, int PRE, int kCrThreads>
__device__ __forceinline__ void reduced_cr_body(const DevView& V, int s, int w, double* smem) {
    VBA_SKIP_CALL(V, w);
    int tsi = 0;
    const bool tson = threadIdx.x == 0;
    VBA_KSTAMP(tson, tsi++);
    WinScalars& sc = V.sc[w];
    if (sc.done || !solver_mine<PIVOT>(V, sc)) return;
    const int n0 = n_separators(V.n[w], s);             // separators of the window
    if (n0 <= 0) return;
    if (PRE ? (n0 < kCrSplitMin || n0 > (PRE == 3 ? 8 : (PRE == 2 ? 4 : 2)) * kCrMax) : (n0 >= kCrSplitMin || n0 > kCrMax)) return;   // the other variant's window
    const int n1 = PRE == 3 ? n0 / 8 : (PRE == 2 ? n0 / 4 : (PRE ? n0 / 2 : n0));             // blocks of the system solved here
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int NW = kCrThreads / 64;
    const size_t rb = (size_t)w * V.p_max;
    const double lam32 = (double)(float)sc.lam[V.par];
    CrLanes g;
    if (PRE) {
        // all loads of a thread before its first store: a copy loop waits for every element in turn (up to 16 dependent
        // round trips here -- a third of this kernel's time when it was written that way)
        const double* R = V.cL2 + rb * 171;
        constexpr int kFill = (kCrMax * 252 + kCrThreads - 1) / kCrThreads;
        double v[kFill];
#pragma unroll
        for (int k = 0; k < kFill; ++k) {
            const int idx = tid + k * kCrThreads;
            v[k] = idx < n1 * 252 ? R[idx] : 0.0;
        }
        g = cr_lanes(lane);     // (while the loads are in flight)
#pragma unroll
        for (int k = 0; k < kFill; ++k) {
            const int idx = tid + k * kCrThreads;
            if (idx < n1 * 252) smem[idx] = v[k];
        }
    } else {
        cr_fill<kCrMax / NW>(V, w, s, n1, lam32, wave, NW, smem + (size_t)wave * 252, NW, lane, [&]() { g = cr_lanes(lane); });   // blocks wave, wave + NW, ...
    }
    __syncthreads();
    VBA_KSTAMP(tson, tsi++);
    bool bad = false;
    int h = 1, lv = 0;                          // h = 1 << lv (shifts: a division by a run-time h is ~40 instructions per level)
    for (;; h <<= 1, ++lv) {
        const int cnt = n1 >> lv;               // active blocks of this level
        const int nel = (cnt + 1) / 2;
#pragma nounroll
        for (int t = wave; t < nel; t += NW)    // A: eliminate the odd-ranked blocks
            cr_eliminate<PIVOT>(smem + (size_t)((2 * t + 1) * h - 1) * 252, g, lane, bad);
        __syncthreads();
        VBA_KSTAMP(tson, tsi++);
        if (cnt <= 1) break;
        const int nk = cnt / 2;
#pragma nounroll
        for (int t = wave; t < nk; t += NW) {   // B: fold the eliminated neighbours into the even-ranked blocks
            const int j = (2 * t + 2) * h - 1;
            const bool has_p = j + h < n1;
            cr_fold(smem + (size_t)j * 252, smem + (size_t)(j - h) * 252, smem + (size_t)(has_p ? j + h : j) * 252, has_p, g);
        }
        VBA_KSTAMP(tson, 64 + tsi);
        __syncthreads();
        VBA_KSTAMP(tson, tsi++);
    }
    // back substitution: the level that ended the loop has a single block with no active neighbour (x = Pg)
    for (; h >= 1; h >>= 1, --lv) {
        const int cnt = n1 >> lv;
        const int nel = (cnt + 1) / 2;
        for (int idx = tid; idx < nel * 9; idx += kCrThreads) {
            const int t = idx / 9, r = idx % 9;
            const int k = (2 * t + 1) * h - 1;
            double* B = smem + (size_t)k * 252;
            double x = B[243 + r];
            if (k - h >= 0) {
                const double* xm = smem + (size_t)(k - h) * 252 + 243;
#pragma unroll
                for (int q = 0; q < 9; ++q) x -= B[r * 9 + q] * xm[q];
            }
            if (k + h < n1) {
                const double* xp = smem + (size_t)(k + h) * 252 + 243;
#pragma unroll
                for (int q = 0; q < 9; ++q) x -= B[162 + r * 9 + q] * xp[q];
            }
            B[243 + r] = x;     // read only by this thread at this level (the neighbours belong to coarser levels)
        }
        __syncthreads();
        VBA_KSTAMP(tson, tsi++);
    }
    if (PRE == 3) {
        // separators 8b+7 are the blocks solved here.  8b+3 come from the level-2 eliminations, x = Pg - PL x_{q-4} - PU x_{q+4};
        // then 4b+1 from level 1 (neighbours q -+ 2), then the even ones from level 0 (neighbours q -+ 1)
        double* x2 = smem + (size_t)n1 * 252;                   // [ceil(n0 / 8)][9]
        double* x1 = x2 + (size_t)((n0 + 7) / 8) * 9;           // [ceil(n0 / 4)][9]
        auto x_odd = [&](int q) -> const double* {              // solution of an odd separator
            return (q & 7) == 7 ? smem + (size_t)(q >> 3) * 252 + 243 : ((q & 7) == 3 ? x2 + (size_t)(q >> 3) * 9 : x1 + (size_t)(q >> 2) * 9);
        };
        auto solve_from = [&](int q, int r, int h) {            // row r of separator q from its P rows and the solutions h away
            const double* P = V.csol2 + (rb + q) * 171;
            double x = P[162 + r];
            if (q - h >= 0) {
                const double* xm = x_odd(q - h);
#pragma unroll
                for (int k = 0; k < 9; ++k) x -= P[r * 9 + k] * xm[k];
            }
            if (q + h < n0) {
                const double* xp = x_odd(q + h);
#pragma unroll
                for (int k = 0; k < 9; ++k) x -= P[81 + r * 9 + k] * xp[k];
            }
            return x;
        };
        for (int idx = tid; idx < ((n0 + 7) / 8) * 9; idx += kCrThreads) {
            const int q = 8 * (idx / 9) + 3, r = idx % 9;
            if (q < n0) x2[(size_t)(q >> 3) * 9 + r] = solve_from(q, r, 4);
        }
        __syncthreads();
        for (int idx = tid; idx < ((n0 + 3) / 4) * 9; idx += kCrThreads) {
            const int q = 4 * (idx / 9) + 1, r = idx % 9;
            if (q < n0) x1[(size_t)(q >> 2) * 9 + r] = solve_from(q, r, 2);
        }
        __syncthreads();
        for (int idx = tid; idx < n0 * 9; idx += kCrThreads) {
            const int q = idx / 9, r = idx % 9;
            V.rx[rb * 9 + idx] = (q & 1) ? x_odd(q)[r] : solve_from(q, r, 1);
        }
    } else if (PRE == 2) {
        // separators 4b+3 are the blocks solved here.  4b+1 come from the level-1 eliminations, x = Pg - PL x_{q-2} - PU x_{q+2},
        // then the even ones from level 0, x = Pg - PL x_{q-1} - PU x_{q+1}
        double* x1 = smem + (size_t)n1 * 252;       // [ceil(n0 / 4)][9]: the level-1 solutions (behind the blocks)
        auto x_odd = [&](int q) -> const double* {  // solution of an odd separator
            return (q & 3) == 3 ? smem + (size_t)(q >> 2) * 252 + 243 : x1 + (size_t)(q >> 2) * 9;
        };
        for (int idx = tid; idx < ((n0 + 3) / 4) * 9; idx += kCrThreads) {
            const int q = 4 * (idx / 9) + 1, r = idx % 9;
            if (q < n0) {
                const double* P = V.csol2 + (rb + q) * 171;
                double x = P[162 + r];
                if (q >= 3) {
                    const double* xm = smem + (size_t)((q - 2) >> 2) * 252 + 243;
#pragma unroll
                    for (int k = 0; k < 9; ++k) x -= P[r * 9 + k] * xm[k];
                }
                if (q + 2 < n0) {
                    const double* xp = smem + (size_t)((q + 2) >> 2) * 252 + 243;
#pragma unroll
                    for (int k = 0; k < 9; ++k) x -= P[81 + r * 9 + k] * xp[k];
                }
                x1[(size_t)(q >> 2) * 9 + r] = x;
            }
        }
        __syncthreads();
        VBA_KSTAMP(tson, tsi++);
        for (int idx = tid; idx < n0 * 9; idx += kCrThreads) {
            const int q = idx / 9, r = idx % 9;
            double x;
            if (q & 1) {
                x = x_odd(q)[r];
            } else {
                const double* P = V.csol2 + (rb + q) * 171;
                x = P[162 + r];
                if (q >= 1) {
                    const double* xm = x_odd(q - 1);
#pragma unroll
                    for (int k = 0; k < 9; ++k) x -= P[r * 9 + k] * xm[k];
                }
                if (q + 1 < n0) {
                    const double* xp = x_odd(q + 1);
#pragma unroll
                    for (int k = 0; k < 9; ++k) x -= P[81 + r * 9 + k] * xp[k];
                }
            }
            V.rx[rb * 9 + idx] = x;
        }
    } else if (!PRE) {
        for (int idx = tid; idx < n1 * 9; idx += kCrThreads) V.rx[rb * 9 + idx] = smem[(size_t)(idx / 9) * 252 + 243 + idx % 9];
    } else {
        // separators 2t+1 are the blocks solved here; 2t come from the level-0 eliminations:
        //   x_{2t} = Pg - PL x_{2t-1} - PU x_{2t+1}
        for (int idx = tid; idx < n0 * 9; idx += kCrThreads) {
            const int q = idx / 9, r = idx % 9;
            double x;
            if (q & 1) {
                x = smem[(size_t)(q >> 1) * 252 + 243 + r];
            } else {
                const double* P = V.csol2 + (rb + q) * 171;
                x = P[162 + r];
                if (q >= 1) {
                    const double* xm = smem + (size_t)((q - 1) >> 1) * 252 + 243;
#pragma unroll
                    for (int k = 0; k < 9; ++k) x -= P[r * 9 + k] * xm[k];
                }
                if (q + 1 < n0) {
                    const double* xp = smem + (size_t)((q + 1) >> 1) * 252 + 243;
#pragma unroll
                    for (int k = 0; k < 9; ++k) x -= P[81 + r * 9 + k] * xp[k];
                }
            }
            V.rx[rb * 9 + idx] = x;
        }
    }
    VBA_KSTAMP(tson, tsi++);
    (void)tsi; (void)tson;
    report_pivot<PIVOT>(bad, sc, lane, V.par);
}

template <bool PIVOT, int PRE>
__global__ __launch_bounds__(kCrThreads) void k_solve_reduced_cr(DevView V, int s) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    reduced_cr_body<PIVOT, PRE, kCrThreads>(V, s, blockIdx.x, smem);
}

// dynamic LDS of k_solve_reduced_cr<., 2> for n0 separators: the n0 / 4 blocks it solves and the level-1 solutions behind them
constexpr size_t cr_tail2_lds_bytes(int n0) { return ((size_t)(n0 / 4) * 252 + (size_t)((n0 + 3) / 4) * 9) * sizeof(double); }
// ... and the limits: kCrMax blocks; with two levels in front up to 4 kCrMax separators, so 65 level-1 solutions
constexpr int kCrLdsCap = kCrMax * 252 * (int)sizeof(double);
constexpr int kCrTail2LdsCap = kCrLdsCap + 65 * 9 * 8;

}  // namespace vba
