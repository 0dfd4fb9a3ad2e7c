// vba_solve_chunk_body.h -- device bodies of the partitioned solve: the chunk eliminations (one wave, or two waves that meet in
// the middle), the block source of the reduced system, and the forming two-sided chunk kernel's body.  Included by
// vba_solve_chunks.hip (the kernels) and by the comparison unit, whose resident solve runs the same bodies.
#pragma once

#include "vba_asm.h"
#include "vba_asm_fast.h"
#include "vba_solve_step.h"
#include "vba_solve_units.h"

namespace vba {

// ================================================================================================== partitioned
// chunk c of a window covers blocks [c s, min((c+1) s, n)); its last block is a separator unless c is the last
// chunk.  s >= 2, so every chunk has at least one interior block.
__device__ __forceinline__ void chunk_range(int c, int s, int n, int& a, int& b, bool& has_sep) {
    a = c * s;
    const int end = min((c + 1) * s, n);        // exclusive
    has_sep = end < n;
    b = has_sep ? end - 2 : end - 1;            // last interior block
}

// Reduced system over the separators of a chain given by `Inner`: row q couples separators q-1, q, q+1 (block
// j = (q+1) s - 1 of the inner chain):
//   sub = -L_j Vhat_{j-1},  diag = D_j - L_j What_{j-1} - U_j Vhat_{j+1},  super = -U_j What_{j+1},
//   rhs = g_j - L_j yhat_{j-1} - U_j yhat_{j+1};   the products were left in cL / cR by the chunk waves.
// It is again a block source, so the same chunk elimination can be applied to it (second level).
template <class Inner>
struct ReducedSource {
    Inner inner;
    const double* cL;       // [ns][9][19]
    const double* cR;
    int s;
    __device__ double operator()(int q, int e) const {
        const int j = (q + 1) * s - 1;
        const double* l = cL + (size_t)q * 171;         // [row][19 columns]: row-major like the bands, so that a
        const double* r_ = cR + (size_t)q * 171;        // consumer walking e reads runs of 9 contiguous doubles
        if (e >= 243) {
            const int r = e - 243;
            return inner(j, e) - l[r * 19] - r_[r * 19];
        }
        const int which = e / 81, r = (e % 81) / 9, cc = e % 9;
        if (which == 0) return -l[r * 19 + 1 + cc];
        if (which == 2) return -r_[r * 19 + 10 + cc];
        return inner(j, e) - l[r * 19 + 10 + cc] - r_[r * 19 + 1 + cc];
    }
};

// Eliminates the interior of chunk c of a chain of n blocks with 19 right-hand sides: column 0 = g, 1..9 = L_a
// (coupling to the left separator), 10..18 = U_b (coupling to the right separator).  csol[i][col][r] receives
// T^{-1} of them for every interior block i; cL[c] / cR[c-1] receive L_j / U_j times the solutions next to the
// chunk's two separators (what the reduced system needs).
template <bool PIVOT, bool SPARSE_L, class Src>
__device__ __forceinline__ void chunk_eliminate(const Src& src, int n, int s, int c, double lam32, double* csol, double* cL,
                                                double* cR, double* smem, int lane, bool& zero_pivot) {
    int a0, b0;
    bool has_sep;
    chunk_range(c, s, n, a0, b0, has_sep);
    const int len = b0 - a0 + 1;
    double (*blk)[256] = reinterpret_cast<double (*)[256]>(smem);           // [2][256]
    double* Xb = smem + 512;                                                 // [s][81]
    double* Zb = Xb + (size_t)s * 81;                                        // [s][19][9]
    double* Cm = Zb + (size_t)s * 171;                                       // [2][81]: L of the right separator, U of the left one
    {   // (the loads of a lane before its first store)
        double cm[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int e = lane + 64 * q;
            double v = 0.0;
            if (e < 81) { if (has_sep) v = src(b0 + 1, e); }
            else if (e < 162 && c > 0) v = src(a0 - 1, 162 + (e - 81));
            cm[q] = v;
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int e = lane + 64 * q;
            if (e < 162) Cm[e] = cm[q];
        }
    }
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
    // lanes: D/U groups in 0..17 (alternating), V = 18..26, W = 27..35, y = 36  -> rhs column order in Zb: y, V, W
    const bool isV = lane >= 18 && lane < 27, isW = lane >= 27 && lane < 36, isY = lane == 36;
    const int zcol = isY ? 0 : (isV ? 1 + (lane - 18) : (isW ? 10 + (lane - 27) : 0));
    // one LDS address per lane and role (selecting among loaded values would make every lane load all five)
    auto load_base = [&](const double* b, int db, bool first, bool last, double (&base)[9]) {
        const int ub = 9 - db;
        const bool isD = lane >= db && lane < db + 9, isU = lane >= ub && lane < ub + 9;
        const int cc = isD ? lane - db : (isU ? lane - ub : (isV ? lane - 18 : (isW ? lane - 27 : 0)));
        const bool ok = isD || isU || isY || (isV && first) || (isW && last);
        const int off = isD ? 81 + cc : ((isU || isW) ? 162 + cc : (isY ? 243 : cc));
        const int stride = isY ? 1 : 9;
        const double* p = b + (ok ? off : 0);
#pragma unroll
        for (int r = 0; r < 9; ++r) {
            double v = p[r * stride];
            v = ok ? v : 0.0;
            if (isD && r == cc) v += lam32;
            base[r] = v;
        }
    };
    fetch(a0);
    stash(0);
    __syncthreads();
    for (int t = 0; t < len; ++t) {
        const int buf = t & 1;
        if (t + 1 < len) fetch(a0 + t + 1);
        double base[9];
        if (buf == 0) {
            load_base(blk[0], 0, t == 0, t == len - 1, base);
            forward_step<0, 19, PIVOT, SPARSE_L>(t > 0 ? blk[0] : nullptr, base, a, lane, zero_pivot);
        } else {
            load_base(blk[1], 9, false, t == len - 1, base);
            forward_step<9, 19, PIVOT, SPARSE_L>(blk[1], base, a, lane, zero_pivot);
        }
        const int ub = buf == 0 ? 9 : 0;
        if (lane >= ub && lane < ub + 9) {
#pragma unroll
            for (int r = 0; r < 9; ++r) Xb[(size_t)t * 81 + r * 9 + (lane - ub)] = a[r];
        } else if (isV || isW || isY) {
#pragma unroll
            for (int r = 0; r < 9; ++r) Zb[((size_t)t * 19 + zcol) * 9 + r] = a[r];
        }
        if (t + 1 < len) stash(buf ^ 1);
        __syncthreads();
    }
    // Backward sweep for the 19 right-hand sides on the matrix cores: x_t (9 x 19) = Z_t - X_t x_{t+1}.
    // v_mfma_f64_16x16x4 leaves C[(l >> 4) + 4 i][l & 15] in register i of lane l, and wants B[4 s + (l >> 4)][l & 15] in
    // k-step s: register s of the previous result IS the B operand of k-step s, so x never moves between steps.  Two
    // column tiles (columns 0..15, 16..18), three k-steps (rows 9..11 of x stay zero), one LDS read per A element.
    const int lr = lane & 15, lk = lane >> 4;
    auto load_Z = [&](int t, int tile) {
        vf4 z;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = lk + 4 * i, col = 16 * tile + lr;
            const bool ok = row < 9 && col < 19;
            const double v = Zb[ok ? ((size_t)t * 19 + col) * 9 + row : 0];
            z[i] = ok ? v : 0.0;
        }
        return z;
    };
    auto mul_sub = [&](const double* M, double sign, vf4& acc0, vf4& acc1, const vf4& b0, const vf4& b1) {
        // acc += sign * M (9 x 9, row major in LDS) * b
#pragma unroll
        for (int st = 0; st < 3; ++st) {
            const int k = 4 * st + lk;
            const bool ok = lr < 9 && k < 9;
            const double m = M[ok ? lr * 9 + k : 0];
            const double am = ok ? sign * m : 0.0;
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(am, b0[st], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(am, b1[st], acc1, 0, 0, 0);
        }
    };
    auto store_cols = [&](double* dst, size_t col_stride, size_t row_stride, const vf4& v0, const vf4& v1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = lk + 4 * i;
            if (row < 9) {
                dst[(size_t)lr * col_stride + (size_t)row * row_stride] = v0[i];
                if (lr < 3) dst[(size_t)(16 + lr) * col_stride + (size_t)row * row_stride] = v1[i];
            }
        }
    };
    double* out = csol + (size_t)a0 * 171;
    vf4 x0 = load_Z(len - 1, 0), x1 = load_Z(len - 1, 1);
    store_cols(out + (size_t)(len - 1) * 171, 9, 1, x0, x1);
    // contribution of this chunk to its right separator j = b+1:  L_j [yhat_b | Vhat_b | What_b]   ([row][19 columns])
    if (has_sep) {
        vf4 p0 = {0.0, 0.0, 0.0, 0.0}, p1 = {0.0, 0.0, 0.0, 0.0};
        mul_sub(Cm, 1.0, p0, p1, x0, x1);
        store_cols(cL + (size_t)c * 171, 1, 19, p0, p1);
    }
    for (int t = len - 2; t >= 0; --t) {
        vf4 n0 = load_Z(t, 0), n1 = load_Z(t, 1);
        mul_sub(Xb + (size_t)t * 81, -1.0, n0, n1, x0, x1);
        x0 = n0;
        x1 = n1;
        store_cols(out + (size_t)t * 171, 9, 1, x0, x1);
    }
    // contribution to the left separator j = a-1:  U_j [yhat_a | Vhat_a | What_a]
    if (c > 0) {
        vf4 p0 = {0.0, 0.0, 0.0, 0.0}, p1 = {0.0, 0.0, 0.0, 0.0};
        mul_sub(Cm + 81, 1.0, p0, p1, x0, x1);
        store_cols(cR + (size_t)(c - 1) * 171, 1, 19, p0, p1);
    }
}

// The same elimination by TWO waves per chunk that meet in the middle.  The elimination of a chunk is a chain of dependent
// block steps (~2 us each on a single wave) and in latency mode that chain IS the time of the kernel: wave 0 eliminates
// blocks a .. m-1 left to right, wave 1 blocks b .. m+1 right to left -- the same step on the mirrored chain (sub and super
// diagonal swap roles; the coupling to the right separator enters at its first block the way the left one enters wave 0's)
// -- then wave 0 solves block m with both neighbours folded in,
//     (D_m - L_m X_{m-1} - U_m X'_{m+1}) x_m = g_m - L_m z_{m-1} - U_m z'_{m+1}      (19 right-hand sides),
// and both waves substitute outwards from x_m on the matrix cores.  Half the dependent steps (7 interior blocks: 3 + 1
// + the two substitutions side by side instead of 7 + 6).  Chunks with fewer than 3 interior blocks take the one-wave
// path.  tid: 0 .. 127.
__host__ __device__ constexpr int twosided_half(int s) { return (s + 1) / 2; }
__host__ __device__ constexpr int twosided_region(int s) { return 512 + twosided_half(s) * (81 + 171); }
__host__ __device__ constexpr int twosided_lds_doubles(int s) {
    const int two = 2 * twosided_region(s) + 162 + 256 + 171, one = 512 + s * 252 + 162;
    return two > one ? two : one;
}

template <bool PIVOT, bool SPARSE_L, class Src>
__device__ __forceinline__ void chunk_eliminate_twosided(const Src& src, int n, int s, int c, double lam32, double* csol, double* cL,
                                                         double* cR, double* smem, int tid, bool& zero_pivot) {
    int a0, b0;
    bool has_sep;
    chunk_range(c, s, n, a0, b0, has_sep);
    const int len = b0 - a0 + 1;
    const int side = tid >> 6, lane = tid & 63;
    if (len < 3) {      // (uniform over the workgroup) nothing to share: one wave, the other leaves
        if (side == 0) chunk_eliminate<PIVOT, SPARSE_L>(src, n, s, c, lam32, csol, cL, cR, smem, lane, zero_pivot);
        return;
    }
    const int lenL = len / 2, lenR = len - 1 - lenL, m = a0 + lenL;
    const int lenS = side ? lenR : lenL;
    const int hs = twosided_half(s), RS = twosided_region(s);
    double* reg0 = smem;
    double* reg1 = smem + RS;
    double* reg = side ? reg1 : reg0;
    double (*blk)[256] = reinterpret_cast<double (*)[256]>(reg);            // [2][256]
    double* Xb = reg + 512;                                                  // [hs][81]
    double* Zb = Xb + (size_t)hs * 81;                                       // [hs][19][9]
    double* Cm = smem + 2 * (size_t)RS;                                      // [2][81]: L of the right separator, U of the left one
    double* blkM = Cm + 162;                                                 // block m
    double* xm = blkM + 256;                                                 // [19][9] its solution
    // entry e of real block i as this side's sweep sees it
    auto entry = [&](int i, int e) {
        const int ee = side ? (e < 81 ? e + 162 : ((e >= 162 && e < 243) ? e - 162 : e)) : e;
        return src(i, ee);
    };
    auto block_of = [&](int t) { return side ? b0 - t : a0 + t; };
    {   // (both loads of a lane before its first store)
        double cm[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int e = lane + 64 * q;
            cm[q] = e >= 81 ? 0.0 : (side ? (has_sep ? src(b0 + 1, e) : 0.0) : (c > 0 ? src(a0 - 1, 162 + e) : 0.0));
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int e = lane + 64 * q;
            if (e < 81) Cm[side ? e : 81 + e] = cm[q];
        }
    }
    double mid[4] = {0.0, 0.0, 0.0, 0.0};
    if (side == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = lane + 64 * q;
            mid[q] = e < 252 ? src(m, e) : 0.0;
        }
    }
    double a[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) a[j] = 0.0;
    double pre[4];
    auto fetch = [&](int t) {
        const int i = block_of(t);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = lane + 64 * q;
            pre[q] = e < 252 ? entry(i, e) : 0.0;
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int q = 0; q < 4; ++q) blk[buf][lane + 64 * q] = pre[q];
    };
    // lanes as in chunk_eliminate: D/U groups in 0..17 (alternating), V = 18..26, W = 27..35, y = 36.  "V" is the coupling
    // that enters at the sweep's FIRST block: the left separator for wave 0, the right one for wave 1 (columns swapped
    // back when the results are stored); the W columns stay zero during the sweeps.
    const bool isV = lane >= 18 && lane < 27, isW = lane >= 27 && lane < 36, isY = lane == 36;
    const int zcol = isY ? 0 : (isV ? 1 + (lane - 18) : (isW ? 10 + (lane - 27) : 0));
    auto load_base = [&](const double* b, int db, bool first, double (&base)[9]) {
        const int ub = 9 - db;
        const bool isD = lane >= db && lane < db + 9, isU = lane >= ub && lane < ub + 9;
        const int cc = isD ? lane - db : (isU ? lane - ub : (isV ? lane - 18 : 0));
        const bool ok = isD || isU || isY || (isV && first);
        const int off = isD ? 81 + cc : (isU ? 162 + cc : (isY ? 243 : cc));
        const int stride = isY ? 1 : 9;
        const double* p = b + (ok ? off : 0);
#pragma unroll
        for (int r = 0; r < 9; ++r) {
            double v = p[r * stride];
            v = ok ? v : 0.0;
            if (isD && r == cc) v += lam32;
            base[r] = v;
        }
    };
    // Row layout of the unpivoted path (cr_pivots_dpp): every row of 16 lanes holds D' in lanes 0..8 (the same values in
    // all four rows) and seven of the 28 columns [U | y V W] in lanes 9..15; a pivot broadcasts inside the row (DPP).  What
    // the alternating lane groups of forward_step got for free -- X_{t-1}'s column c already sitting in the lane that forms
    // D'_t's column c -- comes from Xb in LDS here (written for the outward substitution anyway).
#ifndef VBA_CHUNK_READLANE
    constexpr bool kRows = !PIVOT;
#else
    constexpr bool kRows = false;
#endif
    const int rrow = lane >> 4, rc = lane & 15;
    const int ro = rrow * 7 + (rc - 9);                 // column of [U | y V W] of a lane with rc >= 9
    const bool rD = rc < 9, rU = !rD && ro < 9, rR = !rD && ro >= 9;
    const int rz = rR ? ro - 9 : 0;                     // column of Zb: 0 = y, 1..9 = V, 10..18 = W
    auto rows_step = [&](const double* b, const double* Lmat, const double* Xprev, bool first) {
        // base: this lane's column of [D + lam I | U | y | V (first block only)]
        const bool ok = rD || rU || (rR && (rz == 0 || (first && rz < 10)));
        const int off = rD ? 81 + rc : (rU ? 162 + ro : (rz == 0 ? 243 : rz - 1));
        const int stride = (rR && rz == 0) ? 1 : 9;
        const double* p = b + (ok ? off : 0);
        double base[9], xp[9];
#pragma unroll
        for (int r = 0; r < 9; ++r) {
            double v = p[r * stride];
            v = ok ? v : 0.0;
            if (rD && r == rc) v += lam32;
            base[r] = v;
        }
        if (Lmat) {
            // carried column: X_{t-1}[:, c] for the D lanes (from LDS), this lane's own z_{t-1} for the right-hand sides
            const double* xs = Xprev + (rD ? rc : 0);
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                const double xv = xs[j * 9];
                xp[j] = rD ? xv : (rR ? a[j] : 0.0);
            }
#pragma unroll
            for (int r = 0; r < 9; ++r) {
                double v = base[r];
#pragma unroll
                for (int j = 0; j < 9; ++j) {
                    const bool rot_r = (r >= 3 && r < 6), rot_j = (j >= 3 && j < 6);
                    if (!SPARSE_L || rot_r == rot_j) v = fma(-Lmat[r * 9 + j], xp[j], v);
                }
                a[r] = v;
            }
        } else {
#pragma unroll
            for (int r = 0; r < 9; ++r) a[r] = base[r];
        }
        bool mybad = false;
        cr_pivots_dpp<0>(base, a, rc, mybad);
        zero_pivot = zero_pivot | (rD & mybad);
    };
    fetch(0);
    stash(0);
    wave_sync_lds();
    for (int t = 0; t < lenS; ++t) {
        const int buf = t & 1;
        if (t + 1 < lenS) fetch(t + 1);
        if constexpr (kRows) {
            rows_step(blk[buf], t > 0 ? blk[buf] : nullptr, Xb + (size_t)(t > 0 ? t - 1 : 0) * 81, t == 0);
            if (rU) {
#pragma unroll
                for (int r = 0; r < 9; ++r) Xb[(size_t)t * 81 + r * 9 + ro] = a[r];
            } else if (rR) {
#pragma unroll
                for (int r = 0; r < 9; ++r) Zb[((size_t)t * 19 + rz) * 9 + r] = a[r];
            }
            if (t + 1 < lenS) stash(buf ^ 1);
            wave_sync_lds();
            VBA_KSTAMP(tid == 0 && c == 30, 35 + t);
            continue;
        }
        double base[9];
        if (buf == 0) {
            load_base(blk[0], 0, t == 0, base);
            forward_step<0, 19, PIVOT, SPARSE_L>(t > 0 ? blk[0] : nullptr, base, a, lane, zero_pivot);
        } else {
            load_base(blk[1], 9, false, base);
            forward_step<9, 19, PIVOT, SPARSE_L>(blk[1], base, a, lane, zero_pivot);
        }
        const int ub = buf == 0 ? 9 : 0;
        if (lane >= ub && lane < ub + 9) {
#pragma unroll
            for (int r = 0; r < 9; ++r) Xb[(size_t)t * 81 + r * 9 + (lane - ub)] = a[r];
        } else if (isV || isW || isY) {
#pragma unroll
            for (int r = 0; r < 9; ++r) Zb[((size_t)t * 19 + zcol) * 9 + r] = a[r];
        }
        if (t + 1 < lenS) stash(buf ^ 1);
        wave_sync_lds();
    }
    if (side == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) blkM[lane + 64 * q] = mid[q];
    }
    __syncthreads();
    VBA_KSTAMP(tid == 0 && c == 30, 40);
    // block m: both neighbours folded in, then the same Gauss-Jordan step on [M | 19 right-hand sides]
    if (kRows && side == 0) {
        const double* XL = reg0 + 512 + (size_t)(lenL - 1) * 81;
        const double* ZL = reg0 + 512 + (size_t)hs * 81 + (size_t)(lenL - 1) * 171;
        const double* XR = reg1 + 512 + (size_t)(lenR - 1) * 81;
        const double* ZR = reg1 + 512 + (size_t)hs * 81 + (size_t)(lenR - 1) * 171;
        // column of the left / right sweep's results this lane folds in (wave 1 keeps the right coupling in ITS columns 1..9)
        const int cl = rz, cr = rz == 0 ? 0 : (rz < 10 ? rz + 9 : rz - 9);
        const double* pl = rD ? XL + rc : ZL + (size_t)(rR ? cl : 0) * 9;
        const double* pr = rD ? XR + rc : ZR + (size_t)(rR ? cr : 0) * 9;
        const int st = rD ? 9 : 1;
        double base[9];
#pragma unroll
        for (int r = 0; r < 9; ++r) {
            double v = 0.0;
            const double dv = blkM[81 + r * 9 + (rD ? rc : 0)], yv = blkM[243 + r];
            if (rD) v = dv + (r == rc ? lam32 : 0.0);
            else if (rR && rz == 0) v = yv;
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                const bool rot_r = (r >= 3 && r < 6), rot_j = (j >= 3 && j < 6);
                if (!SPARSE_L || rot_r == rot_j) {
                    v -= blkM[r * 9 + j] * pl[j * st];
                    v -= blkM[162 + r * 9 + j] * pr[j * st];
                }
            }
            base[r] = (rD || rR) ? v : 0.0;
            a[r] = base[r];
        }
        bool mybad = false;
        cr_pivots_dpp<0>(base, a, rc, mybad);
        zero_pivot = zero_pivot | (rD & mybad);
        if (rR) {
#pragma unroll
            for (int r = 0; r < 9; ++r) xm[(size_t)rz * 9 + r] = a[r];
        }
    } else if (side == 0) {
        const double* XL = reg0 + 512 + (size_t)(lenL - 1) * 81;
        const double* ZL = reg0 + 512 + (size_t)hs * 81 + (size_t)(lenL - 1) * 171;
        const double* XR = reg1 + 512 + (size_t)(lenR - 1) * 81;
        const double* ZR = reg1 + 512 + (size_t)hs * 81 + (size_t)(lenR - 1) * 171;
        const bool isD = lane < 9, isR = isV || isW || isY;
        // column of the left / right sweep's results this lane folds in (wave 1 keeps the right coupling in ITS columns 1..9)
        const int cl = isY ? 0 : (isV ? 1 + (lane - 18) : (isW ? 10 + (lane - 27) : 0));
        const int cr = isY ? 0 : (isV ? 10 + (lane - 18) : (isW ? 1 + (lane - 27) : 0));
        const double* pl = isD ? XL + lane : ZL + (size_t)cl * 9;
        const double* pr = isD ? XR + lane : ZR + (size_t)cr * 9;
        const int st = isD ? 9 : 1;
        double base[9];
#pragma unroll
        for (int r = 0; r < 9; ++r) {
            double v = 0.0;
            if (isD) v = blkM[81 + r * 9 + lane] + (r == lane ? lam32 : 0.0);
            else if (isY) v = blkM[243 + r];
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                const bool rot_r = (r >= 3 && r < 6), rot_j = (j >= 3 && j < 6);
                if (!SPARSE_L || rot_r == rot_j) {
                    v -= blkM[r * 9 + j] * pl[j * st];
                    v -= blkM[162 + r * 9 + j] * pr[j * st];
                }
            }
            base[r] = (isD || isR) ? v : 0.0;
        }
        forward_step<0, 19, PIVOT, SPARSE_L>(nullptr, base, a, lane, zero_pivot);
        if (isR) {
#pragma unroll
            for (int r = 0; r < 9; ++r) xm[(size_t)zcol * 9 + r] = a[r];
        }
    }
    __syncthreads();
    VBA_KSTAMP(tid == 0 && c == 30, 41);
    // outward substitution on the matrix cores (see chunk_eliminate): x_t = Z_t - X_t x_{t+1}
    const int lr = lane & 15, lk = lane >> 4;
    auto colperm = [&](int col) { return side ? (col == 0 ? 0 : (col < 10 ? col + 9 : col - 9)) : col; };
    auto load_cols = [&](const double* Z, int tile, bool perm) {
        vf4 z;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = lk + 4 * i, col = 16 * tile + lr;
            const bool ok = row < 9 && col < 19;
            const double v = Z[ok ? (size_t)(perm ? colperm(col) : col) * 9 + row : 0];
            z[i] = ok ? v : 0.0;
        }
        return z;
    };
    auto mul_sub = [&](const double* M, double sign, vf4& acc0, vf4& acc1, const vf4& b0v, const vf4& b1v) {
#pragma unroll
        for (int st = 0; st < 3; ++st) {
            const int k = 4 * st + lk;
            const bool ok = lr < 9 && k < 9;
            const double mm = M[ok ? lr * 9 + k : 0];
            const double am = ok ? sign * mm : 0.0;
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(am, b0v[st], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(am, b1v[st], acc1, 0, 0, 0);
        }
    };
    // the real column a value of this side's column `col` belongs to
    // (every lane stores every time: one without an entry repeats its own first one -- row lk < 4 of the first tile always
    // exists -- instead of opening a branch region per store)
    auto store_cols = [&](double* dst, size_t col_stride, size_t row_stride, const vf4& v0, const vf4& v1) {
        const size_t c0 = (size_t)colperm(lr) * col_stride, c1 = (size_t)colperm(lr < 3 ? 16 + lr : 0) * col_stride;
        const size_t home = c0 + (size_t)lk * row_stride;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = lk + 4 * i;
            const bool ok0 = row < 9, ok1 = ok0 && lr < 3;
            dst[ok0 ? c0 + (size_t)row * row_stride : home] = ok0 ? v0[i] : v0[0];
            dst[ok1 ? c1 + (size_t)row * row_stride : home] = ok1 ? v1[i] : v0[0];
        }
    };
    vf4 x0 = load_cols(xm, 0, true), x1 = load_cols(xm, 1, true);
    if (side == 0) store_cols(csol + (size_t)m * 171, 9, 1, x0, x1);
    for (int t = lenS - 1; t >= 0; --t) {
        vf4 n0 = load_cols(Zb + (size_t)t * 171, 0, false), n1 = load_cols(Zb + (size_t)t * 171, 1, false);
        mul_sub(Xb + (size_t)t * 81, -1.0, n0, n1, x0, x1);
        x0 = n0;
        x1 = n1;
        store_cols(csol + (size_t)block_of(t) * 171, 9, 1, x0, x1);
    }
    VBA_KSTAMP(tid == 0 && c == 30, 42);
    // x is now the solution next to this side's separator: its contribution to that row of the reduced system
    if (side == 0 ? c > 0 : has_sep) {
        vf4 p0 = {0.0, 0.0, 0.0, 0.0}, p1 = {0.0, 0.0, 0.0, 0.0};
        mul_sub(side ? Cm : Cm + 81, 1.0, p0, p1, x0, x1);
        store_cols(side ? cL + (size_t)c * 171 : cR + (size_t)(c - 1) * 171, 1, 19, p0, p1);
    }
}

// blocks formed in LDS by the kernel itself (k_solve_chunks_fused, chunks_ts_fused_body)
struct LdsBlockSource {
    const double* blocks;   // [count][252]
    int first;              // pose index of blocks[0]
    __device__ double operator()(int i, int e) const { return blocks[(size_t)(i - first) * 252 + e]; }
};

// scratch of the one-wave elimination (chunk_eliminate), and with the blocks and staged inputs of k_solve_chunks_fused
__host__ __device__ constexpr int chunk_lds_doubles(int s) { return 512 + s * 252 + 162; }
__host__ __device__ constexpr int chunk_fused_lds_doubles(int s, bool reg) {
    return chunk_lds_doubles(s) + (s + 1) * 252 + (s + 2) * (kAsmBase + (reg ? kAsmPrior : 0));
}

// The same with the two-sided elimination and the uniform-pass row former (vba_asm_fast.h): the four waves of the block form
// the chunk's (at most s + 1) blocks in LDS -- one wave per pose row, seven uniform passes -- then waves 0 and 1 eliminate
// from both ends.  No assembly launch in the full phase of the latency mode.
__host__ __device__ constexpr int twosided_fused_lds_doubles(int s, bool reg) {
    return twosided_lds_doubles(s) + (s + 1) * 252 + (s + 2) * (kAsmBase + (reg ? kAsmPrior : 0));
}

template <bool PIVOT, bool REG>
__device__ __forceinline__ void chunks_ts_fused_body(const DevView& V, int s, int w, int c, double* smem) {
    constexpr int kAsmIn = kAsmBase + (REG ? kAsmPrior : 0);
    VBA_SKIP_CALL(V, w);
    WinScalars& sc = V.sc[w];
    if (sc.done || !solver_mine<PIVOT>(V, sc)) return;
    const int n = V.n[w];
    if (c * s >= n) return;
    const int tid = threadIdx.x;
    VBA_KSTAMP(tid == 0 && c == 30, 32);
    const size_t sb = (size_t)w * V.n_max;
    const size_t rb = (size_t)w * V.p_max;
    const double lam32 = (double)(float)sc.lam[V.par];
    // (requested here, in front of the staging: behind the barrier below this load would be a round trip to memory of its own)
    const unsigned long long wmax_bits = sc.wmax_bits[V.par];
    if (c == 0 && tid == 0) {
        sc.lam32 = lam32;
        if (PIVOT) atomicAnd(&sc.fl[V.par], ~8u);
    }
    int a0, b0;
    bool has_sep;
    chunk_range(c, s, n, a0, b0, has_sep);
    const int j0 = a0 > 0 ? a0 - 1 : 0, j1 = has_sep ? b0 + 1 : b0;         // blocks formed here
    const int nblk = j1 - j0 + 1;
    double* elim = smem;                                                     // scratch of the elimination
    double* blocks = smem + twosided_lds_doubles(s);                         // [s + 1][252]
    double* in = blocks + (size_t)(s + 1) * 252;                             // [s + 2][kAsmIn]: poses j0 - 1 .. j1
    // staging: four loads per thread in flight at a time (the address is selected, never the load: vba_asm.h)
    {
        const int total = (nblk + 1) * kAsmIn;
        for (int e0 = 0; e0 < total; e0 += 4 * 256) {
            double v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int e = e0 + tid + 256 * k;
                const int slot = e / kAsmIn, q = e - slot * kAsmIn;
                const int i = j0 - 1 + slot;
                const bool ok = e < total && i >= 0 && i < n;
                v[k] = asm_input_nobranch<REG>(V, sb + (ok ? i : 0), ok ? q : 0);
                v[k] = ok ? v[k] : 0.0;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int e = e0 + tid + 256 * k;
                if (e < total) in[e] = v[k];
            }
        }
    }
    __syncthreads();
    VBA_KSTAMP(tid == 0 && c == 30, 33);
    const double inv_wmax = 1.0 / bits_f64(wmax_bits);
    {
        // formation by column: a row of 16 lanes per pose row, sixteen pose rows per pass of the workgroup
        const int lane = tid & 63, wave = tid >> 6, row = lane >> 4, cc = lane & 15;
        const AsmColLane cl = asm_col_lane(cc);
        for (int q0 = 0; q0 < nblk; q0 += 16) {
            const int q = q0 + wave * 4 + row;
            const bool have = q < nblk;
            const int qq = have ? q : 0;
            const int i = j0 + qq;
            double* blk = blocks + (size_t)qq * 252;
            const bool sep = have && has_sep && i == j1, last = have && i == n - 1;
            double A[9], B[9], Lc[9];
            VBA_KSTAMP(tid == 0 && c == 30, 48);
            asm_form_columns<REG>(cl, cc, in + (size_t)(qq + 1) * kAsmIn, in + (size_t)qq * kAsmIn, true, i < n - 1, i > 0, V.prm.sigma, inv_wmax, A, B, Lc);
#ifdef VBA_RESIDENT_STAMPS
            if (tid == 0 && c == 30) g_kstamps[49] = (unsigned long long)(A[0] + A[8] + B[4] + Lc[7] != 12345.0);
            VBA_KSTAMP(tid == 0 && c == 30, 50);
#endif
            {
                // one destination and one predicate per lane and array, decided once (as nested branches inside the unrolled
                // loop this was some forty basic blocks).  What later kernels read from memory: the right separator's
                // diagonal block and right-hand side (reduced system), the last pose's diagonal block (last_hessian)
                const bool isc = have && cc < 9, isr = have && cc == 9;
                double* pA = blk + (cc < 9 ? 81 + cc : 243);
                const int stA = cc < 9 ? 9 : 1;
                double* gS = cc < 9 ? V.bands + (sb + i) * 243 + 81 + cc : V.rhs + (sb + i) * 9;
                double* gL = V.lastD + (size_t)w * 81 + (cc < 9 ? cc : 0);
                const bool wS = sep && (isc || isr), wL = last && isc;
                // LDS: every lane stores, the lanes without a column into a dump word of the elimination's scratch (idle until
                // the barrier below) -- a predicated store inside the unrolled loop is a branch region of its own, and
                // forty-five of them cost more than the formation itself (1.3 against 0.6 us)
                double* dump = elim + (tid & 63);
                double* pL = isc ? blk + cc : dump;
                double* pD = (isc || isr) ? pA : dump;
                double* pU = isc ? blk + 162 + cc : dump;
                const int sC = isc ? 9 : 0, sD = (isc || isr) ? stA : 0;
#pragma unroll
                for (int a9 = 0; a9 < 9; ++a9) {
                    pL[a9 * sC] = Lc[a9];
                    pD[a9 * sD] = A[a9];
                    pU[a9 * sC] = B[a9];
                }
                if (wS) {
#pragma unroll
                    for (int a9 = 0; a9 < 9; ++a9) gS[a9 * stA] = A[a9];
                }
                if (wL) {
#pragma unroll
                    for (int a9 = 0; a9 < 9; ++a9) gL[a9 * 9] = A[a9];
                }
            }
            VBA_KSTAMP(tid == 0 && c == 30, 51);
        }
    }
    __syncthreads();
    VBA_KSTAMP(tid == 0 && c == 30, 34);
    if (tid >= 128) return;     // the elimination is two waves' work (its barriers count the surviving waves only)
    bool bad = false;
    const LdsBlockSource src{blocks, j0};
    chunk_eliminate_twosided<PIVOT, true>(src, n, s, c, lam32, V.csol + sb * 171, V.cL + rb * 171, V.cR + rb * 171, elim, tid, bad);
    VBA_KSTAMP(tid == 0 && c == 30, 47);
    report_pivot<PIVOT>(bad, sc, tid & 63, V.par);
}

}  // namespace vba
