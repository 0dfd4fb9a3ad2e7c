// vba_schur_rowpass.h -- what the row passes of the free-landmark queries share (k_rel_rows of vba_schur_rel.hip, k_pow_rows of
// vba_schur_power.hip): for a row of non-zero weight the gather of the pose-landmark cross-covariance from the blocks and Y the
// covariance query left resident, the row's Jacobians, and its 2x2 block P_k of the hat matrix.  The gather is the expensive part of
// a row (t products of 6x6 by 6x3 for a track of t rows); a query forms it once per row and continues from the registers.
// Arithmetic and its order are those k_rel_rows has always had: leverage and w-test keep their bits whichever kernel calls it.
#pragma once

#include "vba_schur_context.h"

// Row k (pose i, landmark l, position a in the track of l) after schur_row_blocks:
//   G = sum_{k' in rows(l)} (S^-1)_{i, pose(k')} Y_k' = -Sigma_il   (6x3, k' upwards; the block of the pair from lp_blk, which lists
//       k >= k' only: for k' > k the block of (k', k) is read transposed)
//   jc = A (2x6), jl = Al (2x3), Sii = Sigma_ii (6x6, stored whole and exactly symmetric), Sl = Sigma_ll (3x3)
//   P_k = w [A Al] [[Sigma_ii, Sigma_il], [Sigma_il^T, Sigma_ll]] [A Al]^T = [p00, p01; p01, p11]   (symmetric part)
struct SchurRowBlocks {
    double G[18], jl[6], jc[12];
    const double *Sii, *Sl;
    double p00, p01, p11;
};

__device__ __forceinline__ void schur_row_blocks(const SchurView& V, const double* pair, const int* lp_ptr, const int* lp_blk, const double* lm, int k,
                                                 const RowGeom& q, double w, SchurRowBlocks& b) {
    const int l = V.row_lm[k], beg = V.lm_ptr[l], end = V.lm_ptr[l + 1], a = k - beg, base = lp_ptr[l];
    double* G = b.G;
#pragma unroll
    for (int e = 0; e < 18; ++e) G[e] = 0.0;
    for (int k2 = beg; k2 < end; ++k2) {
        const int c = k2 - beg;
        const bool tr = c > a;
        const int slot = base + (tr ? c * (c + 1) / 2 + a : a * (a + 1) / 2 + c);
        const double* Sg = pair + (size_t)lp_blk[slot] * 36;
        const int sp = tr ? 1 : 6, sq = tr ? 6 : 1;    // entry (p, q) of (S^-1)_{i, pose(k')}: Sg[p sp + q sq]
        double Y2[18];
#pragma unroll
        for (int e = 0; e < 18; ++e) Y2[e] = V.Y[(size_t)k2 * 18 + e];
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            double g[6];
#pragma unroll
            for (int qq = 0; qq < 6; ++qq) g[qq] = Sg[p * sp + qq * sq];
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) {
                double s = G[3 * p + cc];
#pragma unroll
                for (int qq = 0; qq < 6; ++qq) s = fma(g[qq], Y2[3 * qq + cc], s);
                G[3 * p + cc] = s;
            }
        }
    }
    double* jl = b.jl;
    double* jc = b.jc;
    landmark_jacobian(q, jl);
    pose_jacobian(q, jl, jc);
    // A Sigma_ii A^T from the diagonal block of the row's own pair (k, k): stored whole and exactly symmetric
    const double* Sii = pair + (size_t)lp_blk[base + a * (a + 1) / 2 + a] * 36;
    double q00 = 0.0, q01 = 0.0, q11 = 0.0;
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        double tu = 0.0, tv = 0.0;
#pragma unroll
        for (int qq = 0; qq < 6; ++qq) { tu = fma(Sii[6 * p + qq], jc[qq], tu); tv = fma(Sii[6 * p + qq], jc[6 + qq], tv); }
        q00 = fma(jc[p], tu, q00);
        q01 = fma(jc[p], tv, q01);
        q11 = fma(jc[6 + p], tv, q11);
    }
    // A (-Sigma_il) Al^T: x = A G (2x3), then against the rows of Al
    double x00 = 0.0, x01 = 0.0, x10 = 0.0, x11 = 0.0;
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) {
        double xu = 0.0, xv = 0.0;
#pragma unroll
        for (int p = 0; p < 6; ++p) { xu = fma(jc[p], G[3 * p + cc], xu); xv = fma(jc[6 + p], G[3 * p + cc], xv); }
        x00 = fma(xu, jl[cc], x00);
        x01 = fma(xu, jl[3 + cc], x01);
        x10 = fma(xv, jl[cc], x10);
        x11 = fma(xv, jl[3 + cc], x11);
    }
    // Al Sigma_ll Al^T
    const double* Sl = lm + (size_t)l * 9;
    double l00 = 0.0, l01 = 0.0, l11 = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double yu = fma(Sl[3 * r], jl[0], fma(Sl[3 * r + 1], jl[1], Sl[3 * r + 2] * jl[2]));
        const double yv = fma(Sl[3 * r], jl[3], fma(Sl[3 * r + 1], jl[4], Sl[3 * r + 2] * jl[5]));
        l00 = fma(jl[r], yu, l00);
        l01 = fma(jl[r], yv, l01);
        l11 = fma(jl[3 + r], yv, l11);
    }
    b.Sii = Sii;
    b.Sl = Sl;
    b.p00 = w * ((q00 + l00) - (x00 + x00));
    b.p01 = w * ((q01 + l01) - (x01 + x10));
    b.p11 = w * ((q11 + l11) - (x11 + x11));
}
