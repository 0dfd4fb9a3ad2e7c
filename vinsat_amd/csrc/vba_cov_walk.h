// vba_cov_walk.h -- the block recurrence of the covariance query (vba_cov.hip, its only user): forward elimination and backward
// selected inversion over a pose range of one block-tridiagonal chain, by one wavefront.  One function, two instantiations: the plain
// chain (k_cov_seq, k_cov_sep) and the chunk of the partitioned path (k_cov_chunk), which carries 18 coupling columns through the same
// elimination.  A change to the pivot rule, the symmetrisation or the mirroring is made here, once.
#pragma once
#include "vba_device.h"

namespace vba {

// bw [n_rows][3][81] (sub, diag, super; row-major blocks); A^ = (A + A^T) / 2 + lam32 I
__device__ __forceinline__ double cov_ad(const double* bw, int i, int r, int c, double lam32) {     // A^_ii[r][c]
    return 0.5 * (bw[(size_t)i * 243 + 81 + r * 9 + c] + bw[(size_t)i * 243 + 81 + c * 9 + r]) + (r == c ? lam32 : 0.0);
}
__device__ __forceinline__ double cov_b(const double* bw, int i, int r, int c) {                    // A^_i,i+1[r][c]
    return 0.5 * (bw[(size_t)i * 243 + 162 + r * 9 + c] + bw[(size_t)(i + 1) * 243 + c * 9 + r]);
}

// entry t < 45 of the upper triangle of a 9x9 block, row by row: (r, q), r <= q
__device__ __forceinline__ void cov_tri(int t, int& r, int& q) {
    r = 0;
    while (t >= 9 - r) { t -= 9 - r; ++r; }
    q = r + t;
}

// The nine pivots of the Gauss-Jordan elimination of the augmented block whose column the lane holds in a (every lane of the wave
// calls it: the pivot row is read with v_readlane).  d0: the diagonal each pivot started from.  Returns the VBA_FLAG_* bits.
__device__ __forceinline__ unsigned cov_pivots(double (&a)[9], const double (&d0)[9]) {
    unsigned fl = 0u;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const double piv = readlane_f64(a[k], k);
        double f[9];
#pragma unroll
        for (int r = 0; r < 9; ++r) f[r] = r == k ? 0.0 : readlane_f64(a[r], k);
        if (!(fabs(piv) <= 1.79e308)) fl |= VBA_FLAG_NONFINITE;
        else if (!(fabs(piv) > 1e-10 * fabs(d0[k]))) fl |= VBA_FLAG_ZERO_PIVOT;
        else if (piv < 0.0) fl |= VBA_FLAG_INDEFINITE;
        a[k] *= fast_rcp(piv);
#pragma unroll
        for (int r = 0; r < 9; ++r)
            if (r != k) a[r] = fma(-f[r], a[k], a[r]);
    }
    return fl;
}

// The LDS of the recurrence; the kernel declares one __shared__.  The coupled arrays exist in the coupled instantiation only.
template <bool COUPLED> struct CovLds {
    double Bp[81], Yp[81];                  // forward: symmetrised B_{i-1}, Y_{i-1}
    double Sn[81], Yl[81], Su[81], Dl[81];  // backward: S_{i+1,i+1}, Y_i, S_i,i+1, D_i^-1
};
template <> struct CovLds<true> : CovLds<false> {
    double Zp[162];                         // forward: the coupling columns of pose i-1 (rows of X before the backward sweep)
    double Xn[162];                         // backward: x_{i+1}; x_first when the sweep has ended
};

// The selected inversion of poses first .. last of the chain bw (T = the block-tridiagonal matrix of that range, cut off at both ends).
// Lane c owns column c of [A^_ii | B_i | I] (27 columns); Dw / Sw [.][81] get T^-1's blocks S_ii and S_i,i+1 of these poses (the super
// block of `last`: zeros).  COUPLED: lanes 27..44 carry [A^_first,first-1 (hasL) | A^_last,last+1 (hasR)] as 18 more right-hand sides,
// and Xw [.][9][18] gets X = T^-1 of those columns by x_i = z_i - Y_i x_i+1 beside the backward sweep.
// Returns the VBA_FLAG_* bits of the pivots; with VBA_FLAG_ZERO_PIVOT or VBA_FLAG_NONFINITE among them there is no backward sweep and
// the arrays hold the forward sweep's Y_i, D_i^-1 (the caller writes what a singular chain reports).
template <bool COUPLED>
__device__ __forceinline__ unsigned cov_chain(CovLds<COUPLED>& L, const double* __restrict__ bw, int first, int last, double lam32,
                                              double* Dw, double* Sw, bool hasL = false, bool hasR = false, double* Xw = nullptr) {
    const int lane = threadIdx.x;
    unsigned fl = 0u;
    // ---- forward sweep
    // lane c's column for pose i; the next pose's is loaded while this one is eliminated (the walk is a chain of dependent steps: a
    // load issued at the top of the step it feeds would put its latency on that chain).  One branch per lane group around the nine
    // rows, not one per row: with the choice inside the row loop the plain walk measured 20 % slower per step.
    auto column = [&](int i, double (&a)[9]) {
        const int c = lane;
        if (c < 9) {
#pragma unroll
            for (int r = 0; r < 9; ++r) a[r] = cov_ad(bw, i, r, c, lam32);
        } else if (c < 18) {
            const bool has = i < last;
#pragma unroll
            for (int r = 0; r < 9; ++r) a[r] = has ? cov_b(bw, i, r, c - 9) : 0.0;
        } else {
#pragma unroll
            for (int r = 0; r < 9; ++r) a[r] = (c < 27 && r == c - 18) ? 1.0 : 0.0;
            if constexpr (COUPLED) {
                if (c >= 27 && c < 36 && i == first && hasL) {          // A^_first,sL = A^_sL,first^T
#pragma unroll
                    for (int r = 0; r < 9; ++r) a[r] = cov_b(bw, first - 1, c - 27, r);
                } else if (c >= 36 && c < 45 && i == last && hasR) {    // A^_last,sR
#pragma unroll
                    for (int r = 0; r < 9; ++r) a[r] = cov_b(bw, last, r, c - 36);
                }
            }
        }
    };
    double nx[9];
    if (first <= last) column(first, nx);
    for (int i = first; i <= last; ++i) {
        double a[9];
        const int c = lane;
#pragma unroll
        for (int r = 0; r < 9; ++r) a[r] = nx[r];
        if (i < last) column(i + 1, nx);
        double bcol[9];
#pragma unroll
        for (int r = 0; r < 9; ++r) bcol[r] = a[r];
        double d0[9];       // the diagonal each pivot started from (pivot check as in the solve)
#pragma unroll
        for (int k = 0; k < 9; ++k) d0[k] = readlane_f64(a[k], k);
        if (i > first) {    // D_i = A^_ii - B_{i-1}^T Y_{i-1}, and the same update of the coupling columns
            auto minus_BtY = [&](const double* Y, int ld, int j) {
#pragma unroll
                for (int r = 0; r < 9; ++r) {
                    double s = 0.0;
#pragma unroll
                    for (int k = 0; k < 9; ++k) s = fma(L.Bp[k * 9 + r], Y[k * ld + j], s);
                    a[r] -= s;
                }
            };
            if (c < 9) minus_BtY(L.Yp, 9, c);
            else if constexpr (COUPLED)
                if (c >= 27 && c < 45) minus_BtY(L.Zp, 18, c - 27);
        }
        fl |= cov_pivots(a, d0);
        __syncthreads();        // (every lane has read B_{i-1}, Y_{i-1})
        if (c >= 9 && c < 18) {
            const int j = c - 9;
#pragma unroll
            for (int r = 0; r < 9; ++r) {
                Sw[(size_t)i * 81 + r * 9 + j] = a[r];
                L.Yp[r * 9 + j] = a[r];
                L.Bp[r * 9 + j] = bcol[r];
            }
        } else if (c >= 18 && c < 27) {
            const int j = c - 18;
#pragma unroll
            for (int r = 0; r < 9; ++r) Dw[(size_t)i * 81 + r * 9 + j] = a[r];
        } else if constexpr (COUPLED) {
            if (c >= 27 && c < 45) {
                const int j = c - 27;
#pragma unroll
                for (int r = 0; r < 9; ++r) {
                    Xw[(size_t)i * 162 + r * 18 + j] = a[r];
                    L.Zp[r * 18 + j] = a[r];
                }
            }
        }
        __syncthreads();
    }
    if (first > last || (fl & (VBA_FLAG_ZERO_PIVOT | VBA_FLAG_NONFINITE))) return fl;
    // ---- backward sweep: entries e = lane, lane + 64 of a 9x9 block (and lane + 128 of a 9x18 one)
    const int e0 = lane, e1 = lane + 64, e2 = lane + 128;
    const bool has1 = e1 < 81, has2 = e2 < 162;
    {   // S_last = D_last^-1 from its upper triangle, mirrored: exactly symmetric
        const size_t o = (size_t)last * 81;
        L.Dl[e0] = Dw[o + e0];
        if (has1) L.Dl[e1] = Dw[o + e1];
        if constexpr (COUPLED) {
            const double* xl = Xw + (size_t)last * 162;
            L.Xn[e0] = xl[e0];
            L.Xn[e1] = xl[e1];
            if (has2) L.Xn[e2] = xl[e2];
        }
        __syncthreads();
        auto upper = [&](int e) { const int r = e / 9, q = e % 9; return r <= q ? L.Dl[r * 9 + q] : L.Dl[q * 9 + r]; };
        const double v0 = upper(e0), v1 = has1 ? upper(e1) : 0.0;
        L.Sn[e0] = v0; Dw[o + e0] = v0; Sw[o + e0] = 0.0;
        if (has1) { L.Sn[e1] = v1; Dw[o + e1] = v1; Sw[o + e1] = 0.0; }
        __syncthreads();
    }
    // Y_i, D_i^-1 (and z_i: only the lane that loaded an entry of it reads it) of the next step, loaded one step ahead
    double py0 = 0.0, py1 = 0.0, pd0 = 0.0, pd1 = 0.0, pz0 = 0.0, pz1 = 0.0, pz2 = 0.0;
    auto ahead = [&](int i) {
        const size_t o = (size_t)i * 81;
        py0 = Sw[o + e0]; pd0 = Dw[o + e0];
        if (has1) { py1 = Sw[o + e1]; pd1 = Dw[o + e1]; }
        if constexpr (COUPLED) {
            const double* z = Xw + (size_t)i * 162;
            pz0 = z[e0]; pz1 = z[e1];
            if (has2) pz2 = z[e2];
        }
    };
    if (last > first) ahead(last - 1);
    for (int i = last - 1; i >= first; --i) {
        const size_t o = (size_t)i * 81;
        L.Yl[e0] = py0;
        L.Dl[e0] = pd0;
        if (has1) { L.Yl[e1] = py1; L.Dl[e1] = pd1; }
        const double z0 = pz0, z1 = pz1, z2 = pz2;
        if (i > first) ahead(i - 1);
        __syncthreads();
        // S_i,i+1 = -Y_i S_i+1,i+1
        for (int e = lane; e < 81; e += 64) {
            const int r = e / 9, q = e % 9;
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 9; ++k) s = fma(L.Yl[r * 9 + k], L.Sn[k * 9 + q], s);
            L.Su[e] = -s;
            Sw[o + e] = -s;
        }
        double x0 = 0.0, x1 = 0.0, x2 = 0.0;
        if constexpr (COUPLED) {    // x_i = z_i - Y_i x_i+1
            auto yx = [&](int e) {
                const int r = e / 18, q = e % 18;
                double t = 0.0;
#pragma unroll
                for (int k = 0; k < 9; ++k) t = fma(L.Yl[r * 9 + k], L.Xn[k * 18 + q], t);
                return t;
            };
            x0 = z0 - yx(e0);
            x1 = z1 - yx(e1);
            if (has2) x2 = z2 - yx(e2);
        }
        __syncthreads();
        // S_ii = D_i^-1 - S_i,i+1 Y_i^T, upper triangle (45 entries, one lane each), mirrored
        double v = 0.0;
        int r = 0, q = 0;
        if (lane < 45) {
            cov_tri(lane, r, q);
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 9; ++k) s = fma(L.Su[r * 9 + k], L.Yl[q * 9 + k], s);
            v = L.Dl[r * 9 + q] - s;
        }
        __syncthreads();        // (every lane has read S_i+1,i+1 and x_i+1 before they are replaced)
        if (lane < 45) {
            L.Sn[r * 9 + q] = v;
            L.Sn[q * 9 + r] = v;
            Dw[o + r * 9 + q] = v;
            Dw[o + q * 9 + r] = v;
        }
        if constexpr (COUPLED) {
            double* xi = Xw + (size_t)i * 162;
            L.Xn[e0] = x0; xi[e0] = x0;
            L.Xn[e1] = x1; xi[e1] = x1;
            if (has2) { L.Xn[e2] = x2; xi[e2] = x2; }
        }
        __syncthreads();
    }
    return fl;
}

}  // namespace vba
