// vba_cov.hip -- per-pose marginal covariances (vba_covariance): the diagonal and super-diagonal 9x9 blocks of the inverse of the
// symmetrised full-phase system at the resident states.
//
// The system is built by the kernels of a BA() call's front (residuals, exact select, accumulation, dynamics / attitude / long-gap
// factors, assembly) run on a SHADOW view: every array those kernels write is scratch of the query (allocated on the first query,
// like d_dbg), the window scalars and the carried chunk states of the long edges are copies.  The handle's own memory -- states,
// damping, flags, carried keys and histograms, bin buckets, chain pool, graph keys -- is only read, so the calls that follow give the
// bits they would have given without the query.
//
// Selected inversion of the symmetric block-tridiagonal matrix, blocks A_ii (diagonal) and B_i = A_i,i+1:
//   forward   D_i = A_ii - B_{i-1}^T Y_{i-1},  Y_i = D_i^-1 B_i      (block LDL^T; D_i^-1 comes from the same elimination)
//   backward  S_n-1 = D_n-1^-1,  S_i,i+1 = -Y_i S_i+1,  S_ii = D_i^-1 - S_i,i+1 Y_i^T
// Two paths, chosen by the solver setting of the handle (vba_set_solver): the sequential walk, one wavefront per window (k_cov_seq);
// the partitioned path over the solver's chunks (k_cov_chunk, k_cov_sep, k_cov_fix; see there).  Lane c owns column c of [D_i | B_i | I] (27 columns): the Gauss-Jordan elimination of that
// augmented block leaves Y_i in lanes 9..17 and D_i^-1 in lanes 18..26 -- the solve's own step (vba_solve_step.h) with nine identity
// right-hand sides in its idle lanes.  The pivot row is read with v_readlane (one system per wave: the row is uniform).  Y_i and
// D_i^-1 are kept in the two output arrays and overwritten by S_i,i+1 and S_ii in the backward sweep.
#include "vba_context.h"
#include "vba_step.h"

namespace vba {

// The selected inversion of one block-tridiagonal chain by one wavefront: bw [n_rows][3][81] (sub, diag, super; row-major blocks) of
// which the first n are poses, A^ = (A + A^T) / 2 + lam32 I.  Dw / Sw [n_rows][81]: S_ii and S_i,i+1 (rows >= n and the super block of
// the last pose: zeros; NaN blocks if a pivot was zero or not finite).  Returns the VBA_FLAG_* bits of the pivots.
__device__ unsigned cov_walk(const double* __restrict__ bw, int n, int n_rows, double lam32, double* Dw, double* Sw) {
    __shared__ double Bp[81], Yp[81];       // forward: symmetrised B_{i-1}, Y_{i-1}
    __shared__ double Sn[81], Yl[81], Su[81], Dl[81];   // backward: S_{i+1,i+1}, Y_i, S_i,i+1, D_i^-1
    const int lane = threadIdx.x;
    const int n_max = n_rows;
    unsigned fl = 0u;
    // ---- forward sweep
    // lane c's column of [A^_ii | B_i | I] for pose i; the next pose's is loaded while this one is eliminated (the walk is a chain of
    // dependent steps: a load issued at the top of the step it feeds would put its latency on that chain)
    auto column = [&](int i, double (&a)[9]) {
        const double* bi = bw + (size_t)i * 243;
        const int c = lane;
        if (c < 9) {
#pragma unroll
            for (int r = 0; r < 9; ++r) a[r] = 0.5 * (bi[81 + r * 9 + c] + bi[81 + c * 9 + r]) + (r == c ? lam32 : 0.0);
        } else if (c < 18) {
            const int j = c - 9;
            const bool has = i + 1 < n;
#pragma unroll
            for (int r = 0; r < 9; ++r) a[r] = has ? 0.5 * (bi[162 + r * 9 + j] + bi[243 + j * 9 + r]) : 0.0;
        } else {
#pragma unroll
            for (int r = 0; r < 9; ++r) a[r] = (c < 27 && r == c - 18) ? 1.0 : 0.0;
        }
    };
    double nx[9];
    if (n > 0) column(0, nx);
    for (int i = 0; i < n; ++i) {
        double a[9];
        const int c = lane;
#pragma unroll
        for (int r = 0; r < 9; ++r) a[r] = nx[r];
        if (i + 1 < n) column(i + 1, nx);
        double bcol[9];
#pragma unroll
        for (int r = 0; r < 9; ++r) bcol[r] = a[r];
        double d0[9];       // the diagonal each pivot started from (pivot check as in the solve)
#pragma unroll
        for (int k = 0; k < 9; ++k) d0[k] = readlane_f64(a[k], k);
        if (i > 0 && c < 9) {
#pragma unroll
            for (int r = 0; r < 9; ++r) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 9; ++k) s = fma(Bp[k * 9 + r], Yp[k * 9 + c], s);
                a[r] -= s;
            }
        }
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
        __syncthreads();        // (every lane has read B_{i-1}, Y_{i-1})
        if (c >= 9 && c < 18) {
            const int j = c - 9;
#pragma unroll
            for (int r = 0; r < 9; ++r) {
                Sw[(size_t)i * 81 + r * 9 + j] = a[r];
                Yp[r * 9 + j] = a[r];
                Bp[r * 9 + j] = bcol[r];
            }
        } else if (c >= 18 && c < 27) {
            const int j = c - 18;
#pragma unroll
            for (int r = 0; r < 9; ++r) Dw[(size_t)i * 81 + r * 9 + j] = a[r];
        }
        __syncthreads();
    }
    // ---- rows without a pose
    for (int e = lane; e < (n_max - n) * 81; e += 64) {
        Dw[(size_t)n * 81 + e] = 0.0;
        Sw[(size_t)n * 81 + e] = 0.0;
    }
    if (fl & (VBA_FLAG_ZERO_PIVOT | VBA_FLAG_NONFINITE)) {     // numerically singular: no covariance
        for (int e = lane; e < n * 81; e += 64) {
            Dw[e] = __builtin_nan("");
            Sw[e] = (e >= (n - 1) * 81) ? 0.0 : __builtin_nan("");
        }
        return fl;
    }
    // ---- backward sweep: entries e = lane, lane + 64 of a 9x9 block
    const int e0 = lane, e1 = lane + 64;
    const bool has1 = e1 < 81;
    auto upper = [&](int e, double* dst, const double* src) {      // S_ii from the upper triangle, mirrored: exactly symmetric
        const int r = e / 9, q = e % 9;
        dst[e] = r <= q ? src[r * 9 + q] : src[q * 9 + r];
    };
    if (n > 0) {
        const size_t o = (size_t)(n - 1) * 81;
        Dl[e0] = Dw[o + e0];
        if (has1) Dl[e1] = Dw[o + e1];
        __syncthreads();
        upper(e0, Sn, Dl);
        if (has1) upper(e1, Sn, Dl);
        Dw[o + e0] = Sn[e0];
        Sw[o + e0] = 0.0;
        if (has1) { Dw[o + e1] = Sn[e1]; Sw[o + e1] = 0.0; }
        __syncthreads();
    }
    double py0 = 0.0, py1 = 0.0, pd0 = 0.0, pd1 = 0.0;      // Y_i, D_i^-1 of the next step, loaded one step ahead
    if (n >= 2) {
        const size_t o = (size_t)(n - 2) * 81;
        py0 = Sw[o + e0]; pd0 = Dw[o + e0];
        if (has1) { py1 = Sw[o + e1]; pd1 = Dw[o + e1]; }
    }
    for (int i = n - 2; i >= 0; --i) {
        const size_t o = (size_t)i * 81;
        Yl[e0] = py0;
        Dl[e0] = pd0;
        if (has1) { Yl[e1] = py1; Dl[e1] = pd1; }
        if (i > 0) {
            const size_t o1 = (size_t)(i - 1) * 81;
            py0 = Sw[o1 + e0]; pd0 = Dw[o1 + e0];
            if (has1) { py1 = Sw[o1 + e1]; pd1 = Dw[o1 + e1]; }
        }
        __syncthreads();
        // S_i,i+1 = -Y_i S_i+1,i+1
        for (int e = lane; e < 81; e += 64) {
            const int r = e / 9, q = e % 9;
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 9; ++k) s = fma(Yl[r * 9 + k], Sn[k * 9 + q], s);
            Su[e] = -s;
            Sw[o + e] = -s;
        }
        __syncthreads();
        // S_ii = D_i^-1 - S_i,i+1 Y_i^T, upper triangle (45 entries, one lane each), mirrored
        double v = 0.0;
        int r = 0, q = 0;
        if (lane < 45) {
            int t = lane;
            while (t >= 9 - r) { t -= 9 - r; ++r; }
            q = r + t;
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 9; ++k) s = fma(Su[r * 9 + k], Yl[q * 9 + k], s);
            v = Dl[r * 9 + q] - s;
        }
        __syncthreads();        // (every lane has read S_i+1,i+1 before it is replaced)
        if (lane < 45) {
            Sn[r * 9 + q] = v;
            Sn[q * 9 + r] = v;
            Dw[o + r * 9 + q] = v;
            Dw[o + q * 9 + r] = v;
        }
        __syncthreads();
    }
    return fl;
}

// Sequential path: one wavefront walks the whole chain of its window.  bands [W][n_max][243]; sc / par: the damping of the call the
// resident states feed; diag / sup [W][n_max][81]; flags [W].
__global__ __launch_bounds__(64) void k_cov_seq(const double* __restrict__ bands, const int* __restrict__ nw, int n_max,
                                                const WinScalars* __restrict__ sc, int par, int damped, double* diag, double* sup,
                                                unsigned* flags) {
    const int w = blockIdx.x;
    const double lam32 = damped ? (double)(float)sc[w].lam[par] : 0.0;     // torch.eye() is float32 (BA_filtering.py:54)
    const unsigned fl = cov_walk(bands + (size_t)w * n_max * 243, nw[w], n_max, lam32, diag + (size_t)w * n_max * 81,
                                 sup + (size_t)w * n_max * 81);
    if (threadIdx.x == 0) flags[w] = fl;
}

// ---- partitioned path (latency-mode handles, chunked solver setting): the chain is cut into chunks of s poses whose last pose is a
// separator, as the partitioned solve cuts it.  With I the interior poses (block diagonal over chunks, T_c per chunk), S the
// separators and X = T^-1 A_IS:
//   Sigma_SS = (A_SS - A_SI X)^-1,  Sigma_IS = -X Sigma_SS,  Sigma_II = T^-1 + X Sigma_SS X^T
// Three launches behind the front: k_cov_chunk (one wave per chunk: T^-1's diagonal / super-diagonal blocks by the recurrence of
// cov_walk, X by the same elimination with the 18 coupling columns as right-hand sides in lanes 27..44, and the chunk's part of the
// separator Schur complement), k_cov_sep (one wave per window: the separator system assembled and walked by cov_walk), k_cov_fix
// (one wave per chunk: T^-1 + X Sigma_SS X^T, the interior-separator blocks, the separators' own blocks).
__device__ __forceinline__ double cov_ad(const double* bw, int i, int r, int c, double lam32) {     // A^_ii[r][c]
    return 0.5 * (bw[(size_t)i * 243 + 81 + r * 9 + c] + bw[(size_t)i * 243 + 81 + c * 9 + r]) + (r == c ? lam32 : 0.0);
}
__device__ __forceinline__ double cov_b(const double* bw, int i, int r, int c) {                    // A^_i,i+1[r][c]
    return 0.5 * (bw[(size_t)i * 243 + 162 + r * 9 + c] + bw[(size_t)(i + 1) * 243 + c * 9 + r]);
}

// X [W][n_max][9][18] (left, right coupling columns); contrib [W][p_rows][3][81]: per chunk A_sL,first X_first[:, L], A_sR,last X_last[:, R],
// A_sL,first X_first[:, R]
__global__ __launch_bounds__(64) void k_cov_chunk(const double* __restrict__ bands, const int* __restrict__ nw, int n_max, int s,
                                                  const WinScalars* __restrict__ sc, int par, int damped, double* diag, double* sup,
                                                  double* X, double* contrib, int p_rows, unsigned* flags) {
    __shared__ double Bp[81], Yp[81], Zp[162];
    __shared__ double Sn[81], Yl[81], Su[81], Dl[81], Zl[162], Xn[162];
    const int w = blockIdx.y, ch = blockIdx.x, lane = threadIdx.x;
    const int n = nw[w];
    const int P = (n + s - 1) / s;
    if (ch >= P) return;
    const bool hasL = ch > 0, hasR = ch < P - 1;
    const int first = ch * s, last = hasR ? (ch + 1) * s - 2 : n - 1;
    const int sL = first - 1;
    const double* bw = bands + (size_t)w * n_max * 243;
    double* Dw = diag + (size_t)w * n_max * 81;
    double* Sw = sup + (size_t)w * n_max * 81;
    double* Xw = X + (size_t)w * n_max * 162;
    const double lam32 = damped ? (double)(float)sc[w].lam[par] : 0.0;
    unsigned fl = 0u;
    auto column = [&](int i, double (&a)[9]) {
        const int c = lane;
#pragma unroll
        for (int r = 0; r < 9; ++r) {
            double v = 0.0;
            if (c < 9) v = cov_ad(bw, i, r, c, lam32);
            else if (c < 18) v = i < last ? cov_b(bw, i, r, c - 9) : 0.0;
            else if (c < 27) v = r == c - 18 ? 1.0 : 0.0;
            else if (c < 36) v = (i == first && hasL) ? cov_b(bw, sL, c - 27, r) : 0.0;      // A^_first,sL = A^_sL,first^T
            else if (c < 45) v = (i == last && hasR) ? cov_b(bw, last, r, c - 36) : 0.0;     // A^_last,sR
            a[r] = v;
        }
    };
    double nx[9];
    column(first, nx);
    for (int i = first; i <= last; ++i) {
        double a[9];
        const int c = lane;
#pragma unroll
        for (int r = 0; r < 9; ++r) a[r] = nx[r];
        if (i < last) column(i + 1, nx);
        double bcol[9];
#pragma unroll
        for (int r = 0; r < 9; ++r) bcol[r] = a[r];
        double d0[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) d0[k] = readlane_f64(a[k], k);
        if (i > first) {
            if (c < 9) {
#pragma unroll
                for (int r = 0; r < 9; ++r) {
                    double t = 0.0;
#pragma unroll
                    for (int k = 0; k < 9; ++k) t = fma(Bp[k * 9 + r], Yp[k * 9 + c], t);
                    a[r] -= t;
                }
            } else if (c >= 27 && c < 45) {
                const int j = c - 27;
#pragma unroll
                for (int r = 0; r < 9; ++r) {
                    double t = 0.0;
#pragma unroll
                    for (int k = 0; k < 9; ++k) t = fma(Bp[k * 9 + r], Zp[k * 18 + j], t);
                    a[r] -= t;
                }
            }
        }
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
        __syncthreads();
        if (c >= 9 && c < 18) {
            const int j = c - 9;
#pragma unroll
            for (int r = 0; r < 9; ++r) {
                Sw[(size_t)i * 81 + r * 9 + j] = a[r];
                Yp[r * 9 + j] = a[r];
                Bp[r * 9 + j] = bcol[r];
            }
        } else if (c >= 18 && c < 27) {
            const int j = c - 18;
#pragma unroll
            for (int r = 0; r < 9; ++r) Dw[(size_t)i * 81 + r * 9 + j] = a[r];
        } else if (c >= 27 && c < 45) {
            const int j = c - 27;
#pragma unroll
            for (int r = 0; r < 9; ++r) {
                Xw[(size_t)i * 162 + r * 18 + j] = a[r];
                Zp[r * 18 + j] = a[r];
            }
        }
        __syncthreads();
    }
    if (fl & (VBA_FLAG_ZERO_PIVOT | VBA_FLAG_NONFINITE)) {      // k_cov_fix writes the NaN blocks
        if (lane == 0) atomicOr(flags + w, fl);
        return;
    }
    // ---- backward inside the chunk: T^-1 (as cov_walk) and x_i = z_i - Y_i x_i+1
    {
        const size_t o = (size_t)last * 81;
        for (int e = lane; e < 81; e += 64) Dl[e] = Dw[o + e];
        for (int e = lane; e < 162; e += 64) Xn[e] = Xw[(size_t)last * 162 + e];
        __syncthreads();
        for (int e = lane; e < 81; e += 64) {
            const int r = e / 9, q = e % 9;
            const double v = r <= q ? Dl[r * 9 + q] : Dl[q * 9 + r];
            Sn[e] = v;
            Dw[o + e] = v;
        }
        __syncthreads();
    }
    for (int i = last - 1; i >= first; --i) {
        const size_t o = (size_t)i * 81;
        for (int e = lane; e < 81; e += 64) { Yl[e] = Sw[o + e]; Dl[e] = Dw[o + e]; }
        for (int e = lane; e < 162; e += 64) Zl[e] = Xw[(size_t)i * 162 + e];
        __syncthreads();
        for (int e = lane; e < 81; e += 64) {
            const int r = e / 9, q = e % 9;
            double t = 0.0;
#pragma unroll
            for (int k = 0; k < 9; ++k) t = fma(Yl[r * 9 + k], Sn[k * 9 + q], t);
            Su[e] = -t;
            Sw[o + e] = -t;
        }
        double xv[3];
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int e = lane + 64 * u;
            xv[u] = 0.0;
            if (e < 162) {
                const int r = e / 18, q = e % 18;
                double t = 0.0;
#pragma unroll
                for (int k = 0; k < 9; ++k) t = fma(Yl[r * 9 + k], Xn[k * 18 + q], t);
                xv[u] = Zl[e] - t;
            }
        }
        __syncthreads();
        double v = 0.0;
        int r = 0, q = 0;
        if (lane < 45) {
            int t = lane;
            while (t >= 9 - r) { t -= 9 - r; ++r; }
            q = r + t;
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 9; ++k) acc = fma(Su[r * 9 + k], Yl[q * 9 + k], acc);
            v = Dl[r * 9 + q] - acc;
        }
        __syncthreads();
        if (lane < 45) {
            Sn[r * 9 + q] = v; Sn[q * 9 + r] = v;
            Dw[o + r * 9 + q] = v; Dw[o + q * 9 + r] = v;
        }
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int e = lane + 64 * u;
            if (e < 162) { Xn[e] = xv[u]; Xw[(size_t)i * 162 + e] = xv[u]; }
        }
        __syncthreads();
    }
    // ---- this chunk's part of the separator Schur complement (Xn = x_first; x_last from memory)
    double* cb = contrib + ((size_t)w * p_rows + ch) * 243;
    const double* xl = Xw + (size_t)last * 162;
    for (int e = lane; e < 81; e += 64) {
        const int r = e / 9, q = e % 9;
        double dl = 0.0, dr = 0.0, lr = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            if (hasL) {
                const double bl = cov_b(bw, sL, r, k);          // A^_sL,first
                dl = fma(bl, Xn[k * 18 + q], dl);
                lr = fma(bl, Xn[k * 18 + 9 + q], lr);
            }
            if (hasR) dr = fma(cov_b(bw, last, k, r), xl[k * 18 + 9 + q], dr);      // A^_sR,last = A^_last,sR^T
        }
        cb[e] = dl;
        cb[81 + e] = dr;
        cb[162 + e] = lr;
    }
    if (lane == 0 && fl) atomicOr(flags + w, fl);
}

// the separator system of window w (assembled into sepb [W][p_rows][243]) and its selected inversion -> SSd / SSs [W][p_rows][81]
__global__ __launch_bounds__(64) void k_cov_sep(const double* __restrict__ bands, const int* __restrict__ nw, int n_max, int s,
                                                const WinScalars* __restrict__ sc, int par, int damped, const double* contrib,
                                                double* sepb, int p_rows, double* SSd, double* SSs, unsigned* flags) {
    const int w = blockIdx.x, lane = threadIdx.x;
    const int n = nw[w];
    const int q = (n + s - 1) / s - 1;
    if (q <= 0 || (flags[w] & (VBA_FLAG_ZERO_PIVOT | VBA_FLAG_NONFINITE))) return;
    const double* bw = bands + (size_t)w * n_max * 243;
    const double* cb = contrib + (size_t)w * p_rows * 243;
    double* sb = sepb + (size_t)w * p_rows * 243;
    const double lam32 = damped ? (double)(float)sc[w].lam[par] : 0.0;
    for (int e = lane; e < q * 243; e += 64) {
        const int j = e / 243, k = e % 243, blk = k / 81, rc = k % 81, r = rc / 9, c = rc % 9;
        double v = 0.0;
        if (blk == 1) v = cov_ad(bw, (j + 1) * s - 1, r, c, lam32) - cb[(size_t)j * 243 + 81 + rc] - cb[(size_t)(j + 1) * 243 + rc];
        else if (blk == 2) v = j + 1 < q ? -cb[(size_t)(j + 1) * 243 + 162 + rc] : 0.0;      // (sep j, sep j+1): chunk j + 1 couples them
        else v = j > 0 ? -cb[(size_t)j * 243 + 162 + c * 9 + r] : 0.0;                        // (sep j, sep j-1): the transpose
        sb[e] = v;
    }
    __syncthreads();
    const unsigned fl = cov_walk(sb, q, p_rows, 0.0, SSd + (size_t)w * p_rows * 81, SSs + (size_t)w * p_rows * 81);
    if (lane == 0 && fl) atomicOr(flags + w, fl);
}

__global__ __launch_bounds__(64) void k_cov_fix(const int* __restrict__ nw, int n_max, int s, double* diag, double* sup, const double* X,
                                                const double* SSd, const double* SSs, int p_rows, const unsigned* flags) {
    __shared__ double M[324], Xi[162], Xj[162], XM[162];
    const int w = blockIdx.y, ch = blockIdx.x, lane = threadIdx.x;
    const int n = nw[w];
    const int P = (n + s - 1) / s;
    if (ch >= P) return;
    const bool hasL = ch > 0, hasR = ch < P - 1;
    const int first = ch * s, last = hasR ? (ch + 1) * s - 2 : n - 1;
    const int sL = first - 1, sR = last + 1;
    double* Dw = diag + (size_t)w * n_max * 81;
    double* Sw = sup + (size_t)w * n_max * 81;
    const double* Xw = X + (size_t)w * n_max * 162;
    const double* sd = SSd + (size_t)w * p_rows * 81;
    const double* ss = SSs + (size_t)w * p_rows * 81;
    if (ch == P - 1)
        for (int e = lane; e < (n_max - n) * 81; e += 64) { Dw[(size_t)n * 81 + e] = 0.0; Sw[(size_t)n * 81 + e] = 0.0; }
    if (flags[w] & (VBA_FLAG_ZERO_PIVOT | VBA_FLAG_NONFINITE)) {     // numerically singular: no covariance
        const double nan = __builtin_nan("");
        for (int e = lane; e < (last - first + 1) * 81; e += 64) {
            Dw[(size_t)first * 81 + e] = nan;
            Sw[(size_t)first * 81 + e] = (first * 81 + e >= (n - 1) * 81) ? 0.0 : nan;
        }
        for (int e = lane; e < 81; e += 64) {
            if (hasR) Dw[(size_t)sR * 81 + e] = nan;
            if (hasL) Sw[(size_t)sL * 81 + e] = nan;
        }
        return;
    }
    for (int e = lane; e < 324; e += 64) {
        const int r = e / 18, c = e % 18;
        double v = 0.0;
        if (r < 9 && c < 9) v = hasL ? sd[(size_t)(ch - 1) * 81 + r * 9 + c] : 0.0;
        else if (r < 9) v = (hasL && hasR) ? ss[(size_t)(ch - 1) * 81 + r * 9 + (c - 9)] : 0.0;
        else if (c < 9) v = (hasL && hasR) ? ss[(size_t)(ch - 1) * 81 + c * 9 + (r - 9)] : 0.0;
        else v = hasR ? sd[(size_t)ch * 81 + (r - 9) * 9 + (c - 9)] : 0.0;
        M[e] = v;
    }
    for (int e = lane; e < 162; e += 64) Xi[e] = Xw[(size_t)first * 162 + e];
    __syncthreads();
    for (int i = first; i <= last; ++i) {
        const size_t o = (size_t)i * 81;
        for (int e = lane; e < 162; e += 64) {
            const int r = e / 18, c = e % 18;
            double t = 0.0;
#pragma unroll
            for (int k = 0; k < 18; ++k) t = fma(Xi[r * 18 + k], M[k * 18 + c], t);
            XM[e] = t;
        }
        if (i < last)
            for (int e = lane; e < 162; e += 64) Xj[e] = Xw[(size_t)(i + 1) * 162 + e];
        __syncthreads();
        if (lane < 45) {        // Sigma_ii = T^-1_ii + (X M X^T)_ii: upper triangle, mirrored
            int t = lane, r = 0;
            while (t >= 9 - r) { t -= 9 - r; ++r; }
            const int q = r + t;
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 18; ++k) acc = fma(XM[r * 18 + k], Xi[q * 18 + k], acc);
            const double v = Dw[o + r * 9 + q] + acc;
            Dw[o + r * 9 + q] = v;
            Dw[o + q * 9 + r] = v;
        }
        for (int e = lane; e < 81; e += 64) {
            const int r = e / 9, q = e % 9;
            if (i < last) {
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < 18; ++k) acc = fma(XM[r * 18 + k], Xj[q * 18 + k], acc);
                Sw[o + e] += acc;
            } else {
                Sw[o + e] = hasR ? -XM[r * 18 + 9 + q] : 0.0;       // Sigma_last,sR = -(X M)_last[:, R]
            }
            if (i == first && hasL) Sw[(size_t)sL * 81 + e] = -XM[q * 18 + r];     // Sigma_sL,first = -((X M)_first[:, L])^T
        }
        __syncthreads();
        for (int e = lane; e < 162; e += 64) Xi[e] = Xj[e];
        __syncthreads();
    }
    if (hasR)
        for (int e = lane; e < 81; e += 64) Dw[(size_t)sR * 81 + e] = sd[(size_t)ch * 81 + e];
}

}  // namespace vba

// ---------------------------------------------------------------------------------------------------------- host side

// The scratch of the covariance step: the shadow of every array the front of a call writes (into V), and what the selected inversion
// writes.  Sizes come from V alone, so the counting and the placing run agree by construction.
struct CovBufs {
    WinScalars* sc;
    double* pool;
    double *diag, *sup;         // the two [W][n_max][81] result arrays
    unsigned* flags;
    double *X, *contrib, *sepb, *SSd, *SSs;     // partitioned path: X, chunk contributions, separator bands, separator blocks of Sigma
};
static CovBufs cov_layout(Carver& c, DevView& V, size_t W) {
    const size_t N = V.n_max, M = V.m_max, PR = (size_t)V.p_max;
    CovBufs b;
    b.sc = c.take<WinScalars>(W);
    V.sc = b.sc;
    V.absr = c.take<double>(W * 2 * M);
    V.wraw = c.take<double>(W * M);
    V.ckeys = c.take<double>(W * 2 * M);
    V.part_init = c.take<double>(W * V.nblk_obs);
    V.part_trial = c.take<double>(W * V.trial_stride);
    V.part_next = c.take<double>(W * V.nblk_obs);
    V.part_pred = c.take<double>(W * 2 * V.pred_stride);
    V.part_prior = c.take<double>(W * 2 * V.pred_stride);
    V.lastD = c.take<double>(W * 81);
    V.hist = c.take<unsigned>(W * kHistStride);
    V.Hraw = c.take<double>(W * N * 21);
    V.braw = c.take<double>(W * N * 6);
    {
        double* d = c.take<double>(W * N * (6 + 36 + 6 + 1 + 3 + 9 + 9 + 9));
        V.xhat = d; d += W * N * 6; V.Phi = d; d += W * N * 36; V.rorb = d; d += W * N * 6; V.fatt = d; d += W * N;
        V.qgrad = d; d += W * N * 3; V.Hd = d; d += W * N * 9; V.Hu = d; d += W * N * 9; V.Hl = d;
    }
    V.bands = c.take<double>(W * N * 243);
    V.rhs = c.take<double>(W * N * 9);
    V.states_new = c.take<double>(W * N * 10);
    b.pool = c.take<double>(W * 2 * (size_t)V.long_pool_cap * 6);
    b.diag = c.take<double>(W * N * 81);
    b.sup = c.take<double>(W * N * 81);
    b.flags = c.take<unsigned>(W);
    b.X = c.take<double>(W * N * 162);
    b.contrib = c.take<double>(W * PR * 243);
    b.sepb = c.take<double>(W * PR * 243);
    b.SSd = c.take<double>(W * PR * 81);
    b.SSs = c.take<double>(W * PR * 81);
    return b;
}

int query_reserve(vba_handle h, QueryScratch& q, size_t bytes, const char* what) {
    if (q.cap >= bytes) return VBA_OK;
    if (q.d) (void)hipFree(q.d);
    q.d = nullptr;
    q.cap = 0;
    if (hipMalloc(&q.d, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(VBA_ENOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes of " + what);
    }
    q.cap = bytes;
    return VBA_OK;
}

int query_finish(vba_handle h, QueryScratch& q) {
    if (!q.ev) HIPCHK(hipEventCreate(&q.ev));
    HIPCHK(hipEventRecord(q.ev, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipEventElapsedTime(&q.ms, h->cov_ev0, q.ev));
    q.ran = true;
    return VBA_OK;
}

int query_last_ms(vba_handle h, QueryScratch vba_context::*q, float* ms, const char* none_ran) {
    if (!h || !ms) return fail(VBA_EINVAL, "null argument");
    if (!(h->*q).ran) return fail(VBA_ESTATE, none_ran);
    *ms = (h->*q).ms;
    return VBA_OK;
}

// What every query checks first: the arguments, the handle's mode, a speculated call (dropped as a mismatched resident call drops
// it), states in every window.  `who` names the entry point in the messages.
int cov_begin(vba_handle h, int iter, const char* who) {
    if (!h) return fail(VBA_EINVAL, "null handle");
    if (iter < 0) return fail(VBA_EINVAL, "iter must be >= 0");
    if (h->sharded) return fail(VBA_ESTATE, std::string(who) + " does not serve observation-sharded handles");
    if (int rc_settle = settle(h)) return rc_settle;        // a speculated call is dropped as a mismatched resident call drops it
    if (int rc = ready(h)) return rc;
    HIPCHK(hipSetDevice(h->device));
    return VBA_OK;
}

// The shadow front and the selected inversion, enqueued on the handle's stream into the scratch of the query: the step
// vba_covariance, vba_reliability (vba_rel.hip) and vba_outlier_power (vba_power.hip) share.  cov_ev0 is recorded in front of it;
// the caller ends with query_finish.  q: the shadow view (its wraw, its window scalars with the maximum raw weight and its bands stay valid
// until the next query) and the device results.
int cov_build_invert(vba_handle h, int iter, int damped, CovQuery& q) {
    hipStream_t s = h->stream;
    const size_t W = h->W;
    // the shadow view: the view of the next call (parity h->par, full phase, nothing carried, nothing emitted) with every array
    // the front writes redirected into the scratch
    CallSpec c;
    c.iter = iter; c.initialize = 0; c.call = -1; c.par = h->par; c.emit = 0; c.carry = 0;
    DevView& V = q.V;
    view_for_call(h, V, c);
    Carver count;
    cov_layout(count, V, W);
    if (int rc = query_reserve(h, h->q_cov, count.total(), "covariance scratch failed")) return rc;
    if (!h->cov_ev0) HIPCHK(hipEventCreate(&h->cov_ev0));
    Carver place{static_cast<char*>(h->q_cov.d)};
    const CovBufs b = cov_layout(place, V, W);
    const size_t PR = (size_t)V.p_max;
    V.wbucket = nullptr;            // nothing carried: the bin buckets are neither read nor written
    V.wmax_ext = nullptr;
    V.hist0_ext[0] = V.hist0_ext[1] = nullptr;
    V.sel_slots = nullptr;
    V.host_states = nullptr;
    V.sel_inline = 0;
    V.dyn_in_acc = 0;
    // the window scalars as the next call would find them, without a pending repeat
    std::vector<WinScalars> hsc(W);
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipMemcpy(hsc.data(), h->V.sc, W * sizeof(WinScalars), hipMemcpyDeviceToHost));
    for (auto& x : hsc) { x.miss = 0; x.call_idx = 0; x.pending = -1; }
    HIPCHK(hipMemcpyAsync(b.sc, hsc.data(), W * sizeof(WinScalars), hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(h->cov_ev0, s));
    if (V.nblk_long > 0)
        HIPCHK(hipMemcpyAsync(b.pool, h->V.long_pool, W * 2 * (size_t)V.long_pool_cap * 6 * 8, hipMemcpyDeviceToDevice, s));
    V.long_pool = b.pool;
    HIPCHK(hipMemsetAsync(V.hist, 0, W * kHistStride * 4, s));
    // the front of a full-phase call with nothing carried (enqueue_front, the profiled order), then the assembly
    launch_obs_residual(V, nullptr, s);
    launch_select(V, false, s);
    V.median_ready = V.lat ? 0 : 1;
    if (V.median_ready) launch_select_finish(V, s);
    launch_obs_accumulate(V, s);
    launch_dynamics(V, s);
    launch_assemble(V, 0, s);
    // the path follows the solver setting (vba_set_solver): a chunked solve is served by the partitioned path with the same chunks,
    // the sequential walk by one wave per window
    const int s_chunk = h->V.chunk;
    if (s_chunk >= 2) {
        const int pc = (h->n_max + s_chunk - 1) / s_chunk;
        HIPCHK(hipMemsetAsync(b.flags, 0, W * 4, s));
        hipLaunchKernelGGL(k_cov_chunk, dim3(pc, h->W), dim3(64), 0, s, V.bands, V.n, h->n_max, s_chunk, h->V.sc, h->par, damped ? 1 : 0,
                           b.diag, b.sup, b.X, b.contrib, (int)PR, b.flags);
        hipLaunchKernelGGL(k_cov_sep, dim3(h->W), dim3(64), 0, s, V.bands, V.n, h->n_max, s_chunk, h->V.sc, h->par, damped ? 1 : 0,
                           b.contrib, b.sepb, (int)PR, b.SSd, b.SSs, b.flags);
        hipLaunchKernelGGL(k_cov_fix, dim3(pc, h->W), dim3(64), 0, s, V.n, h->n_max, s_chunk, b.diag, b.sup, b.X, b.SSd, b.SSs, (int)PR,
                           b.flags);
    } else {
        hipLaunchKernelGGL(k_cov_seq, dim3(h->W), dim3(64), 0, s, V.bands, V.n, h->n_max, h->V.sc, h->par, damped ? 1 : 0, b.diag, b.sup,
                           b.flags);
    }
    HIPCHK(hipGetLastError());
    q.diag = b.diag;
    q.sup = b.sup;
    q.flags = b.flags;
    return VBA_OK;
}

int vba_covariance(vba_handle h, int iter, int damped, double* diag, double* super, unsigned* flags) {
    if (int rc = cov_begin(h, iter, "vba_covariance")) return rc;
    CovQuery q;
    if (int rc = cov_build_invert(h, iter, damped, q)) return rc;
    if (int rc = query_finish(h, h->q_cov)) return rc;
    const size_t W = h->W, N = h->n_max;
    if (diag) HIPCHK(hipMemcpy(diag, q.diag, W * N * 81 * 8, hipMemcpyDeviceToHost));
    if (super) HIPCHK(hipMemcpy(super, q.sup, W * N * 81 * 8, hipMemcpyDeviceToHost));
    if (flags) HIPCHK(hipMemcpy(flags, q.flags, W * 4, hipMemcpyDeviceToHost));
    return VBA_OK;
}

int vba_last_covariance_ms(vba_handle h, float* ms) { return query_last_ms(h, &vba_context::q_cov, ms, "no covariance query has run"); }
