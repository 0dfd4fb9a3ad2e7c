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
// the partitioned path over the solver's chunks (k_cov_chunk, k_cov_sep, k_cov_fix; see there).  Both run ONE recurrence, cov_chain
// (vba_cov_walk.h): lane c owns column c of [D_i | B_i | I] (27 columns): the Gauss-Jordan elimination of that
// augmented block leaves Y_i in lanes 9..17 and D_i^-1 in lanes 18..26 -- the solve's own step (vba_solve_step.h) with nine identity
// right-hand sides in its idle lanes.  The pivot row is read with v_readlane (one system per wave: the row is uniform).  Y_i and
// D_i^-1 are kept in the two output arrays and overwritten by S_i,i+1 and S_ii in the backward sweep.
// The shadow front and the scratch are the scaffold every query shares (vba_query.hip); launch_cov_invert below is what it calls.
#include "vba_context.h"
#include "vba_cov_walk.h"

namespace vba {

// What a plain chain of n poses in n_rows rows leaves beside cov_chain's blocks: zero rows beyond n; NaN blocks (the super block of
// the last pose: zeros) if a pivot was zero or not finite -- numerically singular: no covariance.
__device__ void cov_pad_or_nan(unsigned fl, int n, int n_rows, double* Dw, double* Sw) {
    const int lane = threadIdx.x;
    for (int e = lane; e < (n_rows - n) * 81; e += 64) {
        Dw[(size_t)n * 81 + e] = 0.0;
        Sw[(size_t)n * 81 + e] = 0.0;
    }
    if (fl & (VBA_FLAG_ZERO_PIVOT | VBA_FLAG_NONFINITE)) {
        for (int e = lane; e < n * 81; e += 64) {
            Dw[e] = __builtin_nan("");
            Sw[e] = (e >= (n - 1) * 81) ? 0.0 : __builtin_nan("");
        }
    }
}

// Sequential path: one wavefront walks the whole chain of its window.  bands [W][n_max][243]; sc / par: the damping of the call the
// resident states feed; diag / sup [W][n_max][81]; flags [W].
// One wave per SIMD (as k_cov_sep): a walk is one chain of dependent steps, and the registers a second wave would need are worth more
// to it as loads in flight (measured: docs/NOTEBOOK.md section 7).
__attribute__((amdgpu_waves_per_eu(1, 1)))
__global__ __launch_bounds__(64) void k_cov_seq(const double* __restrict__ bands, const int* __restrict__ nw, int n_max,
                                                const WinScalars* __restrict__ sc, int par, int damped, double* diag, double* sup,
                                                unsigned* flags) {
    __shared__ CovLds<false> lds;
    const int w = blockIdx.x, n = nw[w];
    const double lam32 = damped ? (double)(float)sc[w].lam[par] : 0.0;     // torch.eye() is float32 (BA_filtering.py:54)
    double* Dw = diag + (size_t)w * n_max * 81;
    double* Sw = sup + (size_t)w * n_max * 81;
    const unsigned fl = cov_chain<false>(lds, bands + (size_t)w * n_max * 243, 0, n - 1, lam32, Dw, Sw);
    cov_pad_or_nan(fl, n, n_max, Dw, Sw);
    if (threadIdx.x == 0) flags[w] = fl;
}

// ---- partitioned path (latency-mode handles, chunked solver setting): the chain is cut into chunks of s poses whose last pose is a
// separator, as the partitioned solve cuts it.  With I the interior poses (block diagonal over chunks, T_c per chunk), S the
// separators and X = T^-1 A_IS:
//   Sigma_SS = (A_SS - A_SI X)^-1,  Sigma_IS = -X Sigma_SS,  Sigma_II = T^-1 + X Sigma_SS X^T
// Three launches behind the front: k_cov_chunk (one wave per chunk: T^-1's diagonal / super-diagonal blocks and X by the coupled
// form of cov_chain, the 18 coupling columns as right-hand sides in lanes 27..44, and the chunk's part of the separator Schur
// complement), k_cov_sep (one wave per window: the separator system assembled and walked by the plain form), k_cov_fix
// (one wave per chunk: T^-1 + X Sigma_SS X^T, the interior-separator blocks, the separators' own blocks).

// X [W][n_max][9][18] (left, right coupling columns); contrib [W][p_rows][3][81]: per chunk A_sL,first X_first[:, L], A_sR,last X_last[:, R],
// A_sL,first X_first[:, R]
__global__ __launch_bounds__(64) void k_cov_chunk(const double* __restrict__ bands, const int* __restrict__ nw, int n_max, int s,
                                                  const WinScalars* __restrict__ sc, int par, int damped, double* diag, double* sup,
                                                  double* X, double* contrib, int p_rows, unsigned* flags) {
    __shared__ CovLds<true> lds;
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
    const unsigned fl = cov_chain<true>(lds, bw, first, last, lam32, Dw, Sw, hasL, hasR, Xw);
    if (fl & (VBA_FLAG_ZERO_PIVOT | VBA_FLAG_NONFINITE)) {      // k_cov_fix writes the NaN blocks
        if (lane == 0) atomicOr(flags + w, fl);
        return;
    }
    // ---- this chunk's part of the separator Schur complement (Xn = x_first; x_last from memory)
    const double* Xn = lds.Xn;
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
__attribute__((amdgpu_waves_per_eu(1, 1)))
__global__ __launch_bounds__(64) void k_cov_sep(const double* __restrict__ bands, const int* __restrict__ nw, int n_max, int s,
                                                const WinScalars* __restrict__ sc, int par, int damped, const double* contrib,
                                                double* sepb, int p_rows, double* SSd, double* SSs, unsigned* flags) {
    __shared__ CovLds<false> lds;
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
    double* Dw = SSd + (size_t)w * p_rows * 81;
    double* Sw = SSs + (size_t)w * p_rows * 81;
    const unsigned fl = cov_chain<false>(lds, sb, 0, q - 1, 0.0, Dw, Sw);
    cov_pad_or_nan(fl, q, p_rows, Dw, Sw);
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
            int r, q;
            cov_tri(lane, r, q);
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

// The selected inversion of the system in V.bands into b's result arrays, behind the front on stream s.  The path follows the solver
// setting (vba_set_solver): a chunked solve is served by the partitioned path with the same chunks, the sequential walk by one wave
// per window.
int launch_cov_invert(vba_handle h, const DevView& V, const CovBufs& b, int damped, hipStream_t s) {
    const int s_chunk = h->V.chunk, PR = V.p_max;
    const size_t W = h->W;
    if (s_chunk >= 2) {
        const int pc = (h->n_max + s_chunk - 1) / s_chunk;
        HIPCHK(hipMemsetAsync(b.flags, 0, W * 4, s));
        hipLaunchKernelGGL(k_cov_chunk, dim3(pc, h->W), dim3(64), 0, s, V.bands, V.n, h->n_max, s_chunk, h->V.sc, h->par, damped ? 1 : 0,
                           b.diag, b.sup, b.X, b.contrib, PR, b.flags);
        hipLaunchKernelGGL(k_cov_sep, dim3(h->W), dim3(64), 0, s, V.bands, V.n, h->n_max, s_chunk, h->V.sc, h->par, damped ? 1 : 0,
                           b.contrib, b.sepb, PR, b.SSd, b.SSs, b.flags);
        hipLaunchKernelGGL(k_cov_fix, dim3(pc, h->W), dim3(64), 0, s, V.n, h->n_max, s_chunk, b.diag, b.sup, b.X, b.SSd, b.SSs, PR,
                           b.flags);
    } else {
        hipLaunchKernelGGL(k_cov_seq, dim3(h->W), dim3(64), 0, s, V.bands, V.n, h->n_max, h->V.sc, h->par, damped ? 1 : 0, b.diag, b.sup,
                           b.flags);
    }
    HIPCHK(hipGetLastError());
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
