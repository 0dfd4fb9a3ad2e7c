// vba_schur.hip -- free-landmark bundle adjustment with a Schur-complement solve (ADD-ON, PARITY UNPINNED).
//
// The reference keeps its landmarks fixed (estimation/BA/BA_filtering.py:32-37): every observation touches only the
// 6x6 block of its own pose and there is nothing to marginalise.  This file is the variant BASELINE.json's north_star
// describes on top of that: the landmarks become unknowns (3 each, held by a catalogue prior N(X0, sigma^2 I)), the
// normal equations
//        [ B   E ] [dc]   [v]        B: 6x6 per pose,   C: 3x3 per landmark,   E: 6x3 per observation
//        [ E^T C ] [dl] = [w]
// are reduced to the cameras,  S = B - E C^-1 E^T,  g = v - E C^-1 w,  the dense reduced camera system S dc = g is
// factorised on the matrix cores (blocked Cholesky, v_mfma_f64_16x16x4), and the landmarks follow by back substitution
// dl = C^-1 (w - E^T dc).  It has NO counterpart in the reference; it is checked against this repository's own CPU
// restatement (oracle/schur_oracle.py) only and never runs inside vba_iterate / BA().
//
// Reprojection and its pose Jacobian are the reference's (vba_math.h: BA_utils.py:30-49); the landmark Jacobian is
// d uv / d X = A R^T = -(translation part of the pose Jacobian).  Weights are the observation confidences (the
// reference's alpha = 2 case, BA_filtering.py:22-25, where the robust weight is constant) until vba_schur_reweight is called.
//
// Kernels (all reductions in a fixed order -- no float atomics):
//   k_lm_blocks     thread per landmark: C_l, w_l over its rows, C_l^-1, then E_k and Y_k = E_k C_l^-1 per row
//   k_pose_blocks   16 lanes per pose: B_i, v_i over its rows, g_i = v_i - sum Y_k w_l; diagonal block of S
//   k_pair_blocks   wave per (i, j) block of S: S_ij -= sum over the rows pairs sharing a landmark of Y_k E_k'^T
//   k_potrf64       64x64 diagonal block: Cholesky factor and its inverse (one workgroup, LDS)
//   k_gemm_abt      64x64x64 tiles on the matrix cores: panel = A inv(L)^T (MODE 0), trailing S_IJ -= L_I L_J^T (MODE 1)
//   k_trsv_step     one tile step of the forward / backward substitution (stored inverse diagonal factors), a launch per step
//   k_lm_update     dl, new landmarks, new poses (retraction as BA_filtering.py:56-60)
//   k_cost          sum w |r|^2 + prior, block partials
// Covariance query (vba_schur_covariance: build and factor into scratch of its own, then)
//   k_trinv_step    W = Lg^-1 on the matrix cores, a launch per tile distance from the diagonal, products beyond the band skipped
//   k_syrk_wtw      S^-1 = W^T W on the matrix cores, block per tile of the lower triangle
//   k_cov_gather    the listed 6x6 blocks of S^-1 (pair_cov) and its diagonal blocks (pose_cov)
//   k_lm_cov        thread per landmark: C_l^-1 + sum Y_k^T Sigma_{pose(k), pose(k')} Y_k'
// Reliability query (vba_schur_reliability: the device part of the covariance query, then)
//   k_rel_rows      thread per row: pose-landmark cross-covariance Sigma_il from the gathered blocks and Y, leverage and w-test
//   k_rel_stats     thread per landmark / per pose: their rows' statistics; the catalogue prior of a landmark as an observation
//   k_rel_totals    one block: cost, redundancy, variance factor, largest tests (strided partial sums, one tree)
// Data snooping (vba_schur_snoop: the device part of the reliability query, then the passes of vba_schur_snoop.hip)
// Robust re-weighting (vba_schur_reweight, vba_schur_median: the passes of vba_schur_robust.hip)
// Orbit-dynamics factor with velocity unknowns (vba_schur_enable_dynamics: the kernels of vba_schur_dyn.hip; the reduced system
// becomes [6 n pose | 3 n velocity] unknowns, the kernels of this file fill and factorise it unchanged)
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/vinsat_ba.h"
#include "vba_math.h"
#include "vba_schur_dyn.h"
#include "vba_schur_dyn_math.h"
#include "vba_schur_rel_math.h"
#include "vba_schur_robust.h"
#include "vba_schur_snoop.h"

namespace {

using namespace vba;

typedef double vf4 __attribute__((ext_vector_type(4)));

constexpr int kT = 64;              // tile of the blocked Cholesky
constexpr int kPanel = 4;           // tile columns per panel: the trailing update runs with K = kPanel * kT = 256 (round 4)

struct SchurView {
    int n, L;
    int64_t m;
    int N, Npad, nb;                // reduced system: N = 6 n (9 n with the dynamics factor), padded to a multiple of kT, nb tiles per side
    // rows sorted by landmark: CSR lm_ptr[L+1]
    const int* lm_ptr;
    const int* row_pose;            // [m]
    const int* row_lm;              // [m]
    const double *row_u, *row_v, *row_w;    // [m] measurement, weight
    // rows of a pose: CSR pose_ptr[n+1] -> pose_rows[m] (indices into the landmark-sorted rows)
    const int* pose_ptr;
    const int* pose_rows;
    // blocks (i >= j) of S that receive pair products: CSR blk_ptr[nblk+1] -> (pair_k, pair_k2); blk_i, blk_j
    int nblk;
    const int *blk_i, *blk_j, *blk_ptr, *pair_k, *pair_k2;
    const double* intr;             // [n][4]
    const double* X0;               // [L][3] catalogue positions
    double inv_sigma2;              // 1 / sigma_prior^2
    double lamda;
    // state
    const double* states;           // [n][10]
    const double* X;                // [L][3]
    double* states_new;
    double* X_new;
    // work
    double* Cinv;                   // [L][6] symmetric inverse (00,01,02,11,12,22)
    double* wl;                     // [L][3]
    double* E;                      // [m][18] row major 6x3
    double* Y;                      // [m][18]
    double* S;                      // [Npad][Npad] row major, lower triangle used
    double* g;                      // [Npad] right-hand side, then the step of the poses
    double* ybuf;                   // [Npad] intermediate of the two substitutions
    double* invL;                   // [nb][kT*kT] inverse of the diagonal Cholesky factors
    double* dl;                     // [L][3]
    double* part;                   // cost partials
    int npart;
};

// row k of the landmark-sorted rows: residual, A (d uv / d p_c), camera point, for pose / landmark state given
struct RowGeom {
    double ru, rv, a00, a02, a11, a12, cam[3];
    PoseCam pc;
};

__device__ __forceinline__ void row_geometry(const SchurView& V, const double* states, const double* X, int k, RowGeom& q) {
    const int i = V.row_pose[k], l = V.row_lm[k];
    pose_camera(states + (size_t)i * 10, V.intr + (size_t)i * 4, q.pc);
    double u, v, d;
    project(q.pc, X[3 * l], X[3 * l + 1], X[3 * l + 2], u, v, q.cam, d);
    q.ru = V.row_u[k] - u;
    q.rv = V.row_v[k] - v;
    const double live = q.cam[2] > kZMin ? 1.0 : 0.0;
    q.a00 = q.pc.fx * d;
    q.a11 = q.pc.fy * d;
    q.a02 = -(q.a00 * (q.cam[0] * d * live));
    q.a12 = -(q.a11 * (q.cam[1] * d * live));
}

// J_l = A R^T (2x3): row u -> jl[0..2], row v -> jl[3..5]
__device__ __forceinline__ void landmark_jacobian(const RowGeom& q, double* jl) {
    const double* R = q.pc.R;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        jl[c] = q.a00 * R[3 * c] + q.a02 * R[3 * c + 2];
        jl[3 + c] = q.a11 * R[3 * c + 1] + q.a12 * R[3 * c + 2];
    }
}

// J_c = [-J_l | 2 A hat(p_c)] (2x6): row u -> jc[0..5], row v -> jc[6..11]
__device__ __forceinline__ void pose_jacobian(const RowGeom& q, const double* jl, double* jc) {
    const double x = q.cam[0], y = q.cam[1], z = q.cam[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) { jc[c] = -jl[c]; jc[6 + c] = -jl[3 + c]; }
    jc[3] = 2.0 * (-q.a02 * y);
    jc[4] = 2.0 * (-q.a00 * z + q.a02 * x);
    jc[5] = 2.0 * (q.a00 * y);
    jc[9] = 2.0 * (q.a11 * z - q.a12 * y);
    jc[10] = 2.0 * (q.a12 * x);
    jc[11] = 2.0 * (-q.a11 * x);
}

// ------------------------------------------------------------------------------------------------ landmark side
__global__ __launch_bounds__(256) void k_lm_blocks(SchurView V) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= V.L) return;
    const int beg = V.lm_ptr[l], end = V.lm_ptr[l + 1];
    double C[6] = {0, 0, 0, 0, 0, 0}, w3[3] = {0, 0, 0};
    for (int k = beg; k < end; ++k) {
        RowGeom q;
        row_geometry(V, V.states, V.X, k, q);
        double jl[6];
        landmark_jacobian(q, jl);
        const double w = V.row_w[k];
        int e = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int b = a; b < 3; ++b) { C[e] = fma(w * jl[a], jl[b], fma(w * jl[3 + a], jl[3 + b], C[e])); ++e; }
            w3[a] = fma(w * jl[a], q.ru, fma(w * jl[3 + a], q.rv, w3[a]));
        }
    }
    const double dg = V.inv_sigma2 + V.lamda;
    C[0] += dg; C[3] += dg; C[5] += dg;
#pragma unroll
    for (int a = 0; a < 3; ++a) w3[a] -= V.inv_sigma2 * (V.X[3 * l + a] - V.X0[3 * l + a]);
    // inverse of the symmetric 3x3 by cofactors
    const double c00 = C[0], c01 = C[1], c02 = C[2], c11 = C[3], c12 = C[4], c22 = C[5];
    const double m00 = c11 * c22 - c12 * c12, m01 = c02 * c12 - c01 * c22, m02 = c01 * c12 - c02 * c11;
    const double det = c00 * m00 + c01 * m01 + c02 * m02;
    const double id = 1.0 / det;
    double Ci[6] = {m00 * id, m01 * id, m02 * id, (c00 * c22 - c02 * c02) * id, (c01 * c02 - c00 * c12) * id, (c00 * c11 - c01 * c01) * id};
#pragma unroll
    for (int e = 0; e < 6; ++e) V.Cinv[(size_t)l * 6 + e] = Ci[e];
#pragma unroll
    for (int a = 0; a < 3; ++a) V.wl[(size_t)l * 3 + a] = w3[a];
    const double Cm[3][3] = {{Ci[0], Ci[1], Ci[2]}, {Ci[1], Ci[3], Ci[4]}, {Ci[2], Ci[4], Ci[5]}};
    for (int k = beg; k < end; ++k) {
        RowGeom q;
        row_geometry(V, V.states, V.X, k, q);
        double jl[6], jc[12];
        landmark_jacobian(q, jl);
        pose_jacobian(q, jl, jc);
        const double w = V.row_w[k];
        double* Ek = V.E + (size_t)k * 18;
        double* Yk = V.Y + (size_t)k * 18;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            double e3[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) e3[c] = w * (jc[a] * jl[c] + jc[6 + a] * jl[3 + c]);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                Ek[3 * a + c] = e3[c];
                Yk[3 * a + c] = e3[0] * Cm[0][c] + e3[1] * Cm[1][c] + e3[2] * Cm[2][c];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ pose side
// 16 lanes per pose: lane t < 16 strides over the pose's rows, 21 + 6 + 6 partial sums, xor butterfly over the 16 lanes
__global__ __launch_bounds__(256) void k_pose_blocks(SchurView V) {
    const int i = blockIdx.x * 16 + (threadIdx.x >> 4);
    const int l16 = threadIdx.x & 15;
    double acc[33];
#pragma unroll
    for (int q = 0; q < 33; ++q) acc[q] = 0.0;
    if (i < V.n) {
        const int beg = V.pose_ptr[i], end = V.pose_ptr[i + 1];
        for (int r = beg + l16; r < end; r += 16) {
            const int k = V.pose_rows[r];
            RowGeom q;
            row_geometry(V, V.states, V.X, k, q);
            double jl[6], jc[12];
            landmark_jacobian(q, jl);
            pose_jacobian(q, jl, jc);
            const double w = V.row_w[k];
            int e = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                const double ja = w * jc[a], jb = w * jc[6 + a];
#pragma unroll
                for (int b = a; b < 6; ++b) { acc[e] = fma(ja, jc[b], fma(jb, jc[6 + b], acc[e])); ++e; }
                acc[21 + a] = fma(ja, q.ru, fma(jb, q.rv, acc[21 + a]));
            }
            // g_i -= Y_k w_l
            const double* Yk = V.Y + (size_t)k * 18;
            const double* wl = V.wl + (size_t)V.row_lm[k] * 3;
#pragma unroll
            for (int a = 0; a < 6; ++a) acc[27 + a] = fma(Yk[3 * a], wl[0], fma(Yk[3 * a + 1], wl[1], fma(Yk[3 * a + 2], wl[2], acc[27 + a])));
        }
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) {
#pragma unroll
        for (int q = 0; q < 33; ++q) acc[q] += __shfl_xor(acc[q], off, 64);
    }
    if (i < V.n && l16 == 0) {
        double* Sd = V.S + (size_t)(6 * i) * V.Npad + 6 * i;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = 0; b <= a; ++b) Sd[(size_t)a * V.Npad + b] = acc[sym6(b, a)] + (a == b ? V.lamda : 0.0);
#pragma unroll
        for (int a = 0; a < 6; ++a) V.g[6 * i + a] = acc[21 + a] - acc[27 + a];
    }
}

// S_ij -= sum_{(k, k')} Y_k E_k'^T over the row pairs (k of pose i, k' of pose j) that share a landmark; one wave per block,
// lane t < 36 owns entry (t / 6, t % 6); the pair list is walked in a fixed order
__global__ __launch_bounds__(64) void k_pair_blocks(SchurView V) {
    const int bq = blockIdx.x;
    if (bq >= V.nblk) return;
    const int i = V.blk_i[bq], j = V.blk_j[bq];
    const int t = threadIdx.x;
    const int a = t / 6, b = t % 6;
    double s = 0.0;
    if (t < 36) {
        for (int p = V.blk_ptr[bq]; p < V.blk_ptr[bq + 1]; ++p) {
            const double* Yk = V.Y + (size_t)V.pair_k[p] * 18 + 3 * a;
            const double* Ek = V.E + (size_t)V.pair_k2[p] * 18 + 3 * b;
            s = fma(Yk[0], Ek[0], fma(Yk[1], Ek[1], fma(Yk[2], Ek[2], s)));
        }
        if (i != j || b <= a) V.S[(size_t)(6 * i + a) * V.Npad + 6 * j + b] -= s;
    }
}

// padding rows of the reduced system (N up to the next multiple of the tile): identity, so the factorisation runs on whole tiles
__global__ void k_pad_identity(SchurView V) {
    const int r = V.N + blockIdx.x * 64 + threadIdx.x;      // (grid: enough blocks of 64 for the padding rows)
    if (r < V.Npad) V.S[(size_t)r * V.Npad + r] = 1.0;
}

// ------------------------------------------------------------------------------------------------ dense Cholesky
// Diagonal tile kb: A_kk = L L^T in place (lower), inverse of L into invL[kb] (row major, lower).  ONE WAVE, the tile in
// registers: lane r holds row r (64 doubles); column j is scaled and the rank-1 update of the rows below runs with the
// column entries broadcast from their lanes (v_readlane) -- no LDS, no barrier (the LDS version spent its 130 us in 192
// workgroup barriers).  The inverse (needed so that the panel solve is a matrix product for the matrix cores) follows the
// same way: lane c owns column c of L^-1, the entries L[r][k] are broadcast.
__device__ __forceinline__ double bcast64(double v, int lane) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)b, lane);
    const unsigned hi = __builtin_amdgcn_readlane((unsigned)(b >> 32), lane);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__global__ __launch_bounds__(64) void k_potrf64(SchurView V, int kb, int* info) {
    const int r = threadIdx.x;
    double* At = V.S + (size_t)(kb * kT) * V.Npad + kb * kT;
    double a[kT];
#pragma unroll
    for (int c = 0; c < kT; ++c) a[c] = At[(size_t)r * V.Npad + c];     // (the upper part is never used)
    int bad = -1;                   // first column with a non-positive pivot (the same in every lane)
#pragma unroll
    for (int j = 0; j < kT; ++j) {
        const double d = bcast64(a[j], j);
        if (!(d > 0.0) && bad < 0) bad = j;
        const double sd = sqrt(d > 0.0 ? d : 1.0), isd = 1.0 / sd;
        a[j] = r == j ? sd : a[j] * isd;            // column j: L[r][j] for r > j (rows above j hold garbage there, never read)
#pragma unroll
        for (int c = j + 1; c < kT; ++c) a[c] = fma(-a[j], bcast64(a[j], c), a[c]);     // A[r][c] -= L[r][j] L[c][j]; used for r >= c
    }
    // the FIRST failing row of the whole factorisation stays on record: the tile launches are ordered on one stream, and only
    // that pivot means anything (later ones follow a pivot replaced by 1)
    if (bad >= 0 && r == 0 && *info == 0) *info = kb * kT + bad + 1;
#pragma unroll
    for (int c = 0; c < kT; ++c)
        if (c <= r) At[(size_t)r * V.Npad + c] = a[c];
    // inverse: lane c owns column c of X = L^-1 (x[k] = X[k][c]); X[rr][c] = (delta - sum_{k < rr} L[rr][k] X[k][c]) / L[rr][rr]
    double x[kT];
#pragma unroll
    for (int rr = 0; rr < kT; ++rr) {
        double s = rr == r ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < rr; ++k) s = fma(-bcast64(a[k], rr), x[k], s);
        x[rr] = s / bcast64(a[rr], rr);
    }
    double* out = V.invL + (size_t)kb * kT * kT;
#pragma unroll
    for (int rr = 0; rr < kT; ++rr) out[(size_t)rr * kT + r] = r <= rr ? x[rr] : 0.0;
}

// The same tile factorisation BLOCKED (round 4): four block columns of 16.  Only the 16 x 16 diagonal blocks are factorised
// and inverted element by element (one wave, row per lane, 16 steps each instead of 64); the panel below a diagonal block, the
// update of the tile's remaining blocks and the assembly of the full inverse (block lower triangular: X_jj = W_j,
// X_ij = -W_i sum_k L_ik X_kj) are 16 x 16 x 16 products on the matrix cores, the tile living in LDS.  256 threads; the
// chain of tile factorisations is the critical path of the whole Cholesky once the trailing update runs at K = 256 beside it.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}
// acc += A B^T (bt = true: b feeds B[lr][k]) or A B (bt = false: b feeds B[k][lr]); 16 x 16 blocks in LDS with leading dimension ld
__device__ __forceinline__ vf4 mm16(vf4 acc, const double* A, const double* B, int ld, bool bt, int lr, int lk) {
#pragma unroll
    for (int sidx = 0; sidx < 4; ++sidx) {
        const int k = 4 * sidx + lk;
        const double a = A[lr * ld + k];
        const double b = bt ? B[lr * ld + k] : B[k * ld + lr];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
    return acc;
}

__global__ __launch_bounds__(256) void k_potrf64b(SchurView V, int kb, int* info) {
    constexpr int LD = kT + 1;
    __shared__ double T[kT * LD];           // the tile, then its factor (lower)
    __shared__ double X[kT * LD];           // its inverse (lower)
    __shared__ double Y[4][16 * 17];        // per wave: an intermediate product
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, lr = lane & 15, lk = lane >> 4;
    double* At = V.S + (size_t)(kb * kT) * V.Npad + kb * kT;
    for (int e = t; e < kT * kT; e += 256) {
        const int r = e >> 6, c = e & 63;
        T[r * LD + c] = At[(size_t)r * V.Npad + c];
        X[r * LD + c] = 0.0;
    }
    __syncthreads();
    int bad_row = -1;               // wave 0: first row of this tile with a non-positive pivot
    for (int jb = 0; jb < 4; ++jb) {
        const int o = 16 * jb;
        if (wv == 0) {      // diagonal block: factor and inverse, row per lane (lanes 16 .. 63 ride along on an identity)
            const int r = lane;
            double a[16], x[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) a[c] = r < 16 ? T[(o + r) * LD + o + c] : (c == (r & 15) ? 1.0 : 0.0);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const double d = bcast64(a[j], j);
                if (!(d > 0.0) && bad_row < 0) bad_row = o + j;
                const double sd = sqrt(d > 0.0 ? d : 1.0), isd = 1.0 / sd;
                a[j] = r == j ? sd : a[j] * isd;
#pragma unroll
                for (int c = j + 1; c < 16; ++c) a[c] = fma(-a[j], bcast64(a[j], c), a[c]);
            }
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                double sacc = rr == r ? 1.0 : 0.0;
#pragma unroll
                for (int k = 0; k < rr; ++k) sacc = fma(-bcast64(a[k], rr), x[k], sacc);
                x[rr] = sacc / bcast64(a[rr], rr);
            }
            if (r < 16) {
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    T[(o + r) * LD + o + c] = c <= r ? a[c] : 0.0;
                    X[(o + c) * LD + o + r] = r <= c ? x[c] : 0.0;      // x[c] = X[c][r] of this block (lane r owns column r)
                }
            }
        }
        __syncthreads();
        // panel below: L_i,jb = A_i,jb W^T, one row tile per wave
        if (wv < 3 - jb) {
            const int i = jb + 1 + wv;
            double* Aij = T + (16 * i) * LD + o;
            vf4 acc = (vf4){0.0, 0.0, 0.0, 0.0};
            acc = mm16(acc, Aij, X + o * LD + o, LD, true, lr, lk);
            wave_lds_sync();        // (all operands of this wave are read before it overwrites its own tile)
#pragma unroll
            for (int q = 0; q < 4; ++q) Aij[(lk + 4 * q) * LD + lr] = acc[q];
        }
        __syncthreads();
        // the tile's remaining blocks: A_ik -= L_i,jb L_k,jb^T for jb < k <= i
        {
            int q = 0;
            for (int i = jb + 1; i < 4; ++i)
                for (int k = jb + 1; k <= i; ++k, ++q) {
                    if ((q & 3) != wv) continue;
                    vf4 acc = (vf4){0.0, 0.0, 0.0, 0.0};
                    acc = mm16(acc, T + (16 * i) * LD + o, T + (16 * k) * LD + o, LD, true, lr, lk);
                    double* C = T + (16 * i) * LD + 16 * k;
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq) C[(lk + 4 * qq) * LD + lr] -= acc[qq];
                }
        }
        __syncthreads();
    }
    // the inverse below its diagonal blocks, by distance from the diagonal: X_ij = -W_i (sum_{k = j}^{i-1} L_ik X_kj)
    for (int dist = 1; dist < 4; ++dist) {
        if (wv < 4 - dist) {
            const int j = wv, i = j + dist;
            vf4 acc = (vf4){0.0, 0.0, 0.0, 0.0};
            for (int k = j; k < i; ++k) acc = mm16(acc, T + (16 * i) * LD + 16 * k, X + (16 * k) * LD + 16 * j, LD, false, lr, lk);
#pragma unroll
            for (int q = 0; q < 4; ++q) Y[wv][(lk + 4 * q) * 17 + lr] = acc[q];
            wave_lds_sync();
            vf4 acc2 = (vf4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int sidx = 0; sidx < 4; ++sidx) {
                const int k = 4 * sidx + lk;
                acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(X[(16 * i + lr) * LD + 16 * i + k], Y[wv][k * 17 + lr], acc2, 0, 0, 0);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) X[(16 * i + lk + 4 * q) * LD + 16 * j + lr] = -acc2[q];
        }
        __syncthreads();
    }
    if (t == 0 && bad_row >= 0 && *info == 0) *info = kb * kT + bad_row + 1;       // (the first failing row stays, as in k_potrf64)
    double* out = V.invL + (size_t)kb * kT * kT;
    for (int e = t; e < kT * kT; e += 256) {
        const int r = e >> 6, c = e & 63;
        if (c <= r) At[(size_t)r * V.Npad + c] = T[r * LD + c];
        out[e] = c <= r ? X[r * LD + c] : 0.0;
    }
}

// One 64x64 tile of  out = alpha * (C + sign * A B^T)  on the matrix cores.  A, B: 64x64 row major with leading dimension
// lda / ldb.  256 threads = 4 waves, wave wv owns the 32x32 quadrant (wv >> 1, wv & 1) = 2x2 MFMA tiles of 16x16, K = 64
// in 16 steps of 4.  v_mfma_f64_16x16x4: lane l feeds A[l & 15][4 s + (l >> 4)] and B^T[4 s + (l >> 4)][l & 15] = B[l & 15][..]
// and owns C[(l >> 4) + 4 i][l & 15], i = 0..3.  Both operand tiles are staged in LDS first (which also makes the in-place
// panel form safe).
//   MODE 0 (panel):    S_{I,kb} <- S_{I,kb} invL_kb^T              grid = tiles I > kb
//   MODE 1 (trailing): S_{I,J}  -= S_{I,kb} S_{J,kb}^T             grid = tiles kb < J <= I
//   MODE 2 (inside a panel): as MODE 1 for the tile columns kb < J <= jhi only, grid = (rows I >= kb + 1, those columns)
template <int MODE>
__global__ __launch_bounds__(256) void k_gemm_abt(SchurView V, int kb, int jhi = 0) {
    __shared__ double As[kT][kT + 1];
    __shared__ double Bs[kT][kT + 1];
    const int t = threadIdx.x;
    int I, J;
    if (MODE == 0) {
        I = kb + 1 + blockIdx.x;
        J = kb;
    } else if (MODE == 2) {
        I = kb + 1 + blockIdx.x;
        J = kb + 1 + blockIdx.y;
        if (J > jhi || I < J) return;
    } else {        // blockIdx.x enumerates the lower triangle of the (nb - kb - 1)^2 trailing tiles
        const int q = blockIdx.x;
        int r = (int)((sqrt(8.0 * q + 1.0) - 1.0) * 0.5);
        while ((r + 1) * (r + 2) / 2 <= q) ++r;
        while (r * (r + 1) / 2 > q) --r;
        const int c = q - r * (r + 1) / 2;
        I = kb + 1 + r;
        J = kb + 1 + c;
    }
    const double* Ap = V.S + (size_t)(I * kT) * V.Npad + kb * kT;
    const double* Bp = MODE == 0 ? V.invL + (size_t)kb * kT * kT : V.S + (size_t)(J * kT) * V.Npad + kb * kT;
    const int ldb = MODE == 0 ? kT : V.Npad;
    for (int e = t; e < kT * kT; e += 256) {
        const int r = e / kT, c = e % kT;
        As[r][c] = Ap[(size_t)r * V.Npad + c];
        Bs[r][c] = Bp[(size_t)r * ldb + c];
    }
    __syncthreads();
    const int lane = t & 63, wv = t >> 6;
    const int r0 = (wv >> 1) * 32, c0 = (wv & 1) * 32;
    const int lr = lane & 15, lk = lane >> 4;
    vf4 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = (vf4){0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int s = 0; s < kT / 4; ++s) {
        const int k = 4 * s + lk;
        const double a0 = As[r0 + lr][k], a1 = As[r0 + 16 + lr][k];
        const double b0 = Bs[c0 + lr][k], b1 = Bs[c0 + 16 + lr][k];
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    double* Cp = MODE == 0 ? V.S + (size_t)(I * kT) * V.Npad + kb * kT : V.S + (size_t)(I * kT) * V.Npad + J * kT;
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = r0 + 16 * x + lk + 4 * i, c = c0 + 16 * y + lr;
                double* p = Cp + (size_t)r * V.Npad + c;
                if (MODE == 0) *p = acc[x][y][i];
                else if (I != J || c <= r) *p -= acc[x][y][i];
            }
}

// Trailing update of a whole PANEL of kPanel tile columns (round 4): S_{I,J} -= sum_{k in panel} S_{I,k} S_{J,k}^T with K = 256 per
// launch.  With K = 64 every 64 x 64 tile of the trailing matrix was read and written once per 64 columns -- 4 flop per byte,
// the update ran at the speed of memory (13.9 TFLOP/s = 3.5 TB/s); here a block owns 128 x 128 of C and walks K = 256 in
// chunks of 32 through LDS (16 x the arithmetic per byte of C, 2 x per byte of the operands); the next chunk's operands are
// requested from memory before the current chunk's matrix operations are issued.  Grid: (128-row blocks from the first trailing one, 128-column
// blocks [cj_lo, cj_hi]); blocks above the diagonal leave at once, diagonal blocks store their lower triangle.
#ifndef VBA_SYRK_CHUNK
#define VBA_SYRK_CHUNK 16
#endif
constexpr int kSyrkChunk = VBA_SYRK_CHUNK;
// (four waves per SIMD: two blocks per compute unit, one computes while the other stages, waits at a barrier or updates C)
__global__ __launch_bounds__(512, 4) void k_syrk_panel(SchurView V, int kb0, int b0, int cj_lo) {
    __shared__ double As[128][kSyrkChunk + 1];
    __shared__ double Bs[128][kSyrkChunk + 1];
    const int bi = b0 + (int)blockIdx.x, bj = cj_lo + (int)blockIdx.y;
    if (bi < bj) return;
    // 512 threads = 8 waves, wave wv owns 64 rows x 32 columns of the block (4 x 2 matrix-core tiles, 8 accumulators: two waves
    // per SIMD fit, one covers the other's LDS round trips and barriers -- with 64 x 64 per wave and one wave per SIMD the
    // matrix pipe was busy a quarter of the time)
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    const int r0 = (wv >> 2) * 64, c0 = (wv & 3) * 32;
    const size_t ld = (size_t)V.Npad;
    const double* Ap = V.S + (size_t)(bi * 128) * ld + (size_t)kb0 * kT;
    const double* Bp = V.S + (size_t)(bj * 128) * ld + (size_t)kb0 * kT;
    constexpr int K = kPanel * kT, NK = K / kSyrkChunk;
    // staging: 128 rows x kSyrkChunk columns per operand and chunk = 64 kSyrkChunk double2 / 512 threads = kSyrkChunk / 8 each
    constexpr int NS = kSyrkChunk / 8, C2 = kSyrkChunk / 2;       // double2 per thread; double2 per row
    double2 pa[NS], pb[NS];
    auto fetch = [&](int kc) {
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const int e = t + 512 * i, row = e / C2, c2 = (e % C2) * 2;
            pa[i] = *reinterpret_cast<const double2*>(Ap + (size_t)row * ld + kc * kSyrkChunk + c2);
            pb[i] = *reinterpret_cast<const double2*>(Bp + (size_t)row * ld + kc * kSyrkChunk + c2);
        }
    };
    vf4 acc[4][2];
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = (vf4){0.0, 0.0, 0.0, 0.0};
    fetch(0);
    for (int kc = 0; kc < NK; ++kc) {
        __syncthreads();            // the matrix operations of the previous chunk have read their operands
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const int e = t + 512 * i, row = e / C2, c2 = (e % C2) * 2;
            As[row][c2] = pa[i].x; As[row][c2 + 1] = pa[i].y;
            Bs[row][c2] = pb[i].x; Bs[row][c2 + 1] = pb[i].y;
        }
        __syncthreads();
        if (kc + 1 < NK) fetch(kc + 1);
#pragma unroll
        for (int sidx = 0; sidx < kSyrkChunk / 4; ++sidx) {
            const int k = 4 * sidx + lk;
            double a[4], b[2];
#pragma unroll
            for (int x = 0; x < 4; ++x) a[x] = As[r0 + 16 * x + lr][k];
#pragma unroll
            for (int y = 0; y < 2; ++y) b[y] = Bs[c0 + 16 * y + lr][k];
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y) acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[x], b[y], acc[x][y], 0, 0, 0);
        }
    }
    double* Cp = V.S + (size_t)(bi * 128) * ld + (size_t)bj * 128;
    const bool diag = bi == bj;
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = r0 + 16 * x + lk + 4 * i, c = c0 + 16 * y + lr;
                if (!diag || c <= r) Cp[(size_t)r * ld + c] -= acc[x][y][i];
            }
}

// One tile step of the forward (L y = g) / backward (L^T x = y) substitution, a launch per step (as the factorisation):
// block 0 forms the step's 64 solution entries from the stored inverse diagonal factor, every other block forms them too
// (a 64x64 product, cheaper than a hand-off) and updates ONE tile of the right-hand side with them.  Tiles further than bw
// from the diagonal are zero (the factor of a banded matrix keeps its band) and get no block.
//   forward:  y_kb = invL_kb g_kb (-> ybuf),  g_I    -= L_{I,kb}   y_kb   for kb < I <= kb + bw
//   backward: x_kb = invL_kb^T ybuf_kb (-> g), ybuf_J -= L_{kb,J}^T x_kb   for kb - bw <= J < kb
__global__ __launch_bounds__(256) void k_trsv_step(SchurView V, int kb, int backward) {
    __shared__ double xb[kT];
    __shared__ double gb[kT];
    __shared__ double part[4][kT];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const double* Li = V.invL + (size_t)kb * kT * kT;
    const double* rhs = backward ? V.ybuf : V.g;
    if (t < kT) gb[t] = rhs[kb * kT + t];
    __syncthreads();
    for (int e = wv; e < kT; e += 4) {      // entry e: a 64-term dot product by one wave
        double sdot = backward ? Li[(size_t)lane * kT + e] * gb[lane] : Li[(size_t)e * kT + lane] * gb[lane];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sdot += __shfl_xor(sdot, o, 64);
        if (lane == 0) xb[e] = sdot;
    }
    __syncthreads();
    if (blockIdx.x == 0) {
        if (t < kT) (backward ? V.g : V.ybuf)[kb * kT + t] = xb[t];
        return;
    }
    if (!backward) {
        const int I = kb + (int)blockIdx.x;
        // rows of the tile over the waves, lanes over its columns (64 consecutive doubles per load)
        for (int rr = wv; rr < kT; rr += 4) {
            const size_t row = (size_t)I * kT + rr;
            double sdot = V.S[row * V.Npad + kb * kT + lane] * xb[lane];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) sdot += __shfl_xor(sdot, o, 64);
            if (lane == 0) V.g[row] -= sdot;
        }
    } else {
        const int J = kb - (int)blockIdx.x;
        // lanes over the tile's columns (= entries of ybuf_J), the 64 rows split over the waves, partial sums through LDS
        double sdot = 0.0;
        for (int c = wv; c < kT; c += 4) sdot = fma(V.S[(size_t)(kb * kT + c) * V.Npad + J * kT + lane], xb[c], sdot);
        part[wv][lane] = sdot;
        __syncthreads();
        if (wv == 0) V.ybuf[J * kT + lane] -= ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
    }
}

// ------------------------------------------------------------------------------------------------ update / cost
__global__ __launch_bounds__(256) void k_lm_update(SchurView V) {
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id < V.L) {
        const int l = id;
        double s[3] = {V.wl[3 * l], V.wl[3 * l + 1], V.wl[3 * l + 2]};
        for (int k = V.lm_ptr[l]; k < V.lm_ptr[l + 1]; ++k) {
            const double* Ek = V.E + (size_t)k * 18;
            const double* dc = V.g + 6 * V.row_pose[k];
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int a = 0; a < 6; ++a) s[c] -= Ek[3 * a + c] * dc[a];
        }
        const double* Ci = V.Cinv + (size_t)l * 6;
        const double d0 = Ci[0] * s[0] + Ci[1] * s[1] + Ci[2] * s[2];
        const double d1 = Ci[1] * s[0] + Ci[3] * s[1] + Ci[4] * s[2];
        const double d2 = Ci[2] * s[0] + Ci[4] * s[1] + Ci[5] * s[2];
        V.dl[3 * l] = d0; V.dl[3 * l + 1] = d1; V.dl[3 * l + 2] = d2;
        V.X_new[3 * l] = V.X[3 * l] + d0;
        V.X_new[3 * l + 1] = V.X[3 * l + 1] + d1;
        V.X_new[3 * l + 2] = V.X[3 * l + 2] + d2;
    }
    if (id < V.n) {
        const double* dc = V.g + 6 * id;
        const double d9[9] = {dc[0], dc[1], dc[2], dc[3], dc[4], dc[5], 0.0, 0.0, 0.0};
        double o[10];
        retract(V.states + (size_t)id * 10, d9, o);
#pragma unroll
        for (int r = 0; r < 10; ++r) V.states_new[(size_t)id * 10 + r] = o[r];
    }
}

// cost at (states, X) given as arguments: sum w (ru^2 + rv^2) over rows + inv_sigma2 |X - X0|^2 over landmarks
__global__ __launch_bounds__(256) void k_cost(SchurView V, const double* states, const double* X) {
    __shared__ double red[4];
    const int id = blockIdx.x * 256 + threadIdx.x;
    double s = 0.0;
    if (id < V.m) {
        RowGeom q;
        row_geometry(V, states, X, id, q);
        s = V.row_w[id] * (q.ru * q.ru + q.rv * q.rv);
    }
    if (id < V.L) {
        const double dx = X[3 * id] - V.X0[3 * id], dy = X[3 * id + 1] - V.X0[3 * id + 1], dz = X[3 * id + 2] - V.X0[3 * id + 2];
        s += V.inv_sigma2 * (dx * dx + dy * dy + dz * dz);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) V.part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// ------------------------------------------------------------------------------------------------ covariance query
// vba_schur_covariance: S^-1 = W^T W with W = Lg^-1, over the nbu = ceil(N / kT) tiles that hold unknowns (the tiles of nothing
// but padding are never touched; inside the last used tile the padding rows of W are rows of the identity and meet the columns
// < N with exact zeros).  W and the result are [Npad][Npad] row major like S, lower tile triangle.
//
// acc += op(A) B for 64x64 tiles staged in LDS, in the fragment layout of k_gemm_abt (wave quadrant r0 / c0, lane lr / lk):
// TA = false reads A[r][k], TA = true reads A[k][r] (A^T B); B is read as B[k][c].
template <bool TA>
__device__ __forceinline__ void tile_mma(vf4 (&acc)[2][2], const double (*As)[kT + 1], const double (*Bs)[kT + 1], int r0, int c0, int lr, int lk) {
#pragma unroll 4
    for (int s = 0; s < kT / 4; ++s) {
        const int k = 4 * s + lk;
        const double a0 = TA ? As[k][r0 + lr] : As[r0 + lr][k], a1 = TA ? As[k][r0 + 16 + lr] : As[r0 + 16 + lr][k];
        const double b0 = Bs[k][c0 + lr], b1 = Bs[k][c0 + 16 + lr];
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
}

__device__ __forceinline__ void tile_stage(double (*Ts)[kT + 1], const double* src, size_t ld, int t) {
    for (int e = t; e < kT * kT; e += 256) Ts[e / kT][e % kT] = src[(size_t)(e / kT) * ld + e % kT];
}

// The tiles at distance d below the diagonal of W = Lg^-1, a launch per distance (every tile of a launch reads tiles of smaller
// distances only): W_JJ = invL_J,  W_IJ = -invL_I sum_{K = max(J, I - bw)}^{I - 1} L_IK W_KJ  for I = J + d; block J.  The factor
// of a banded matrix keeps its band, so L_IK = 0 for I - K > bw and those products are skipped (as k_trsv_step skips them); W
// itself is full below the diagonal.  K runs upwards: one fixed order.
__global__ __launch_bounds__(256) void k_trinv_step(SchurView V, double* W, int d, int bw) {
    __shared__ double As[kT][kT + 1];
    __shared__ double Bs[kT][kT + 1];
    const int t = threadIdx.x, J = blockIdx.x, I = J + d;
    const size_t ld = (size_t)V.Npad;
    double* Wij = W + (size_t)(I * kT) * ld + (size_t)J * kT;
    if (d == 0) {
        const double* Li = V.invL + (size_t)J * kT * kT;
        for (int e = t; e < kT * kT; e += 256) Wij[(size_t)(e / kT) * ld + e % kT] = Li[e];
        return;
    }
    const int lane = t & 63, wv = t >> 6, r0 = (wv >> 1) * 32, c0 = (wv & 1) * 32, lr = lane & 15, lk = lane >> 4;
    vf4 acc[2][2], out[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = out[x][y] = (vf4){0.0, 0.0, 0.0, 0.0};
    for (int K = max(J, I - bw); K < I; ++K) {
        tile_stage(As, V.S + (size_t)(I * kT) * ld + (size_t)K * kT, ld, t);
        tile_stage(Bs, W + (size_t)(K * kT) * ld + (size_t)J * kT, ld, t);
        __syncthreads();
        tile_mma<false>(acc, As, Bs, r0, c0, lr, lk);
        __syncthreads();
    }
    tile_stage(As, V.invL + (size_t)I * kT * kT, kT, t);
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int i = 0; i < 4; ++i) Bs[r0 + 16 * x + lk + 4 * i][c0 + 16 * y + lr] = acc[x][y][i];
    __syncthreads();
    tile_mma<false>(out, As, Bs, r0, c0, lr, lk);
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int i = 0; i < 4; ++i) Wij[(size_t)(r0 + 16 * x + lk + 4 * i) * ld + c0 + 16 * y + lr] = -out[x][y][i];
}

// Tile (I, J), I >= J, of S^-1 = W^T W:  sum_{K = I}^{nbu - 1} W_KI^T W_KJ  (W_KI = 0 above the diagonal), K upwards, one block per
// tile of the lower triangle (enumerated as k_gemm_abt<1> does); diagonal tiles are stored whole.  out may be the array the factor
// lived in: W is all this kernel reads.
__global__ __launch_bounds__(256) void k_syrk_wtw(SchurView V, const double* W, double* out, int nbu) {
    __shared__ double As[kT][kT + 1];
    __shared__ double Bs[kT][kT + 1];
    const int t = threadIdx.x, q = blockIdx.x;
    int I = (int)((sqrt(8.0 * q + 1.0) - 1.0) * 0.5);
    while ((I + 1) * (I + 2) / 2 <= q) ++I;
    while (I * (I + 1) / 2 > q) --I;
    const int J = q - I * (I + 1) / 2;
    const size_t ld = (size_t)V.Npad;
    const int lane = t & 63, wv = t >> 6, r0 = (wv >> 1) * 32, c0 = (wv & 1) * 32, lr = lane & 15, lk = lane >> 4;
    vf4 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = (vf4){0.0, 0.0, 0.0, 0.0};
    for (int K = I; K < nbu; ++K) {
        tile_stage(As, W + (size_t)(K * kT) * ld + (size_t)I * kT, ld, t);
        tile_stage(Bs, W + (size_t)(K * kT) * ld + (size_t)J * kT, ld, t);
        __syncthreads();
        tile_mma<true>(acc, As, Bs, r0, c0, lr, lk);
        __syncthreads();
    }
    double* Cp = out + (size_t)(I * kT) * ld + (size_t)J * kT;
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int i = 0; i < 4; ++i) Cp[(size_t)(r0 + 16 * x + lk + 4 * i) * ld + c0 + 16 * y + lr] = acc[x][y][i];
}

// The listed 6x6 blocks (i >= j) of S^-1 in block-list order, thread per entry; a diagonal block is read from its lower triangle
// and mirrored, and goes to pose[i] as well (the same values: bitwise equal).
__global__ __launch_bounds__(256) void k_cov_gather(SchurView V, const double* Sinv, double* pair, double* pose) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= (int64_t)V.nblk * 36) return;
    const int b = (int)(id / 36), e = (int)(id % 36), a = e / 6, c = e % 6;
    const int i = V.blk_i[b], j = V.blk_j[b];
    const int r = i == j ? 6 * i + max(a, c) : 6 * i + a, cc = i == j ? 6 * i + min(a, c) : 6 * j + c;
    const double v = Sinv[(size_t)r * V.Npad + cc];
    pair[id] = v;
    if (i == j) pose[(size_t)i * 36 + e] = v;
}

// Landmark marginals, thread per landmark:  C_l^-1 + sum over the row pairs (k >= k') of l of  T (k = k')  or  T + T^T (k > k'),
// T = Y_k^T Sigma_{pose(k), pose(k')} Y_k',  in the order k upwards, k' upwards inside; lp_blk (CSR lp_ptr over the landmarks,
// pairs in that order) names the gathered block of each pair.  The upper triangle is summed and mirrored.  A landmark without
// rows gets 1 / (inv_sigma2 + lamda) on its diagonal (one division) and exact zeros beside it.
__global__ __launch_bounds__(256) void k_lm_cov(SchurView V, const double* pair, const int* lp_ptr, const int* lp_blk, double* lm) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= V.L) return;
    const int beg = V.lm_ptr[l], end = V.lm_ptr[l + 1];
    double o[6];                    // 00, 01, 02, 11, 12, 22
    if (beg == end) {
        const double d = 1.0 / (V.inv_sigma2 + V.lamda);
        o[0] = o[3] = o[5] = d;
        o[1] = o[2] = o[4] = 0.0;
    } else {
#pragma unroll
        for (int e = 0; e < 6; ++e) o[e] = V.Cinv[(size_t)l * 6 + e];
        int slot = lp_ptr[l];
        for (int k = beg; k < end; ++k) {
            const double* Yk = V.Y + (size_t)k * 18;
            for (int k2 = beg; k2 <= k; ++k2, ++slot) {
                const double* Sg = pair + (size_t)lp_blk[slot] * 36;
                const double* Y2 = V.Y + (size_t)k2 * 18;
                double M[6][3], T[3][3];
#pragma unroll
                for (int p = 0; p < 6; ++p)
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        double s = 0.0;
#pragma unroll
                        for (int q = 0; q < 6; ++q) s = fma(Sg[6 * p + q], Y2[3 * q + c], s);
                        M[p][c] = s;
                    }
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        double s = 0.0;
#pragma unroll
                        for (int p = 0; p < 6; ++p) s = fma(Yk[3 * p + r], M[p][c], s);
                        T[r][c] = s;
                    }
                int e = 0;
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = r; c < 3; ++c) { o[e] += k2 == k ? T[r][c] : T[r][c] + T[c][r]; ++e; }
            }
        }
    }
    double* out = lm + (size_t)l * 9;
    out[0] = o[0]; out[1] = o[1]; out[2] = o[2];
    out[3] = o[1]; out[4] = o[3]; out[5] = o[4];
    out[6] = o[2]; out[7] = o[4]; out[8] = o[5];
}

// ------------------------------------------------------------------------------------------------ reliability query
// vba_schur_reliability, after the device part of the covariance query (gathered blocks, Y, Cinv, landmark marginals resident).
//
// Row pass, THREAD PER ROW k (pose i, landmark l, position a in the track of l):
//   Sigma_il = -sum_{k' in rows(l)} (S^-1)_{i, pose(k')} Y_k'   (6x3, k' upwards; the block of the pair from lp_blk, which lists
//                                                               k >= k' only: for k' > k the block of (k', k) is read transposed)
//   P_k = w [A Al] [[Sigma_ii, Sigma_il], [Sigma_il^T, Sigma_ll]] [A Al]^T   (symmetric part), leverage = tr P_k, w-test by
//   rel_wtest2.  A row costs t products of 6x6 by 6x3 for a track of t rows, so the rows of a landmark together cost the t^2 of
//   k_lm_cov -- spread over t threads that sit side by side in a wave and read the same Y and the same blocks.
// om[k] = w |r|^2 is kept for the totals.
__global__ __launch_bounds__(256) void k_rel_rows(SchurView V, const double* pair, const int* lp_ptr, const int* lp_blk, const double* lm,
                                                  double* lev, double* wt, double* om) {
    const int64_t k64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k64 >= V.m) return;
    const int k = (int)k64;
    const double w = V.row_w[k];
    RowGeom q;
    row_geometry(V, V.states, V.X, k, q);
    om[k] = w * (q.ru * q.ru + q.rv * q.rv);
    if (w == 0.0) { lev[k] = 0.0; wt[k] = 0.0; return; }
    const int l = V.row_lm[k], beg = V.lm_ptr[l], end = V.lm_ptr[l + 1], a = k - beg, base = lp_ptr[l];
    double G[18];                   // sum (S^-1)_{i, pose(k')} Y_k' = -Sigma_il
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
    double jl[6], jc[12];
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
    const double p00 = w * ((q00 + l00) - (x00 + x00));
    const double p01 = w * ((q01 + l01) - (x01 + x10));
    const double p11 = w * ((q11 + l11) - (x11 + x11));
    lev[k] = p00 + p11;
    wt[k] = rel_wtest2(p00, p01, p11, q.ru, q.rv, w);
}

// sum of leverage, largest finite w-test, count of rows with w > 0 over a list of rows in list order (idx == nullptr: beg .. end)
__device__ __forceinline__ void rel_row_stats(const SchurView& V, const int* idx, int beg, int end, const double* lev, const double* wt, double* out) {
    double s = 0.0, mx = 0.0, cnt = 0.0;
    for (int r = beg; r < end; ++r) {
        const int k = idx ? idx[r] : r;
        s += lev[k];
        const double t = wt[k];
        if (t <= 1.79e308 && t > mx) mx = t;    // (NaN fails both)
        cnt += V.row_w[k] > 0.0 ? 1.0 : 0.0;
    }
    out[0] = s; out[1] = mx; out[2] = cnt;
}

// Thread id < L: the statistics of landmark id over its rows and the test of its catalogue prior as an observation,
// e = X - X0, P_l = Sigma_ll / sigma^2; lmom = |e|^2 / sigma^2 is kept for the totals.  Thread id < n: the statistics of pose id.
__global__ __launch_bounds__(256) void k_rel_stats(SchurView V, const double* lm, const double* lev, const double* wt, double* lmlev, double* lmwt,
                                                   double* lmom, double* lm_stats, double* pose_stats) {
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id < V.L) {
        const int l = id, beg = V.lm_ptr[l], end = V.lm_ptr[l + 1];
        rel_row_stats(V, nullptr, beg, end, lev, wt, lm_stats + (size_t)l * 3);
        const double e[3] = {V.X[3 * l] - V.X0[3 * l], V.X[3 * l + 1] - V.X0[3 * l + 1], V.X[3 * l + 2] - V.X0[3 * l + 2]};
        lmom[l] = V.inv_sigma2 * (e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
        if (beg == end) {           // tested by nothing: the closed form of k_lm_cov's d
            const double d = 1.0 / (V.inv_sigma2 + V.lamda);
            lmlev[l] = (3.0 * d) * V.inv_sigma2;
            lmwt[l] = 0.0;
        } else {
            const double* Sl = lm + (size_t)l * 9;
            const double is2 = V.inv_sigma2;
            const double p[6] = {Sl[0] * is2, Sl[1] * is2, Sl[2] * is2, Sl[4] * is2, Sl[5] * is2, Sl[8] * is2};
            lmlev[l] = (p[0] + p[3]) + p[5];
            const double mI[6] = {1.0 - p[0], -p[1], -p[2], 1.0 - p[3], -p[4], 1.0 - p[5]};
            lmwt[l] = rel_wtest3(mI, e, is2);
        }
    }
    if (id < V.n) rel_row_stats(V, V.pose_rows, V.pose_ptr[id], V.pose_ptr[id + 1], lev, wt, pose_stats + (size_t)id * 3);
}

// Totals, ONE block: thread t sums the rows t, t + 256, ... and the landmarks likewise, then a tree over the 256 partials -- one
// shape for every problem.  fit[8] = Omega, m_eff, t_rows, t_prior, rho, s0sq, largest finite row / landmark w-test.
__global__ __launch_bounds__(256) void k_rel_totals(SchurView V, const double* lev, const double* wt, const double* om, const double* lmlev,
                                                    const double* lmwt, const double* lmom, double* fit) {
    __shared__ double red[7][256];
    const int t = threadIdx.x;
    double a[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};     // om rows, m_eff, t_rows, max row, om prior, t_prior, max landmark
    for (int64_t k = t; k < V.m; k += 256) {
        a[0] += om[k];
        a[1] += V.row_w[k] > 0.0 ? 1.0 : 0.0;
        a[2] += lev[k];
        const double x = wt[k];
        if (x <= 1.79e308 && x > a[3]) a[3] = x;
    }
    for (int l = t; l < V.L; l += 256) {
        a[4] += lmom[l];
        a[5] += lmlev[l];
        const double x = lmwt[l];
        if (x <= 1.79e308 && x > a[6]) a[6] = x;
    }
#pragma unroll
    for (int e = 0; e < 7; ++e) red[e][t] = a[e];
    for (int o = 128; o > 0; o >>= 1) {
        __syncthreads();
        if (t < o) {
#pragma unroll
            for (int e = 0; e < 7; ++e) {
                const double x = red[e][t], y = red[e][t + o];
                red[e][t] = (e == 3 || e == 6) ? (y > x ? y : x) : x + y;
            }
        }
    }
    if (t == 0) {
        const double Omega = red[0][0] + red[4][0], meff = red[1][0], trows = red[2][0], tprior = red[5][0];
        const double rho = ((2.0 * meff + 3.0 * (double)V.L) - trows) - tprior;
        fit[0] = Omega; fit[1] = meff; fit[2] = trows; fit[3] = tprior; fit[4] = rho;
        fit[5] = rho > 0.0 ? Omega / rho : __builtin_nan("");
        fit[6] = red[3][0]; fit[7] = red[6][0];
    }
}

// Scratch of vba_schur_covariance, allocated by the first query of a handle: every array the build and the factorisation write,
// W, the gathered blocks and the landmarks' pair -> block index (built on the host from the uploaded lists, once per upload).
struct SchurQuery {
    char* arena = nullptr;
    double *Cinv = nullptr, *wl = nullptr, *E = nullptr, *Y = nullptr, *S = nullptr, *g = nullptr, *ybuf = nullptr, *invL = nullptr, *dl = nullptr;
    double *W = nullptr, *pair = nullptr, *pose = nullptr, *lm = nullptr;
    int *info = nullptr, *lp_ptr = nullptr, *lp_blk = nullptr;
    hipEvent_t ev[2] = {};
    bool indexed = false;
    float ms = 0.0f;
};

// What vba_schur_reliability needs beyond that, allocated by the first reliability query of a handle: its outputs on the device,
// the per-row and per-landmark cost terms of the totals, and two timing events of its own.
struct SchurRel {
    char* arena = nullptr;
    double *lev = nullptr, *wt = nullptr, *om = nullptr, *lmlev = nullptr, *lmwt = nullptr, *lmom = nullptr, *lm_stats = nullptr,
           *pose_stats = nullptr, *fit = nullptr;
    hipEvent_t ev[2] = {};
    float ms = 0.0f;
};

// State of vba_schur_snoop, allocated by the first snoop of a handle and cleared by vba_schur_upload: the weight a rejected row
// had and a byte per row, a byte per landmark (both cumulative), the per-call decisions of the passes, two timing events.
struct SchurSnoop {
    char* arena = nullptr;
    double *saved = nullptr, *crit_used = nullptr;
    unsigned char *row_mask = nullptr, *lm_mask = nullptr;
    int *lm_dec = nullptr, *pose_pick = nullptr, *pose_short = nullptr, *pose_out = nullptr, *lm_out = nullptr;
    hipEvent_t ev[2] = {};
    int totals[3] = {0, 0, 0};  // rows rejected by their own test, landmarks rejected, rows zeroed through rejected landmarks
    float ms = 0.0f;
};

// State of vba_schur_reweight, allocated by the first re-weighting of a handle and cleared by vba_schur_upload: the weights as
// uploaded, the 2 m keys |r| and the raw weights of the last call, the select's histograms, two timing events.
struct SchurRobust {
    char* arena = nullptr;
    double *base = nullptr, *keys = nullptr, *q = nullptr, *part = nullptr, *res = nullptr;
    unsigned long long *hist = nullptr, *state = nullptr;
    hipEvent_t ev[2] = {};
    bool captured = false;      // base holds the weights of the current upload
    bool have_keys = false;     // keys are those of a re-weighting since the current upload
    int launches = 0;           // kernel launches of the last re-weighting
    float ms = 0.0f;
};

// State of vba_schur_enable_dynamics: the reduced system re-sized for N = 9 n (S, g, ybuf, invL: the view points here from then on),
// the edges' step counts, the factor of the last build and the partials of its cost.
struct SchurDyn {
    char* arena = nullptr;
    bool enabled = false;
    double sigma = 0.0;
    int* steps = nullptr;
    double *r = nullptr, *A = nullptr, *ecost = nullptr, *part = nullptr;
    int npart = 0;
    std::vector<double> h_part;
};

// one grow-only workspace per process for vba_schur_median (keys, the select's scratch, the result)
struct MedianWorkspace {
    std::mutex m;
    int device = -1;
    char* base = nullptr;
    size_t size = 0;
    hipStream_t stream = nullptr;
} g_median_ws;

// why the three queries refuse a handle with the dynamics factor
const char* const kDynRefusal = " is not available on a handle with the dynamics factor: its redundancy counts and gathers assume the "
                                "6 n reduced system of the reprojection rows";

thread_local std::string g_serr;
int sfail(int code, const std::string& msg) { g_serr = msg; return code; }

#define SCHK(expr)                                                                                     \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return sfail(VBA_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

}  // namespace

struct vba_schur_context {
    int device = 0;
    SchurView V{};
    char* arena = nullptr;
    hipStream_t stream = nullptr, aux = nullptr;    // aux: the bulk of a panel's trailing update beside the next panel's factorisation
    hipEvent_t ev[5] = {};
    hipEvent_t ev_chain = nullptr, ev_bulk = nullptr;
    int classic = 0;                // VBA_SCHUR_CLASSIC=1: the round-2 tile-by-tile factorisation (comparison)
    int* d_info = nullptr;
    int last_info = 0;              // 0, or 1 + the row at which the last factorisation met a non-positive pivot
    double* S0 = nullptr;       // states buffers
    double* S1 = nullptr;
    double* X0buf = nullptr;
    double* X1buf = nullptr;
    std::vector<double> h_part;
    bool uploaded = false, have_state = false;
    float ms[4] = {0, 0, 0, 0};
    int64_t npairs = 0;
    SchurQuery q;               // vba_schur_covariance's scratch (nothing until the first query)
    SchurRel rel;               // vba_schur_reliability's scratch on top of it (nothing until the first reliability query)
    SchurSnoop snoop;           // vba_schur_snoop's state (nothing until the first snoop)
    SchurRobust robust;         // vba_schur_reweight's state (nothing until the first re-weighting)
    SchurDyn dyn;               // vba_schur_enable_dynamics' state (nothing on a handle without the dynamics factor)
    int bw = 1 << 30;           // tile bandwidth of the reduced system (max |I - J| over its non-zero tiles), from the block list
};

extern "C" {

const char* vba_schur_last_error(void) { return g_serr.c_str(); }

int vba_schur_create(int device, int n, int64_t m, int L, int nblk, int64_t npairs, vba_schur_handle* out) {
    if (!out) return sfail(VBA_EINVAL, "null out");
    *out = nullptr;
    if (n < 1 || m < 1 || L < 1 || nblk < n || npairs < m) return sfail(VBA_EINVAL, "sizes out of range");
    if (m > INT32_MAX || npairs > INT32_MAX) return sfail(VBA_EINVAL, "m and npairs must fit 32-bit indices (CSR and pair lists are int32)");
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt == 0) return sfail(VBA_ENODEV, "no HIP device visible");
    if (device < 0 || device >= cnt) return sfail(VBA_EINVAL, "device index out of range");
    SCHK(hipSetDevice(device));
    vba_schur_context* h = new (std::nothrow) vba_schur_context();
    if (!h) return sfail(VBA_ENOMEM, "host allocation failed");
    h->device = device;
    SchurView& V = h->V;
    V.n = n; V.m = m; V.L = L; V.nblk = nblk;
    V.N = 6 * n;
    V.nb = (V.N + kT * kPanel - 1) / (kT * kPanel) * kPanel;    // whole panels (the padding rows are an identity block)
    V.Npad = V.nb * kT;
    V.npart = (int)((std::max<int64_t>(m, L) + 255) / 256);
    h->npairs = npairs;
    size_t bytes = 0;
    auto need = [&](size_t b) { size_t o = bytes; bytes += (b + 255) & ~size_t(255); return o; };
    const size_t o_lmptr = need((size_t)(L + 1) * 4), o_rpose = need(m * 4), o_rlm = need(m * 4), o_u = need(m * 8), o_v = need(m * 8), o_w = need(m * 8);
    const size_t o_pptr = need((size_t)(n + 1) * 4), o_prows = need(m * 4);
    const size_t o_bi = need((size_t)nblk * 4), o_bj = need((size_t)nblk * 4), o_bptr = need((size_t)(nblk + 1) * 4), o_pk = need(npairs * 4), o_pk2 = need(npairs * 4);
    const size_t o_intr = need((size_t)n * 32), o_X0 = need((size_t)L * 24);
    const size_t o_s0 = need((size_t)n * 80), o_s1 = need((size_t)n * 80), o_x0 = need((size_t)L * 24), o_x1 = need((size_t)L * 24);
    const size_t o_ci = need((size_t)L * 48), o_wl = need((size_t)L * 24), o_E = need(m * 144), o_Y = need(m * 144);
    const size_t o_S = need((size_t)V.Npad * V.Npad * 8), o_g = need((size_t)V.Npad * 8), o_y = need((size_t)V.Npad * 8), o_iL = need((size_t)V.nb * kT * kT * 8);
    const size_t o_dl = need((size_t)L * 24), o_part = need((size_t)V.npart * 8), o_info = need(256);
    if (hipMalloc(&h->arena, bytes) != hipSuccess) { delete h; return sfail(VBA_ENOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes failed"); }
    if (hipMemset(h->arena, 0, bytes) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess) { hipFree(h->arena); delete h; return sfail(VBA_EHIP, "hipMemset failed"); }
    char* A = h->arena;
    V.lm_ptr = (int*)(A + o_lmptr); V.row_pose = (int*)(A + o_rpose); V.row_lm = (int*)(A + o_rlm);
    V.row_u = (double*)(A + o_u); V.row_v = (double*)(A + o_v); V.row_w = (double*)(A + o_w);
    V.pose_ptr = (int*)(A + o_pptr); V.pose_rows = (int*)(A + o_prows);
    V.blk_i = (int*)(A + o_bi); V.blk_j = (int*)(A + o_bj); V.blk_ptr = (int*)(A + o_bptr); V.pair_k = (int*)(A + o_pk); V.pair_k2 = (int*)(A + o_pk2);
    V.intr = (double*)(A + o_intr); V.X0 = (double*)(A + o_X0);
    h->S0 = (double*)(A + o_s0); h->S1 = (double*)(A + o_s1); h->X0buf = (double*)(A + o_x0); h->X1buf = (double*)(A + o_x1);
    V.Cinv = (double*)(A + o_ci); V.wl = (double*)(A + o_wl); V.E = (double*)(A + o_E); V.Y = (double*)(A + o_Y);
    V.S = (double*)(A + o_S); V.g = (double*)(A + o_g); V.ybuf = (double*)(A + o_y); V.invL = (double*)(A + o_iL);
    V.dl = (double*)(A + o_dl); V.part = (double*)(A + o_part); h->d_info = (int*)(A + o_info);
    h->h_part.resize(V.npart);
    bool ok = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) == hipSuccess &&
              hipStreamCreateWithFlags(&h->aux, hipStreamNonBlocking) == hipSuccess &&
              hipEventCreateWithFlags(&h->ev_chain, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&h->ev_bulk, hipEventDisableTiming) == hipSuccess;
    if (const char* e = std::getenv("VBA_SCHUR_CLASSIC")) h->classic = std::atoi(e);
    for (int k = 0; k < 5 && ok; ++k) ok = hipEventCreate(&h->ev[k]) == hipSuccess;
    if (!ok) { vba_schur_destroy(h); return sfail(VBA_EHIP, "stream / event creation failed"); }
    *out = h;
    return VBA_OK;
}

int vba_schur_destroy(vba_schur_handle h) {
    if (!h) return VBA_OK;
    hipSetDevice(h->device);
    if (h->stream) { hipStreamSynchronize(h->stream); hipStreamDestroy(h->stream); }
    if (h->aux) { hipStreamSynchronize(h->aux); hipStreamDestroy(h->aux); }
    if (h->ev_chain) hipEventDestroy(h->ev_chain);
    if (h->ev_bulk) hipEventDestroy(h->ev_bulk);
    for (hipEvent_t e : h->ev) if (e) hipEventDestroy(e);
    for (hipEvent_t e : h->q.ev) if (e) hipEventDestroy(e);
    for (hipEvent_t e : h->rel.ev) if (e) hipEventDestroy(e);
    for (hipEvent_t e : h->snoop.ev) if (e) hipEventDestroy(e);
    for (hipEvent_t e : h->robust.ev) if (e) hipEventDestroy(e);
    if (h->dyn.arena) hipFree(h->dyn.arena);
    if (h->robust.arena) hipFree(h->robust.arena);
    if (h->snoop.arena) hipFree(h->snoop.arena);
    if (h->rel.arena) hipFree(h->rel.arena);
    if (h->q.arena) hipFree(h->q.arena);
    if (h->arena) hipFree(h->arena);
    delete h;
    return VBA_OK;
}

int vba_schur_upload(vba_schur_handle h, const int* lm_ptr, const int* row_pose, const int* row_lm, const double* row_u,
                     const double* row_v, const double* row_w, const int* pose_ptr, const int* pose_rows, const int* blk_i,
                     const int* blk_j, const int* blk_ptr, const int* pair_k, const int* pair_k2, const double* intrinsics,
                     const double* X0, double sigma_prior) {
    if (!h) return sfail(VBA_EINVAL, "null handle");
    if (!lm_ptr || !row_pose || !row_lm || !row_u || !row_v || !row_w || !pose_ptr || !pose_rows || !blk_i || !blk_j || !blk_ptr ||
        !pair_k || !pair_k2 || !intrinsics || !X0)
        return sfail(VBA_EINVAL, "null array");
    if (!(sigma_prior > 0.0)) return sfail(VBA_EINVAL, "sigma_prior must be positive");
    const SchurView& V = h->V;
    // the structure arrays index each other: check them on the host before a kernel trusts them
    if (lm_ptr[0] != 0 || lm_ptr[V.L] != V.m || pose_ptr[0] != 0 || pose_ptr[V.n] != V.m || blk_ptr[0] != 0 || blk_ptr[V.nblk] != h->npairs)
        return sfail(VBA_EINVAL, "CSR pointers do not span their arrays");
    for (int l = 0; l < V.L; ++l) if (lm_ptr[l + 1] < lm_ptr[l]) return sfail(VBA_EINVAL, "lm_ptr not monotone");
    for (int i = 0; i < V.n; ++i) if (pose_ptr[i + 1] < pose_ptr[i]) return sfail(VBA_EINVAL, "pose_ptr not monotone");
    for (int b = 0; b < V.nblk; ++b) {
        if (blk_ptr[b + 1] < blk_ptr[b]) return sfail(VBA_EINVAL, "blk_ptr not monotone");
        if (blk_i[b] < 0 || blk_i[b] >= V.n || blk_j[b] < 0 || blk_j[b] > blk_i[b]) return sfail(VBA_EINVAL, "block index outside the lower triangle");
    }
    for (int64_t k = 0; k < V.m; ++k) {
        if (row_pose[k] < 0 || row_pose[k] >= V.n || row_lm[k] < 0 || row_lm[k] >= V.L || pose_rows[k] < 0 || pose_rows[k] >= V.m)
            return sfail(VBA_EINVAL, "row index out of range");
    }
    for (int64_t p = 0; p < h->npairs; ++p)
        if (pair_k[p] < 0 || pair_k[p] >= V.m || pair_k2[p] < 0 || pair_k2[p] >= V.m) return sfail(VBA_EINVAL, "pair index out of range");
    SCHK(hipSetDevice(h->device));
    auto up = [&](const void* dst, const void* src, size_t bytes) { return hipMemcpy(const_cast<void*>(dst), src, bytes, hipMemcpyHostToDevice); };
    SCHK(up(V.lm_ptr, lm_ptr, (size_t)(V.L + 1) * 4)); SCHK(up(V.row_pose, row_pose, V.m * 4)); SCHK(up(V.row_lm, row_lm, V.m * 4));
    SCHK(up(V.row_u, row_u, V.m * 8)); SCHK(up(V.row_v, row_v, V.m * 8)); SCHK(up(V.row_w, row_w, V.m * 8));
    SCHK(up(V.pose_ptr, pose_ptr, (size_t)(V.n + 1) * 4)); SCHK(up(V.pose_rows, pose_rows, V.m * 4));
    SCHK(up(V.blk_i, blk_i, (size_t)V.nblk * 4)); SCHK(up(V.blk_j, blk_j, (size_t)V.nblk * 4)); SCHK(up(V.blk_ptr, blk_ptr, (size_t)(V.nblk + 1) * 4));
    SCHK(up(V.pair_k, pair_k, h->npairs * 4)); SCHK(up(V.pair_k2, pair_k2, h->npairs * 4));
    SCHK(up(V.intr, intrinsics, (size_t)V.n * 32)); SCHK(up(V.X0, X0, (size_t)V.L * 24));
    h->V.inv_sigma2 = 1.0 / (sigma_prior * sigma_prior);
    h->bw = 0;
    for (int b = 0; b < V.nblk; ++b) h->bw = std::max(h->bw, (6 * blk_i[b] + 5) / kT - (6 * blk_j[b]) / kT);
    if (h->dyn.enabled) h->bw = V.nb - 1;       // velocity rows reach every pose column
    h->q.indexed = false;
    if (h->snoop.arena) {       // new weights: nothing is rejected
        SCHK(hipMemset(h->snoop.row_mask, 0, (size_t)V.m));
        SCHK(hipMemset(h->snoop.lm_mask, 0, (size_t)V.L));
        SCHK(hipStreamSynchronize(nullptr));
        std::fill(h->snoop.totals, h->snoop.totals + 3, 0);
    }
    h->robust.captured = h->robust.have_keys = false;       // new weights: they are the base of the next re-weighting
    h->uploaded = true;
    return VBA_OK;
}

int vba_schur_set_state(vba_schur_handle h, const double* states, const double* landmarks) {
    if (!h || !states || !landmarks) return sfail(VBA_EINVAL, "null argument");
    SCHK(hipSetDevice(h->device));
    SCHK(hipStreamSynchronize(h->stream));
    SCHK(hipMemcpy(h->S0, states, (size_t)h->V.n * 80, hipMemcpyHostToDevice));
    SCHK(hipMemcpy(h->X0buf, landmarks, (size_t)h->V.L * 24, hipMemcpyHostToDevice));
    h->have_state = true;
    return VBA_OK;
}

int vba_schur_get_state(vba_schur_handle h, double* states, double* landmarks) {
    if (!h) return sfail(VBA_EINVAL, "null handle");
    if (!h->have_state) return sfail(VBA_ESTATE, "no state set");
    SCHK(hipSetDevice(h->device));
    SCHK(hipStreamSynchronize(h->stream));
    if (states) SCHK(hipMemcpy(states, h->S0, (size_t)h->V.n * 80, hipMemcpyDeviceToHost));
    if (landmarks) SCHK(hipMemcpy(landmarks, h->X0buf, (size_t)h->V.L * 24, hipMemcpyDeviceToHost));
    return VBA_OK;
}

// the dynamics arrays of a handle with the factor enabled, at the damping of the view
static SchurDynView schur_dyn_view(vba_schur_handle h, const SchurView& V) {
    const SchurDyn& D = h->dyn;
    SchurDynView W{};
    W.n = V.n; W.Npad = V.Npad; W.sigma = D.sigma; W.lamda = V.lamda;
    W.steps = D.steps; W.r = D.r; W.A = D.A; W.ecost = D.ecost; W.part = D.part; W.npart = D.npart;
    W.S = V.S; W.g = V.g;
    return W;
}

static int schur_cost(vba_schur_handle h, const double* states, const double* X, double* cost) {
    SchurView V = h->V;
    SchurDyn& D = h->dyn;
    hipLaunchKernelGGL(k_cost, dim3(V.npart), dim3(256), 0, h->stream, V, states, X);
    if (D.enabled) schur_dyn_cost_launch(schur_dyn_view(h, V), states, h->stream);
    SCHK(hipGetLastError());
    SCHK(hipMemcpyAsync(h->h_part.data(), V.part, (size_t)V.npart * 8, hipMemcpyDeviceToHost, h->stream));
    if (D.enabled) SCHK(hipMemcpyAsync(D.h_part.data(), D.part, (size_t)D.npart * 8, hipMemcpyDeviceToHost, h->stream));
    SCHK(hipStreamSynchronize(h->stream));
    double s = 0.0;
    for (int b = 0; b < V.npart; ++b) s += h->h_part[b];      // fixed order
    if (D.enabled) for (int b = 0; b < D.npart; ++b) s += D.h_part[b];     // ... the dynamics partials after the rows' and the prior's
    *cost = s;
    return VBA_OK;
}

// Build the reduced camera system of the view's state and damping and factorise it, on stream s (the bulk of a panel's trailing
// update beside it on h->aux): S, g, Cinv, wl, E, Y, invL and *d_info are the view's and the caller's, so vba_schur_iterate runs it
// on the handle's arrays and vba_schur_covariance on scratch of its own.  ev_built (if given) is recorded between the two parts.
static int schur_build_factor(vba_schur_handle h, const SchurView& V, hipStream_t s, int* d_info, hipEvent_t ev_built) {
    SCHK(hipMemsetAsync(V.S, 0, (size_t)V.Npad * V.Npad * 8, s));
    SCHK(hipMemsetAsync(V.g, 0, (size_t)V.Npad * 8, s));
    SCHK(hipMemsetAsync(d_info, 0, 4, s));
    hipLaunchKernelGGL(k_lm_blocks, dim3((V.L + 255) / 256), dim3(256), 0, s, V);
    hipLaunchKernelGGL(k_pose_blocks, dim3((V.n + 15) / 16), dim3(256), 0, s, V);
    hipLaunchKernelGGL(k_pair_blocks, dim3(V.nblk), dim3(64), 0, s, V);
    if (h->dyn.enabled) {       // the dynamics blocks on top of the reprojection blocks (the queries never come here with the factor on)
        const SchurDynView W = schur_dyn_view(h, V);
        schur_dyn_edges_launch(W, V.states, s);
        schur_dyn_scatter_launch(W, s);
    }
    if (V.Npad > V.N) hipLaunchKernelGGL(k_pad_identity, dim3((V.Npad - V.N + 63) / 64), dim3(64), 0, s, V);
    if (ev_built) SCHK(hipEventRecord(ev_built, s));
    if (h->classic == 1) {  // round 2: one tile column at a time, trailing update with K = 64 (VBA_SCHUR_CLASSIC=2: panels, round-2 tile kernel)
        for (int kb = 0; kb < V.nb; ++kb) {
            hipLaunchKernelGGL(k_potrf64, dim3(1), dim3(64), 0, s, V, kb, d_info);
            const int rest = V.nb - kb - 1;
            if (rest > 0) {
                hipLaunchKernelGGL((k_gemm_abt<0>), dim3(rest), dim3(256), 0, s, V, kb, 0);
                hipLaunchKernelGGL((k_gemm_abt<1>), dim3(rest * (rest + 1) / 2), dim3(256), 0, s, V, kb, 0);
            }
        }
    } else {
        // Right-looking by PANELS of kPanel tile columns with look-ahead.  The panel is factorised tile column by tile column
        // (diagonal tile in one wave's registers, panel rows by its inverse, the panel's remaining columns updated with K = 64:
        // skinny, cheap); then the trailing matrix gets ONE update with K = 256.  That update is split: the 256 columns the NEXT
        // panel consists of first, on this stream -- the next panel's factorisation (a chain of small dependent launches) then
        // starts at once and runs beside the bulk of the update on the second stream.
        const int np = V.nb / kPanel, nB = V.nb / 2;            // panels; 128-row blocks
        bool bulk_pending = false;
        for (int p = 0; p < np; ++p) {
            const int kb0 = p * kPanel, klast = kb0 + kPanel - 1;
            for (int kb = kb0; kb <= klast; ++kb) {
                if (h->classic == 2) hipLaunchKernelGGL(k_potrf64, dim3(1), dim3(64), 0, s, V, kb, d_info);
                else hipLaunchKernelGGL(k_potrf64b, dim3(1), dim3(256), 0, s, V, kb, d_info);
                const int rest = V.nb - kb - 1;
                if (rest > 0) hipLaunchKernelGGL((k_gemm_abt<0>), dim3(rest), dim3(256), 0, s, V, kb, 0);
                if (kb < klast) hipLaunchKernelGGL((k_gemm_abt<2>), dim3(rest, klast - kb), dim3(256), 0, s, V, kb, klast);
            }
            const int b0 = (kb0 + kPanel) / 2;                  // first 128-block of the trailing matrix
            if (b0 >= nB) break;
            SCHK(hipEventRecord(h->ev_chain, s));
            if (bulk_pending) SCHK(hipStreamWaitEvent(s, h->ev_bulk, 0));      // the previous bulk update wrote the columns of this one
            hipLaunchKernelGGL(k_syrk_panel, dim3(nB - b0, std::min(2, nB - b0)), dim3(512), 0, s, V, kb0, b0, b0);     // next panel's columns
            bulk_pending = false;
            if (nB - b0 > 2) {
                SCHK(hipStreamWaitEvent(h->aux, h->ev_chain, 0));
                hipLaunchKernelGGL(k_syrk_panel, dim3(nB - b0 - 2, nB - b0 - 2), dim3(512), 0, h->aux, V, kb0, b0 + 2, b0 + 2);
                SCHK(hipEventRecord(h->ev_bulk, h->aux));
                bulk_pending = true;
            }
        }
        if (bulk_pending) SCHK(hipStreamWaitEvent(s, h->ev_bulk, 0));
    }
    return VBA_OK;
}

int vba_schur_iterate(vba_schur_handle h, double lamda, double* cost_before, double* cost_after, int* accepted) {
    if (!h || !cost_before || !cost_after || !accepted) return sfail(VBA_EINVAL, "null argument");
    if (!h->uploaded || !h->have_state) return sfail(VBA_ESTATE, "upload the problem and set the state first");
    if (!(lamda >= 0.0)) return sfail(VBA_EINVAL, "lamda must be >= 0");
    SCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    SchurView V = h->V;
    V.lamda = lamda;
    V.states = h->S0; V.X = h->X0buf; V.states_new = h->S1; V.X_new = h->X1buf;
    if (int rc = schur_cost(h, V.states, V.X, cost_before)) return rc;
    SCHK(hipEventRecord(h->ev[0], s));
    if (int rc = schur_build_factor(h, V, s, h->d_info, h->ev[1])) return rc;
    SCHK(hipEventRecord(h->ev[2], s));
    for (int kb = 0; kb < V.nb; ++kb)
        hipLaunchKernelGGL(k_trsv_step, dim3(1 + std::min(h->bw, V.nb - 1 - kb)), dim3(256), 0, s, V, kb, 0);
    for (int kb = V.nb - 1; kb >= 0; --kb)
        hipLaunchKernelGGL(k_trsv_step, dim3(1 + std::min(h->bw, kb)), dim3(256), 0, s, V, kb, 1);
    hipLaunchKernelGGL(k_lm_update, dim3((std::max(V.L, V.n) + 255) / 256), dim3(256), 0, s, V);
    if (h->dyn.enabled) schur_dyn_update_launch(schur_dyn_view(h, V), V.states, V.states_new, s);
    SCHK(hipEventRecord(h->ev[3], s));
    SCHK(hipGetLastError());
    int info = 0;
    SCHK(hipMemcpyAsync(&info, h->d_info, 4, hipMemcpyDeviceToHost, s));
    SCHK(hipStreamSynchronize(s));
    for (int k = 0; k < 3; ++k) (void)hipEventElapsedTime(&h->ms[k], h->ev[k], h->ev[k + 1]);
    h->last_info = info;
    if (info != 0) {
        // Not positive definite at this damping: the ordinary LM answer to a failed factorisation is a rejected trial (the
        // caller raises lamda), not an error.  The state is untouched; vba_schur_last_info reports the failing row.
        *cost_after = *cost_before;
        *accepted = 0;
        return VBA_OK;
    }
    if (int rc = schur_cost(h, V.states_new, V.X_new, cost_after)) return rc;
    *accepted = (*cost_after < *cost_before) ? 1 : 0;
    if (*accepted) { std::swap(h->S0, h->S1); std::swap(h->X0buf, h->X1buf); }
    return VBA_OK;
}

// first query of a handle: the scratch and its two timing events
static int schur_query_alloc(vba_schur_handle h) {
    SchurQuery& Q = h->q;
    if (Q.arena) return VBA_OK;
    const SchurView& V = h->V;
    const size_t m = (size_t)V.m, L = (size_t)V.L, NN = (size_t)V.Npad * V.Npad * 8;
    size_t bytes = 0;
    auto need = [&](size_t b) { size_t o = bytes; bytes += (b + 255) & ~size_t(255); return o; };
    const size_t o_ci = need(L * 48), o_wl = need(L * 24), o_E = need(m * 144), o_Y = need(m * 144), o_S = need(NN), o_g = need((size_t)V.Npad * 8),
                 o_y = need((size_t)V.Npad * 8), o_iL = need((size_t)V.nb * kT * kT * 8), o_dl = need(L * 24), o_W = need(NN),
                 o_pair = need((size_t)V.nblk * 288), o_pose = need((size_t)V.n * 288), o_lm = need(L * 72), o_info = need(256),
                 o_lpp = need((L + 1) * 4), o_lpb = need((size_t)h->npairs * 4);
    char* A = nullptr;
    if (hipMalloc(&A, bytes) != hipSuccess) { (void)hipGetLastError(); return sfail(VBA_ENOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes of query scratch failed"); }
    hipEvent_t ev[2] = {};
    if (hipMemset(A, 0, bytes) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess || hipEventCreate(&ev[0]) != hipSuccess ||
        hipEventCreate(&ev[1]) != hipSuccess) {
        if (ev[0]) hipEventDestroy(ev[0]);
        hipFree(A);
        return sfail(VBA_EHIP, "query scratch: hipMemset / event creation failed");
    }
    Q.arena = A; Q.ev[0] = ev[0]; Q.ev[1] = ev[1];
    Q.Cinv = (double*)(A + o_ci); Q.wl = (double*)(A + o_wl); Q.E = (double*)(A + o_E); Q.Y = (double*)(A + o_Y); Q.S = (double*)(A + o_S);
    Q.g = (double*)(A + o_g); Q.ybuf = (double*)(A + o_y); Q.invL = (double*)(A + o_iL); Q.dl = (double*)(A + o_dl); Q.W = (double*)(A + o_W);
    Q.pair = (double*)(A + o_pair); Q.pose = (double*)(A + o_pose); Q.lm = (double*)(A + o_lm); Q.info = (int*)(A + o_info);
    Q.lp_ptr = (int*)(A + o_lpp); Q.lp_blk = (int*)(A + o_lpb);
    return VBA_OK;
}

// Once per upload: for every landmark the block of each of its row pairs (k >= k'), in the order k_lm_cov walks them.  The pair
// lists are grouped by block; they are read back and turned round on the host, and checked on the way (every pair of every
// landmark exactly once, in the block of its two poses; every diagonal block listed): k_lm_cov and k_cov_gather rely on that.
static int schur_query_index(vba_schur_handle h) {
    SchurQuery& Q = h->q;
    if (Q.indexed) return VBA_OK;
    const SchurView& V = h->V;
    const size_t m = (size_t)V.m, np = (size_t)h->npairs;
    std::vector<int> lm_ptr(V.L + 1), row_pose(m), row_lm(m), bi(V.nblk), bj(V.nblk), bptr(V.nblk + 1), pk(np), pk2(np);
    auto down = [&](std::vector<int>& dst, const int* src) { return hipMemcpy(dst.data(), src, dst.size() * 4, hipMemcpyDeviceToHost); };
    SCHK(down(lm_ptr, V.lm_ptr)); SCHK(down(row_pose, V.row_pose)); SCHK(down(row_lm, V.row_lm)); SCHK(down(bi, V.blk_i)); SCHK(down(bj, V.blk_j));
    SCHK(down(bptr, V.blk_ptr)); SCHK(down(pk, V.pair_k)); SCHK(down(pk2, V.pair_k2));
    std::vector<int> lp_ptr(V.L + 1, 0);
    int64_t total = 0;
    for (int l = 0; l < V.L; ++l) {
        const int64_t t = lm_ptr[l + 1] - lm_ptr[l];
        total += t * (t + 1) / 2;
        if (total > h->npairs) return sfail(VBA_EINVAL, "the pair lists do not hold every row pair of every landmark");
        lp_ptr[l + 1] = (int)total;
    }
    if (total != h->npairs) return sfail(VBA_EINVAL, "the pair lists do not hold every row pair of every landmark");
    std::vector<int> lp_blk(np, -1);
    std::vector<char> has_diag(V.n, 0);
    for (int b = 0; b < V.nblk; ++b) {
        if (bi[b] == bj[b]) has_diag[bi[b]] = 1;
        for (int p = bptr[b]; p < bptr[b + 1]; ++p) {
            const int k = pk[p], k2 = pk2[p], l = row_lm[k];
            if (row_lm[k2] != l || k2 > k || k2 < lm_ptr[l] || k >= lm_ptr[l + 1] || row_pose[k] != bi[b] || row_pose[k2] != bj[b])
                return sfail(VBA_EINVAL, "a listed row pair does not belong to its block");
            const int a = k - lm_ptr[l], c = k2 - lm_ptr[l];
            int& slot = lp_blk[(size_t)lp_ptr[l] + (size_t)a * (a + 1) / 2 + c];
            if (slot != -1) return sfail(VBA_EINVAL, "a row pair is listed twice");
            slot = b;
        }
    }
    // (np pairs into np distinct slots: every slot is filled)
    for (int i = 0; i < V.n; ++i) if (!has_diag[i]) return sfail(VBA_EINVAL, "the block list lacks a diagonal block");
    SCHK(hipMemcpy(Q.lp_ptr, lp_ptr.data(), lp_ptr.size() * 4, hipMemcpyHostToDevice));
    SCHK(hipMemcpy(Q.lp_blk, lp_blk.data(), np * 4, hipMemcpyHostToDevice));
    Q.indexed = true;
    return VBA_OK;
}

// The device part of vba_schur_covariance, shared with vba_schur_reliability: ev_begin, then build and factorise into the query's
// scratch at this damping (V: the view that was built -- the handle's problem, everything written in the scratch), the info word
// to the host (*bad), and unless the factorisation failed the selected inverse, the gathered blocks (Q.pair, Q.pose) and, with
// with_lm, the landmark marginals (Q.lm).  The launches and their order are those vba_schur_covariance has always issued.
static int schur_query_device(vba_schur_handle h, double lamda, bool with_lm, hipEvent_t ev_begin, SchurView& V, int* bad) {
    SchurQuery& Q = h->q;
    hipStream_t s = h->stream;
    V = h->V;
    V.lamda = lamda;
    V.states = h->S0; V.X = h->X0buf; V.states_new = nullptr; V.X_new = nullptr; V.part = nullptr;
    V.Cinv = Q.Cinv; V.wl = Q.wl; V.E = Q.E; V.Y = Q.Y; V.S = Q.S; V.g = Q.g; V.ybuf = Q.ybuf; V.invL = Q.invL; V.dl = Q.dl;
    SCHK(hipEventRecord(ev_begin, s));
    if (int rc = schur_build_factor(h, V, s, Q.info, nullptr)) return rc;
    SCHK(hipGetLastError());
    *bad = 0;
    SCHK(hipMemcpyAsync(bad, Q.info, 4, hipMemcpyDeviceToHost, s));
    SCHK(hipStreamSynchronize(s));
    if (*bad != 0) return VBA_OK;
    const int nbu = (V.N + kT - 1) / kT;
    const size_t n_pair = (size_t)V.nblk * 36;
    for (int d = 0; d < nbu; ++d) hipLaunchKernelGGL(k_trinv_step, dim3(nbu - d), dim3(256), 0, s, V, Q.W, d, h->bw);
    hipLaunchKernelGGL(k_syrk_wtw, dim3(nbu * (nbu + 1) / 2), dim3(256), 0, s, V, Q.W, Q.S, nbu);      // (over the factor: no longer needed)
    hipLaunchKernelGGL(k_cov_gather, dim3((unsigned)((n_pair + 255) / 256)), dim3(256), 0, s, V, Q.S, Q.pair, Q.pose);
    if (with_lm) hipLaunchKernelGGL(k_lm_cov, dim3((V.L + 255) / 256), dim3(256), 0, s, V, Q.pair, Q.lp_ptr, Q.lp_blk, Q.lm);
    return VBA_OK;
}

int vba_schur_covariance(vba_schur_handle h, double lamda, double* pose_cov, double* pair_cov, double* lm_cov, int* info) {
    if (!h || !info) return sfail(VBA_EINVAL, "null argument");
    if (h->dyn.enabled) return sfail(VBA_ESTATE, std::string("vba_schur_covariance") + kDynRefusal);
    if (!(lamda >= 0.0)) return sfail(VBA_EINVAL, "lamda must be >= 0");
    if (!h->uploaded || !h->have_state) return sfail(VBA_ESTATE, "upload the problem and set the state first");
    SCHK(hipSetDevice(h->device));
    if (int rc = schur_query_alloc(h)) return rc;
    if (int rc = schur_query_index(h)) return rc;
    SchurQuery& Q = h->q;
    hipStream_t s = h->stream;
    SchurView V;
    int bad = 0;
    if (int rc = schur_query_device(h, lamda, lm_cov != nullptr, Q.ev[0], V, &bad)) return rc;
    *info = bad;
    const size_t n_pose = (size_t)V.n * 36, n_pair = (size_t)V.nblk * 36, n_lm = (size_t)V.L * 9;
    if (bad != 0) {                 // no factor, no covariance: NaN, and the row in *info
        SCHK(hipEventRecord(Q.ev[1], s));
        SCHK(hipStreamSynchronize(s));
        (void)hipEventElapsedTime(&Q.ms, Q.ev[0], Q.ev[1]);
        if (pose_cov) std::fill(pose_cov, pose_cov + n_pose, std::nan(""));
        if (pair_cov) std::fill(pair_cov, pair_cov + n_pair, std::nan(""));
        if (lm_cov) std::fill(lm_cov, lm_cov + n_lm, std::nan(""));
        return VBA_OK;
    }
    SCHK(hipEventRecord(Q.ev[1], s));
    SCHK(hipGetLastError());
    if (pose_cov) SCHK(hipMemcpyAsync(pose_cov, Q.pose, n_pose * 8, hipMemcpyDeviceToHost, s));
    if (pair_cov) SCHK(hipMemcpyAsync(pair_cov, Q.pair, n_pair * 8, hipMemcpyDeviceToHost, s));
    if (lm_cov) SCHK(hipMemcpyAsync(lm_cov, Q.lm, n_lm * 8, hipMemcpyDeviceToHost, s));
    SCHK(hipStreamSynchronize(s));
    (void)hipEventElapsedTime(&Q.ms, Q.ev[0], Q.ev[1]);
    return VBA_OK;
}

int vba_schur_last_covariance_ms(vba_schur_handle h, float* ms) {
    if (!h || !ms) return sfail(VBA_EINVAL, "null argument");
    *ms = h->q.ms;
    return VBA_OK;
}

// first reliability query of a handle: its scratch and its two timing events
static int schur_rel_alloc(vba_schur_handle h) {
    SchurRel& R = h->rel;
    if (R.arena) return VBA_OK;
    const SchurView& V = h->V;
    const size_t m = (size_t)V.m, L = (size_t)V.L;
    size_t bytes = 0;
    auto need = [&](size_t b) { size_t o = bytes; bytes += (b + 255) & ~size_t(255); return o; };
    const size_t o_lev = need(m * 8), o_wt = need(m * 8), o_om = need(m * 8), o_ll = need(L * 8), o_lw = need(L * 8), o_lo = need(L * 8),
                 o_ls = need(L * 24), o_ps = need((size_t)V.n * 24), o_fit = need(64);
    char* A = nullptr;
    if (hipMalloc(&A, bytes) != hipSuccess) { (void)hipGetLastError(); return sfail(VBA_ENOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes of reliability scratch failed"); }
    hipEvent_t ev[2] = {};
    if (hipMemset(A, 0, bytes) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess || hipEventCreate(&ev[0]) != hipSuccess ||
        hipEventCreate(&ev[1]) != hipSuccess) {
        if (ev[0]) hipEventDestroy(ev[0]);
        hipFree(A);
        return sfail(VBA_EHIP, "reliability scratch: hipMemset / event creation failed");
    }
    R.arena = A; R.ev[0] = ev[0]; R.ev[1] = ev[1];
    R.lev = (double*)(A + o_lev); R.wt = (double*)(A + o_wt); R.om = (double*)(A + o_om); R.lmlev = (double*)(A + o_ll); R.lmwt = (double*)(A + o_lw);
    R.lmom = (double*)(A + o_lo); R.lm_stats = (double*)(A + o_ls); R.pose_stats = (double*)(A + o_ps); R.fit = (double*)(A + o_fit);
    return VBA_OK;
}

// The device part of vba_schur_reliability, shared with vba_schur_snoop: schur_query_device with the landmark marginals from
// ev_begin on, and unless the factorisation failed (*bad != 0: nothing more is launched) the three passes into the reliability
// scratch.  The launches and their order are those vba_schur_reliability has always issued.
static int schur_rel_device(vba_schur_handle h, double lamda, hipEvent_t ev_begin, SchurView& V, int* bad) {
    SchurQuery& Q = h->q;
    SchurRel& R = h->rel;
    hipStream_t s = h->stream;
    if (int rc = schur_query_device(h, lamda, true, ev_begin, V, bad)) return rc;
    if (*bad != 0) return VBA_OK;
    // every output is formed whatever is asked for: what is asked for decides the copies only
    hipLaunchKernelGGL(k_rel_rows, dim3((unsigned)(((size_t)V.m + 255) / 256)), dim3(256), 0, s, V, Q.pair, Q.lp_ptr, Q.lp_blk, Q.lm, R.lev, R.wt, R.om);
    hipLaunchKernelGGL(k_rel_stats, dim3((std::max(V.L, V.n) + 255) / 256), dim3(256), 0, s, V, Q.lm, R.lev, R.wt, R.lmlev, R.lmwt, R.lmom, R.lm_stats,
                       R.pose_stats);
    hipLaunchKernelGGL(k_rel_totals, dim3(1), dim3(256), 0, s, V, R.lev, R.wt, R.om, R.lmlev, R.lmwt, R.lmom, R.fit);
    return VBA_OK;
}

int vba_schur_reliability(vba_schur_handle h, double lamda, double* leverage, double* wtest, double* lm_leverage, double* lm_wtest,
                          double* lm_stats, double* pose_stats, double* fit, int* info) {
    if (!h || !info) return sfail(VBA_EINVAL, "null argument");
    if (h->dyn.enabled) return sfail(VBA_ESTATE, std::string("vba_schur_reliability") + kDynRefusal);
    if (!(lamda >= 0.0)) return sfail(VBA_EINVAL, "lamda must be >= 0");
    if (!h->uploaded || !h->have_state) return sfail(VBA_ESTATE, "upload the problem and set the state first");
    SCHK(hipSetDevice(h->device));
    if (int rc = schur_query_alloc(h)) return rc;
    if (int rc = schur_query_index(h)) return rc;
    if (int rc = schur_rel_alloc(h)) return rc;
    SchurRel& R = h->rel;
    hipStream_t s = h->stream;
    SchurView V;
    int bad = 0;
    if (int rc = schur_rel_device(h, lamda, R.ev[0], V, &bad)) return rc;
    *info = bad;
    const size_t m = (size_t)V.m, L = (size_t)V.L, n = (size_t)V.n;
    struct Out { double* host; const double* dev; size_t count; };
    const Out outs[7] = {{leverage, R.lev, m}, {wtest, R.wt, m}, {lm_leverage, R.lmlev, L}, {lm_wtest, R.lmwt, L}, {lm_stats, R.lm_stats, 3 * L},
                         {pose_stats, R.pose_stats, 3 * n}, {fit, R.fit, 8}};
    if (bad != 0) {                 // no factor, no covariance, no test: NaN, and the row in *info
        SCHK(hipEventRecord(R.ev[1], s));
        SCHK(hipStreamSynchronize(s));
        (void)hipEventElapsedTime(&R.ms, R.ev[0], R.ev[1]);
        for (const Out& o : outs) if (o.host) std::fill(o.host, o.host + o.count, std::nan(""));
        return VBA_OK;
    }
    SCHK(hipEventRecord(R.ev[1], s));
    SCHK(hipGetLastError());
    for (const Out& o : outs) if (o.host) SCHK(hipMemcpyAsync(o.host, o.dev, o.count * 8, hipMemcpyDeviceToHost, s));
    SCHK(hipStreamSynchronize(s));
    (void)hipEventElapsedTime(&R.ms, R.ev[0], R.ev[1]);
    return VBA_OK;
}

int vba_schur_last_reliability_ms(vba_schur_handle h, float* ms) {
    if (!h || !ms) return sfail(VBA_EINVAL, "null argument");
    *ms = h->rel.ms;
    return VBA_OK;
}

// first snoop of a handle: its state (masks cleared) and its two timing events
static int schur_snoop_alloc(vba_schur_handle h) {
    SchurSnoop& Z = h->snoop;
    if (Z.arena) return VBA_OK;
    const SchurView& V = h->V;
    const size_t m = (size_t)V.m, L = (size_t)V.L, n = (size_t)V.n;
    size_t bytes = 0;
    auto need = [&](size_t b) { size_t o = bytes; bytes += (b + 255) & ~size_t(255); return o; };
    const size_t o_sv = need(m * 8), o_cr = need(8), o_rm = need(m), o_lk = need(L), o_ld = need(L * 4), o_pp = need(n * 4), o_ps = need(n * 4),
                 o_po = need(n * 4), o_lo = need(L * 4);
    char* A = nullptr;
    if (hipMalloc(&A, bytes) != hipSuccess) { (void)hipGetLastError(); return sfail(VBA_ENOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes of snooping state failed"); }
    hipEvent_t ev[2] = {};
    if (hipMemset(A, 0, bytes) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess || hipEventCreate(&ev[0]) != hipSuccess ||
        hipEventCreate(&ev[1]) != hipSuccess) {
        if (ev[0]) hipEventDestroy(ev[0]);
        hipFree(A);
        return sfail(VBA_EHIP, "snooping state: hipMemset / event creation failed");
    }
    Z.arena = A; Z.ev[0] = ev[0]; Z.ev[1] = ev[1];
    Z.saved = (double*)(A + o_sv); Z.crit_used = (double*)(A + o_cr); Z.row_mask = (unsigned char*)(A + o_rm); Z.lm_mask = (unsigned char*)(A + o_lk);
    Z.lm_dec = (int*)(A + o_ld); Z.pose_pick = (int*)(A + o_pp); Z.pose_short = (int*)(A + o_ps); Z.pose_out = (int*)(A + o_po); Z.lm_out = (int*)(A + o_lo);
    std::fill(Z.totals, Z.totals + 3, 0);
    return VBA_OK;
}

static SchurSnoopView schur_snoop_view(vba_schur_handle h) {
    const SchurView& V = h->V;
    const SchurSnoop& Z = h->snoop;
    const SchurRel& R = h->rel;
    SchurSnoopView W{};
    W.n = V.n; W.L = V.L; W.m = V.m;
    W.lm_ptr = V.lm_ptr; W.row_pose = V.row_pose; W.row_lm = V.row_lm; W.pose_ptr = V.pose_ptr; W.pose_rows = V.pose_rows;
    W.row_w = const_cast<double*>(V.row_w);
    W.wt = R.wt; W.lmwt = R.lmwt; W.fit = R.fit;
    W.saved = Z.saved; W.row_mask = Z.row_mask; W.lm_mask = Z.lm_mask;
    W.lm_dec = Z.lm_dec; W.pose_pick = Z.pose_pick; W.pose_short = Z.pose_short; W.pose_out = Z.pose_out; W.lm_out = Z.lm_out;
    W.crit_used = Z.crit_used;
    return W;
}

int vba_schur_snoop(vba_schur_handle h, double lamda, double crit, int scaled, int min_rows, int min_track, int* counts, double* crit_used,
                    int* info) {
    if (!h || !info) return sfail(VBA_EINVAL, "null argument");
    if (h->dyn.enabled) return sfail(VBA_ESTATE, std::string("vba_schur_snoop") + kDynRefusal);
    if (!(lamda >= 0.0)) return sfail(VBA_EINVAL, "lamda must be >= 0");
    if (!(crit >= 0.0)) return sfail(VBA_EINVAL, "crit must be >= 0 (+inf rejects nothing)");
    if (min_rows < 0 || min_track < 0) return sfail(VBA_EINVAL, "min_rows and min_track must be >= 0");
    if (!h->uploaded || !h->have_state) return sfail(VBA_ESTATE, "upload the problem and set the state first");
    SCHK(hipSetDevice(h->device));
    if (int rc = schur_query_alloc(h)) return rc;
    if (int rc = schur_query_index(h)) return rc;
    if (int rc = schur_rel_alloc(h)) return rc;
    if (int rc = schur_snoop_alloc(h)) return rc;
    SchurSnoop& Z = h->snoop;
    hipStream_t s = h->stream;
    SchurView V;
    int bad = 0;
    if (int rc = schur_rel_device(h, lamda, Z.ev[0], V, &bad)) return rc;
    *info = bad;
    if (counts) counts[0] = counts[1] = counts[2] = 0;
    if (bad != 0) {                 // no factor, no test: nothing is rejected; the critical value of a fit that does not exist
        SCHK(hipEventRecord(Z.ev[1], s));
        SCHK(hipStreamSynchronize(s));
        (void)hipEventElapsedTime(&Z.ms, Z.ev[0], Z.ev[1]);
        if (crit_used) *crit_used = scaled ? std::nan("") : crit;
        return VBA_OK;
    }
    const SchurSnoopView W = schur_snoop_view(h);
    schur_snoop_launch(W, crit, scaled ? 1 : 0, min_rows, min_track, s);
    SCHK(hipEventRecord(Z.ev[1], s));
    SCHK(hipGetLastError());
    std::vector<int> out;
    try {
        out.resize((size_t)V.n + (size_t)V.L);
    } catch (const std::bad_alloc&) {
        return sfail(VBA_ENOMEM, "host staging for the counts of vba_schur_snoop failed");
    }
    double c = 0.0;
    SCHK(hipMemcpyAsync(out.data(), Z.pose_out, (size_t)V.n * 4, hipMemcpyDeviceToHost, s));
    SCHK(hipMemcpyAsync(out.data() + V.n, Z.lm_out, (size_t)V.L * 4, hipMemcpyDeviceToHost, s));
    SCHK(hipMemcpyAsync(&c, Z.crit_used, 8, hipMemcpyDeviceToHost, s));
    SCHK(hipStreamSynchronize(s));
    (void)hipEventElapsedTime(&Z.ms, Z.ev[0], Z.ev[1]);
    int now[3] = {0, 0, 0};
    for (int i = 0; i < V.n; ++i) now[0] += out[i];
    for (int l = 0; l < V.L; ++l)
        if (out[(size_t)V.n + l] > 0) { now[1] += 1; now[2] += out[(size_t)V.n + l] - 1; }
    for (int k = 0; k < 3; ++k) {
        Z.totals[k] += now[k];
        if (counts) counts[k] = now[k];
    }
    if (crit_used) *crit_used = c;
    return VBA_OK;
}

int vba_schur_rejected(vba_schur_handle h, unsigned char* row_mask, unsigned char* lm_mask, int* totals) {
    if (!h) return sfail(VBA_EINVAL, "null handle");
    const SchurSnoop& Z = h->snoop;
    if (totals) for (int k = 0; k < 3; ++k) totals[k] = Z.arena ? Z.totals[k] : 0;
    if (!Z.arena) {
        if (row_mask) std::memset(row_mask, 0, (size_t)h->V.m);
        if (lm_mask) std::memset(lm_mask, 0, (size_t)h->V.L);
        return VBA_OK;
    }
    SCHK(hipSetDevice(h->device));
    SCHK(hipStreamSynchronize(h->stream));
    if (row_mask) SCHK(hipMemcpy(row_mask, Z.row_mask, (size_t)h->V.m, hipMemcpyDeviceToHost));
    if (lm_mask) SCHK(hipMemcpy(lm_mask, Z.lm_mask, (size_t)h->V.L, hipMemcpyDeviceToHost));
    return VBA_OK;
}

int vba_schur_snoop_restore(vba_schur_handle h) {
    if (!h) return sfail(VBA_EINVAL, "null handle");
    SchurSnoop& Z = h->snoop;
    if (!Z.arena || (Z.totals[0] == 0 && Z.totals[1] == 0 && Z.totals[2] == 0)) return VBA_OK;
    SCHK(hipSetDevice(h->device));
    schur_snoop_restore_launch(schur_snoop_view(h), h->stream);
    SCHK(hipGetLastError());
    SCHK(hipMemsetAsync(Z.lm_mask, 0, (size_t)h->V.L, h->stream));
    SCHK(hipStreamSynchronize(h->stream));
    std::fill(Z.totals, Z.totals + 3, 0);
    return VBA_OK;
}

int vba_schur_last_snoop_ms(vba_schur_handle h, float* ms) {
    if (!h || !ms) return sfail(VBA_EINVAL, "null argument");
    *ms = h->snoop.ms;
    return VBA_OK;
}

// first re-weighting of a handle: its state and its two timing events
static int schur_robust_alloc(vba_schur_handle h) {
    SchurRobust& Z = h->robust;
    if (Z.arena) return VBA_OK;
    const size_t m = (size_t)h->V.m;
    size_t bytes = 0;
    auto need = [&](size_t b) { size_t o = bytes; bytes += (b + 255) & ~size_t(255); return o; };
    const size_t o_b = need(m * 8), o_k = need(m * 16), o_q = need(m * 8), o_p = need((size_t)kRobustMaxBlocks * 8), o_r = need(16),
                 o_s = need(schur_select_scratch_bytes());
    char* A = nullptr;
    if (hipMalloc(&A, bytes) != hipSuccess) { (void)hipGetLastError(); return sfail(VBA_ENOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes of re-weighting state failed"); }
    hipEvent_t ev[2] = {};
    if (hipMemset(A, 0, bytes) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess || hipEventCreate(&ev[0]) != hipSuccess ||
        hipEventCreate(&ev[1]) != hipSuccess) {
        if (ev[0]) hipEventDestroy(ev[0]);
        hipFree(A);
        return sfail(VBA_EHIP, "re-weighting state: hipMemset / event creation failed");
    }
    Z.arena = A; Z.ev[0] = ev[0]; Z.ev[1] = ev[1];
    Z.base = (double*)(A + o_b); Z.keys = (double*)(A + o_k); Z.q = (double*)(A + o_q); Z.part = (double*)(A + o_p); Z.res = (double*)(A + o_r);
    Z.hist = (unsigned long long*)(A + o_s); Z.state = Z.hist + (size_t)kSelPasses * kSelBins;
    Z.captured = Z.have_keys = false;
    return VBA_OK;
}

static SchurRobustView schur_robust_view(vba_schur_handle h) {
    const SchurView& V = h->V;
    const SchurRobust& Z = h->robust;
    SchurRobustView W{};
    W.n = V.n; W.L = V.L; W.m = V.m;
    W.row_pose = V.row_pose; W.row_lm = V.row_lm; W.row_u = V.row_u; W.row_v = V.row_v; W.intr = V.intr;
    W.states = h->S0; W.X = h->X0buf;
    W.row_w = const_cast<double*>(V.row_w);
    W.saved = h->snoop.arena ? h->snoop.saved : nullptr;
    W.row_mask = h->snoop.arena ? h->snoop.row_mask : nullptr;
    W.base = Z.base; W.keys = Z.keys; W.q = Z.q; W.part = Z.part; W.res = Z.res;
    W.sel.keys = reinterpret_cast<const unsigned long long*>(Z.keys); W.sel.count = 2 * V.m;
    W.sel.hist = Z.hist; W.sel.state = Z.state; W.sel.out = Z.res;
    return W;
}

int vba_schur_reweight(vba_schur_handle h, double alpha, double* c_obs, double* w_max, int* status) {
    if (!h || !c_obs || !w_max || !status) return sfail(VBA_EINVAL, "null argument");
    if (!(alpha >= 1.0 && alpha <= 2.0)) return sfail(VBA_EINVAL, "alpha must lie in [1, 2]");
    if (!h->uploaded || !h->have_state) return sfail(VBA_ESTATE, "upload the problem and set the state first");
    SCHK(hipSetDevice(h->device));
    if (int rc = schur_robust_alloc(h)) return rc;
    SchurRobust& Z = h->robust;
    hipStream_t s = h->stream;
    const SchurRobustView W = schur_robust_view(h);
    if (!Z.captured) {
        schur_robust_capture_launch(W, s);
        SCHK(hipGetLastError());
        Z.captured = true;
    }
    SCHK(hipEventRecord(Z.ev[0], s));
    Z.launches = schur_robust_launch(W, alpha, s);
    SCHK(hipEventRecord(Z.ev[1], s));
    SCHK(hipGetLastError());
    double res[2] = {0.0, 0.0};
    SCHK(hipMemcpyAsync(res, Z.res, 16, hipMemcpyDeviceToHost, s));
    SCHK(hipStreamSynchronize(s));
    (void)hipEventElapsedTime(&Z.ms, Z.ev[0], Z.ev[1]);
    Z.have_keys = true;
    const bool ok = res[0] > 0.0 && std::isfinite(res[0]) && res[1] > 0.0 && std::isfinite(res[1]);     // (the test of k_schur_robust_scale)
    *c_obs = res[0];
    *w_max = ok ? res[1] : std::nan("");
    *status = ok ? 0 : 1;
    return VBA_OK;
}

int vba_schur_get_weights(vba_schur_handle h, double* w, double* base) {
    if (!h) return sfail(VBA_EINVAL, "null handle");
    if (!h->uploaded) return sfail(VBA_ESTATE, "upload the problem first");
    SCHK(hipSetDevice(h->device));
    SCHK(hipStreamSynchronize(h->stream));
    const size_t m = (size_t)h->V.m;
    if (w) SCHK(hipMemcpy(w, h->V.row_w, m * 8, hipMemcpyDeviceToHost));
    if (!base) return VBA_OK;
    if (h->robust.arena && h->robust.captured) {
        SCHK(hipMemcpy(base, h->robust.base, m * 8, hipMemcpyDeviceToHost));
        return VBA_OK;
    }
    SCHK(hipMemcpy(base, h->V.row_w, m * 8, hipMemcpyDeviceToHost));
    if (h->snoop.arena) {           // never re-weighted: the weights in place, a rejected row by its saved value
        std::vector<double> saved;
        std::vector<unsigned char> mask;
        try {
            saved.resize(m);
            mask.resize(m);
        } catch (const std::bad_alloc&) {
            return sfail(VBA_ENOMEM, "host staging for vba_schur_get_weights failed");
        }
        SCHK(hipMemcpy(saved.data(), h->snoop.saved, m * 8, hipMemcpyDeviceToHost));
        SCHK(hipMemcpy(mask.data(), h->snoop.row_mask, m, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < m; ++k) if (mask[k]) base[k] = saved[k];
    }
    return VBA_OK;
}

int vba_schur_last_reweight_ms(vba_schur_handle h, float* ms) {
    if (!h || !ms) return sfail(VBA_EINVAL, "null argument");
    *ms = h->robust.ms;
    return VBA_OK;
}

int vba_schur_median(int device, const double* keys, int64_t count, double* median) {
    if (!keys || !median) return sfail(VBA_EINVAL, "null argument");
    if (count < 1 || count > (int64_t)1 << 31) return sfail(VBA_EINVAL, "count must lie in [1, 2^31]");
    for (int64_t k = 0; k < count; ++k)
        if (std::isnan(keys[k]) || std::signbit(keys[k])) return sfail(VBA_EINVAL, "keys must be non-negative doubles (no NaN, no sign bit)");
    int cnt = 0, prev = -1;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt == 0) return sfail(VBA_ENODEV, "no HIP device visible");
    if (device < 0 || device >= cnt) return sfail(VBA_EINVAL, "device index out of range");
    std::lock_guard<std::mutex> lk(g_median_ws.m);
    MedianWorkspace& G = g_median_ws;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    struct Back {                   // the caller's HIP device, whatever happens below
        int dev;
        ~Back() { if (dev >= 0) (void)hipSetDevice(dev); }
    } back{prev};
    SCHK(hipSetDevice(device));
    const size_t kb = ((size_t)count * 8 + 255) & ~size_t(255), sb = (schur_select_scratch_bytes() + 255) & ~size_t(255);
    const size_t need = kb + sb + 256;
    if (G.device != device || G.size < need) {
        if (G.base) (void)hipFree(G.base);
        G.base = nullptr;
        G.size = 0;
        if (!G.stream || G.device != device) {
            if (G.stream) (void)hipStreamDestroy(G.stream);
            G.stream = nullptr;
            G.device = -1;
            SCHK(hipStreamCreateWithFlags(&G.stream, hipStreamNonBlocking));
        }
        if (hipMalloc(&G.base, need + need / 2) != hipSuccess) { (void)hipGetLastError(); G.base = nullptr; return sfail(VBA_ENOMEM, "hipMalloc of the median workspace failed"); }
        G.size = need + need / 2;
        G.device = device;
    }
    SchurSelectView W{};
    W.keys = reinterpret_cast<const unsigned long long*>(G.base);
    W.count = count;
    W.hist = reinterpret_cast<unsigned long long*>(G.base + kb);
    W.state = W.hist + (size_t)kSelPasses * kSelBins;
    W.out = reinterpret_cast<double*>(G.base + kb + sb);
    SCHK(hipMemcpyAsync(G.base, keys, (size_t)count * 8, hipMemcpyHostToDevice, G.stream));
    schur_select_launch(W, G.stream, nullptr);
    SCHK(hipGetLastError());
    SCHK(hipMemcpyAsync(median, W.out, 8, hipMemcpyDeviceToHost, G.stream));
    SCHK(hipStreamSynchronize(G.stream));
    return VBA_OK;
}

int vba_schur_enable_dynamics(vba_schur_handle h, const int* time_idx, double sigma_dyn) {
    if (!h || !time_idx) return sfail(VBA_EINVAL, "null argument");
    if (!h->uploaded) return sfail(VBA_ESTATE, "upload the problem first");
    if (h->dyn.enabled) return sfail(VBA_ESTATE, "the dynamics factor is already enabled on this handle");
    if (!(sigma_dyn > 0.0) || !std::isfinite(sigma_dyn)) return sfail(VBA_EINVAL, "sigma_dyn must be positive and finite");
    SchurView& V = h->V;
    const int n = V.n;
    if (n < 2) return sfail(VBA_EINVAL, "the dynamics factor needs at least two poses");
    std::vector<int> steps(n - 1);
    for (int i = 0; i + 1 < n; ++i) {
        const int64_t d = (int64_t)time_idx[i + 1] - (int64_t)time_idx[i];
        if (d < 1) return sfail(VBA_EINVAL, "time_idx must increase: poses " + std::to_string(i) + " and " + std::to_string(i + 1));
        if (d > kSchurDynMaxGap)
            return sfail(VBA_EINVAL, "a gap of " + std::to_string(d) + " steps between poses " + std::to_string(i) + " and " + std::to_string(i + 1) +
                                         ": the dynamics factor of this mode covers gaps of 1 .. " + std::to_string(kSchurDynMaxGap) + " steps");
        steps[i] = (int)d;
    }
    SCHK(hipSetDevice(h->device));
    SCHK(hipStreamSynchronize(h->stream));
    const int N = 9 * n, nb = (N + kT * kPanel - 1) / (kT * kPanel) * kPanel, Npad = nb * kT;
    SchurDyn& D = h->dyn;
    const int npart = schur_dyn_partials(n);
    size_t bytes = 0;
    auto need = [&](size_t b) { size_t o = bytes; bytes += (b + 255) & ~size_t(255); return o; };
    const size_t o_S = need((size_t)Npad * Npad * 8), o_g = need((size_t)Npad * 8), o_y = need((size_t)Npad * 8), o_iL = need((size_t)nb * kT * kT * 8);
    const size_t o_st = need((size_t)(n - 1) * 4), o_r = need((size_t)(n - 1) * 48), o_A = need((size_t)(n - 1) * 288), o_ec = need((size_t)(n - 1) * 8),
                 o_part = need((size_t)npart * 8);
    char* A = nullptr;
    if (hipMalloc(&A, bytes) != hipSuccess) { (void)hipGetLastError(); return sfail(VBA_ENOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes for the dynamics factor failed"); }
    if (hipMemset(A, 0, bytes) != hipSuccess || hipMemcpy(A + o_st, steps.data(), (size_t)(n - 1) * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipStreamSynchronize(nullptr) != hipSuccess) {
        hipFree(A);
        return sfail(VBA_EHIP, "dynamics factor: hipMemset / upload failed");
    }
    // the scratch of the queries was sized for 6 n: they refuse this handle from now on, so it goes
    if (h->rel.arena) { hipFree(h->rel.arena); for (hipEvent_t e : h->rel.ev) if (e) hipEventDestroy(e); h->rel = SchurRel{}; }
    if (h->q.arena) { hipFree(h->q.arena); for (hipEvent_t e : h->q.ev) if (e) hipEventDestroy(e); h->q = SchurQuery{}; }
    D.arena = A; D.sigma = sigma_dyn; D.npart = npart;
    D.steps = (int*)(A + o_st); D.r = (double*)(A + o_r); D.A = (double*)(A + o_A); D.ecost = (double*)(A + o_ec); D.part = (double*)(A + o_part);
    D.h_part.assign(npart, 0.0);
    // (the 6 n arrays of vba_schur_create stay in the handle's arena, unused: one allocation, freed with the handle)
    V.N = N; V.nb = nb; V.Npad = Npad;
    V.S = (double*)(A + o_S); V.g = (double*)(A + o_g); V.ybuf = (double*)(A + o_y); V.invL = (double*)(A + o_iL);
    h->bw = nb - 1;             // velocity rows reach every pose column: the substitutions cover every tile of the factor
    D.enabled = true;
    return VBA_OK;
}

int vba_schur_last_info(vba_schur_handle h, int* info) {
    if (!h || !info) return sfail(VBA_EINVAL, "null argument");
    *info = h->last_info;
    return VBA_OK;
}

int vba_schur_last_ms(vba_schur_handle h, float* build_ms, float* factor_ms, float* solve_ms) {
    if (!h) return sfail(VBA_EINVAL, "null handle");
    if (build_ms) *build_ms = h->ms[0];
    if (factor_ms) *factor_ms = h->ms[1];
    if (solve_ms) *solve_ms = h->ms[2];
    return VBA_OK;
}

// what: 0 = step of the last iteration [6 n + 3 L] (dc then dl), 1 = lower triangle of the Cholesky factor as a dense
// [N][N] row-major matrix (upper part zero; N = 6 n, or 9 n with the dynamics factor), 2 = the 2 m keys |r| of the last
// re-weighting; with the dynamics factor 3 = dv [n][3] of the last iteration, 4 = r [n - 1][6], 5 = D Phi [n - 1][6][6] and
// 6 = sigma_dyn |r_e|^2 [n - 1] of its build
int vba_schur_debug_fetch(vba_schur_handle h, int what, double* out, int64_t capacity) {
    if (!h || !out) return sfail(VBA_EINVAL, "null argument");
    SCHK(hipSetDevice(h->device));
    SCHK(hipStreamSynchronize(h->stream));
    const SchurView& V = h->V;
    if (what == 0) {
        const int64_t n6 = 6 * (int64_t)V.n;      // (the pose unknowns come first, with or without the velocities behind them)
        if (capacity < n6 + 3 * (int64_t)V.L) return sfail(VBA_EINVAL, "buffer too small");
        SCHK(hipMemcpy(out, V.g, (size_t)n6 * 8, hipMemcpyDeviceToHost));
        SCHK(hipMemcpy(out + n6, V.dl, (size_t)V.L * 24, hipMemcpyDeviceToHost));
        return VBA_OK;
    }
    if (what >= 3 && what <= 6) {
        const SchurDyn& D = h->dyn;
        if (!D.enabled) return sfail(VBA_ESTATE, "the dynamics factor is not enabled on this handle");
        const int64_t n = V.n;
        const double* src[4] = {V.g + 6 * n, D.r, D.A, D.ecost};
        const int64_t count[4] = {3 * n, 6 * (n - 1), 36 * (n - 1), n - 1};
        if (capacity < count[what - 3]) return sfail(VBA_EINVAL, "buffer too small");
        SCHK(hipMemcpy(out, src[what - 3], (size_t)count[what - 3] * 8, hipMemcpyDeviceToHost));
        return VBA_OK;
    }
    if (what == 1) {
        if (capacity < (int64_t)V.N * V.N) return sfail(VBA_EINVAL, "buffer too small");
        std::vector<double> tmp((size_t)V.Npad * V.Npad);
        SCHK(hipMemcpy(tmp.data(), V.S, tmp.size() * 8, hipMemcpyDeviceToHost));
        for (int r = 0; r < V.N; ++r)
            for (int c = 0; c < V.N; ++c) out[(size_t)r * V.N + c] = c <= r ? tmp[(size_t)r * V.Npad + c] : 0.0;
        return VBA_OK;
    }
    if (what == 2) {
        if (!h->robust.arena || !h->robust.have_keys) return sfail(VBA_ESTATE, "no re-weighting since the upload");
        if (capacity < 2 * V.m) return sfail(VBA_EINVAL, "buffer too small");
        SCHK(hipMemcpy(out, h->robust.keys, (size_t)V.m * 16, hipMemcpyDeviceToHost));
        return VBA_OK;
    }
    return sfail(VBA_EINVAL, "unknown selector");
}

}  // extern "C"
