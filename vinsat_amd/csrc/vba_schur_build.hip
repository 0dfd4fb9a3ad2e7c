// vba_schur_build.hip -- the build stage of the free-landmark mode: the reduced camera system S, g and what the back substitution
// needs (Cinv, wl, E, Y) from the view's state, weights and damping.  vba_schur.hip carries the map of the units; the view and the
// row geometry are vba_schur_context.h's.
#include "vba_schur_context.h"
#include "vba_schur_dyn_long.h"

namespace {

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

}  // namespace

void schur_build_launch(vba_schur_handle h, const SchurView& V, hipStream_t s, const SchurDynView* dyn, const SchurAttView* att,
                        const SchurPriorView* prior) {
    hipLaunchKernelGGL(k_lm_blocks, dim3((V.L + 255) / 256), dim3(256), 0, s, V);
    hipLaunchKernelGGL(k_pose_blocks, dim3((V.n + 15) / 16), dim3(256), 0, s, V);
    hipLaunchKernelGGL(k_pair_blocks, dim3(V.nblk), dim3(64), 0, s, V);
    if (h->dyn.enabled) {       // the dynamics blocks on top of the reprojection blocks (vba_schur_covariance_dyn brings arrays of its own)
        const SchurDynView W = dyn ? *dyn : schur_dyn_view(h, V);
        schur_dyn_edges_launch(W, V.states, s);
        if (W.nlong > 0) schur_dyn_long_edges_launch(W, V.states, s);      // the edges k_sdyn_edges left alone
        schur_dyn_scatter_launch(W, s);
        if (h->att.enabled) {   // the attitude blocks behind them: symmetric positive semidefinite, on the attitude unknowns alone
            const SchurAttView T = att ? *att : schur_att_view(h, V);
            schur_att_edges_launch(T, V.states, s);
            schur_att_scatter_launch(T, s);
        }
        if (h->prior.enabled) { // the state prior's blocks behind both: symmetric, on the 9x9 blocks of the chosen poses alone
            const SchurPriorView P = prior ? *prior : schur_prior_view(h, V);
            schur_prior_terms_launch(P, V.states, s);
            schur_prior_scatter_launch(P, s);
        }
    }
    if (V.Npad > V.N) hipLaunchKernelGGL(k_pad_identity, dim3((V.Npad - V.N + 63) / 64), dim3(64), 0, s, V);
}
