// vba_schur_cov.hip -- the covariance query of the free-landmark mode (vba_schur_covariance, and vba_schur_covariance_dyn on a handle
// with the dynamics factor: the same stages over [6 n pose | 3 n velocity] unknowns; include/vinsat_ba.h carries the contracts): build
// and factor into scratch of its own, then the selected blocks of the inverse.  One device part serves both (schur_query_device); it is
// what the reliability, snoop and outlier power queries start with.  vba_schur.hip carries the map of the units.
#include "vba_schur_context.h"
#include "vba_schur_dyn_cov.h"

namespace {

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

// Tile (I, J), I >= J, of S^-1 = W^T W:  sum_{K = I}^{nbu - 1} W_KI^T W_KJ  (W_KI = 0 above the diagonal), K upwards, by one block;
// diagonal tiles are stored whole.  out may be the array the factor lived in: W is all this reads.  The one body of k_syrk_wtw and
// k_syrk_wtw_sel: a tile has the same bits from either.
__device__ __forceinline__ void syrk_wtw_tile(const SchurView& V, const double* W, double* out, int nbu, int I, int J) {
    __shared__ double As[kT][kT + 1];
    __shared__ double Bs[kT][kT + 1];
    const int t = threadIdx.x;
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

// every tile of the lower triangle, one block each (enumerated as k_gemm_abt<1> does)
__global__ __launch_bounds__(256) void k_syrk_wtw(SchurView V, const double* W, double* out, int nbu) {
    const int q = blockIdx.x;
    int I = (int)((sqrt(8.0 * q + 1.0) - 1.0) * 0.5);
    while ((I + 1) * (I + 2) / 2 <= q) ++I;
    while (I * (I + 1) / 2 > q) --I;
    syrk_wtw_tile(V, W, out, nbu, I, q - I * (I + 1) / 2);
}

// The listed tiles only (tiles: I, J per tile, I >= J, both below nbu -- schur_dyn_cov_tiles), one block each.  The other tiles of
// out keep what was there (the factor) and are never read.
__global__ __launch_bounds__(256) void k_syrk_wtw_sel(SchurView V, const double* W, double* out, int nbu, const int* tiles) {
    syrk_wtw_tile(V, W, out, nbu, tiles[2 * blockIdx.x], tiles[2 * blockIdx.x + 1]);
}

// The 9x9 blocks of vba_schur_covariance_dyn, thread per entry: state[i] = Sigma(x_i, x_i) and edge[i] = Sigma(x_i, x_{i+1}) over
// x = [dp, dtheta, dv], read from the stored lower triangle of S9^-1 through the map of vba_schur_dyn_cov.h.  A state block is
// exactly symmetric (both mirror entries read one stored entry), and its pose part has the bits k_cov_gather gives pose_cov.
__global__ __launch_bounds__(256) void k_state_gather(SchurView V, const double* Sinv, double* state, double* edge) {
    const int e = blockIdx.x * 256 + threadIdx.x, ns = 81 * V.n;
    if (e >= 81 * (2 * V.n - 1)) return;
    const SchurEntry s = schur_state_gather_entry(V.n, e);
    const double v = Sinv[(size_t)s.r * V.Npad + s.c];
    if (e < ns) state[e] = v;
    else edge[e - ns] = v;
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

}  // namespace

// first query of a handle: the scratch and its two timing events
int schur_query_alloc(vba_schur_handle h) {
    SchurQuery& Q = h->q;
    if (Q.sc.arena) return VBA_OK;
    const SchurView& V = h->V;
    const size_t m = (size_t)V.m, L = (size_t)V.L, NN = (size_t)V.Npad * V.Npad * 8;
    SchurLayout lay;
    const size_t o_ci = lay.need(L * 48), o_wl = lay.need(L * 24), o_E = lay.need(m * 144), o_Y = lay.need(m * 144), o_S = lay.need(NN),
                 o_g = lay.need((size_t)V.Npad * 8), o_y = lay.need((size_t)V.Npad * 8), o_iL = lay.need((size_t)V.nb * kT * kT * 8),
                 o_dl = lay.need(L * 24), o_W = lay.need(NN), o_pair = lay.need((size_t)V.nblk * 288), o_pose = lay.need((size_t)V.n * 288),
                 o_lm = lay.need(L * 72), o_info = lay.need(256), o_lpp = lay.need((L + 1) * 4), o_lpb = lay.need((size_t)h->npairs * 4);
    // a handle with the dynamics factor (V.Npad is 9 n based there): the outputs of vba_schur_covariance_dyn, the tile list of its
    // selected product (at most every tile that holds unknowns) and the dynamics arrays of its build
    const bool dyn = h->dyn.enabled;
    const size_t ne = dyn ? (size_t)V.n - 1 : 0, nbu = (size_t)(V.N + kT - 1) / kT;
    const size_t o_st = lay.need(dyn ? (size_t)V.n * 648 : 0), o_ed = lay.need(ne * 648), o_tl = lay.need(dyn ? nbu * (nbu + 1) * 4 : 0),
                 o_dr = lay.need(ne * 48), o_dA = lay.need(ne * 288), o_de = lay.need(ne * 8), o_dp = lay.need(dyn ? (size_t)h->dyn.npart * 8 : 0);
    if (int rc = schur_scratch_alloc(Q.sc, lay.bytes, "query scratch")) return rc;
    char* A = Q.sc.arena;
    if (dyn) {
        Q.state = (double*)(A + o_st); Q.edge = (double*)(A + o_ed); Q.tiles = (int*)(A + o_tl);
        Q.dyn_r = (double*)(A + o_dr); Q.dyn_A = (double*)(A + o_dA); Q.dyn_ecost = (double*)(A + o_de); Q.dyn_part = (double*)(A + o_dp);
    }
    Q.Cinv = (double*)(A + o_ci); Q.wl = (double*)(A + o_wl); Q.E = (double*)(A + o_E); Q.Y = (double*)(A + o_Y); Q.S = (double*)(A + o_S);
    Q.g = (double*)(A + o_g); Q.ybuf = (double*)(A + o_y); Q.invL = (double*)(A + o_iL); Q.dl = (double*)(A + o_dl); Q.W = (double*)(A + o_W);
    Q.pair = (double*)(A + o_pair); Q.pose = (double*)(A + o_pose); Q.lm = (double*)(A + o_lm); Q.info = (int*)(A + o_info);
    Q.lp_ptr = (int*)(A + o_lpp); Q.lp_blk = (int*)(A + o_lpb);
    return VBA_OK;
}

// Once per upload: for every landmark the block of each of its row pairs (k >= k'), in the order k_lm_cov walks them.  The pair
// lists are grouped by block; they are read back and turned round on the host, and checked on the way (every pair of every
// landmark exactly once, in the block of its two poses; every diagonal block listed): k_lm_cov and k_cov_gather rely on that.
int schur_query_index(vba_schur_handle h) {
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
    if (h->dyn.enabled) {       // the tiles of S9^-1 the outputs of vba_schur_covariance_dyn read (the block list was checked at the upload)
        std::vector<int> tiles;
        schur_dyn_cov_tiles(V.n, V.nblk, bi.data(), bj.data(), kT, tiles);
        SCHK(hipMemcpy(Q.tiles, tiles.data(), tiles.size() * 4, hipMemcpyHostToDevice));
        Q.ntiles = (int)(tiles.size() / 2);
    }
    Q.indexed = true;
    return VBA_OK;
}

// the view a query builds: the handle's problem at its resident state and this damping, everything written in the query's scratch
static SchurView query_view(vba_schur_handle h, double lamda) {
    const SchurQuery& Q = h->q;
    SchurView V = h->V;
    V.lamda = lamda;
    V.states = h->S0; V.X = h->X0buf; V.states_new = nullptr; V.X_new = nullptr; V.part = nullptr;
    V.Cinv = Q.Cinv; V.wl = Q.wl; V.E = Q.E; V.Y = Q.Y; V.S = Q.S; V.g = Q.g; V.ybuf = Q.ybuf; V.invL = Q.invL; V.dl = Q.dl;
    return V;
}

// The device part of the covariance query, shared with the reliability query (vba_schur_rel.hip): ev_begin, then build and factorise
// into the query's scratch at this damping (V: the view that was built -- the handle's problem, everything written in the scratch),
// the info word to the host (*bad), and unless the factorisation failed the selected inverse, the gathered blocks (Q.pair, Q.pose)
// and, with with_lm, the landmark marginals (Q.lm).  On a handle with the dynamics factor (the entries check the kind first, so the
// handle decides): the dynamics blocks of the build go through arrays of the scratch (DW; TW likewise on a handle with the attitude
// factor, so debug_fetch 7 .. 9 stay the last iterate's; PW on a handle with the state prior, for 10 .. 12), W is needed in full (h->bw = nb - 1: nothing skipped), the product forms the
// listed tiles of S9^-1 only (every tile with VBA_SCHUR_COV_FULL=1), the 9x9 blocks are gathered (Q.state, Q.edge), and k_cov_gather /
// k_lm_cov run as they are: they index by V.Npad and read the top-left 6 n x 6 n only (E9 has no velocity rows, so the landmark
// formula stands).  The reliability query reads what this leaves resident: Q.state, Q.edge, Q.pair, Q.lm, Q.dyn_A, Q.dyn_ecost.  The
// launches and their order are those the two queries have always issued.
int schur_query_device(vba_schur_handle h, double lamda, bool with_lm, hipEvent_t ev_begin, SchurView& V, int* bad) {
    SchurQuery& Q = h->q;
    hipStream_t s = h->stream;
    const bool dyn = h->dyn.enabled, att = dyn && h->att.enabled;
    V = query_view(h, lamda);
    SchurDynView DW{};
    SchurAttView TW{};
    if (dyn) {
        DW = schur_dyn_view(h, V);
        DW.r = Q.dyn_r; DW.A = Q.dyn_A; DW.ecost = Q.dyn_ecost; DW.part = Q.dyn_part;
    }
    if (att) TW = schur_att_view(h, V, true);
    const bool prior = dyn && h->prior.enabled;
    SchurPriorView PW{};
    if (prior) PW = schur_prior_view(h, V, true);
    SCHK(hipEventRecord(ev_begin, s));
    if (int rc = schur_build_factor(h, V, s, Q.info, nullptr, dyn ? &DW : nullptr, att ? &TW : nullptr, prior ? &PW : nullptr)) return rc;
    SCHK(hipGetLastError());
    *bad = 0;
    SCHK(hipMemcpyAsync(bad, Q.info, 4, hipMemcpyDeviceToHost, s));
    SCHK(hipStreamSynchronize(s));
    if (*bad != 0) return VBA_OK;
    const int nbu = (V.N + kT - 1) / kT;
    const size_t n_pair = (size_t)V.nblk * 36;
    for (int d = 0; d < nbu; ++d) hipLaunchKernelGGL(k_trinv_step, dim3(nbu - d), dim3(256), 0, s, V, Q.W, d, h->bw);
    // (over the factor: no longer needed)
    if (!dyn || h->cov_full) hipLaunchKernelGGL(k_syrk_wtw, dim3(nbu * (nbu + 1) / 2), dim3(256), 0, s, V, Q.W, Q.S, nbu);
    else hipLaunchKernelGGL(k_syrk_wtw_sel, dim3(Q.ntiles), dim3(256), 0, s, V, Q.W, Q.S, nbu, Q.tiles);
    if (dyn) hipLaunchKernelGGL(k_state_gather, dim3((81 * (2 * V.n - 1) + 255) / 256), dim3(256), 0, s, V, Q.S, Q.state, Q.edge);
    hipLaunchKernelGGL(k_cov_gather, dim3((unsigned)((n_pair + 255) / 256)), dim3(256), 0, s, V, Q.S, Q.pair, Q.pose);
    if (with_lm) hipLaunchKernelGGL(k_lm_cov, dim3((V.L + 255) / 256), dim3(256), 0, s, V, Q.pair, Q.lp_ptr, Q.lp_blk, Q.lm);
    return VBA_OK;
}

// Behind the checks of the two entries: the scaffold, the device part from the query's own ev[0], *info, and the outputs -- the
// leading blocks are [n] 6x6 pose blocks or [n] 9x9 state and [n - 1] 9x9 edge blocks, pair_cov and lm_cov follow for both.
static int schur_cov_call(vba_schur_handle h, SchurKind kind, double lamda, double* lead_cov, double* edge_cov, double* pair_cov, double* lm_cov,
                          int* info) {
    if (int rc = schur_query_begin(h, kind, kind == kSchurPlain ? "vba_schur_covariance" : nullptr)) return rc;
    SchurQuery& Q = h->q;
    SchurView V;
    int bad = 0;
    if (int rc = schur_query_device(h, lamda, lm_cov != nullptr, Q.sc.ev[0], V, &bad)) return rc;
    *info = bad;
    const size_t n = (size_t)V.n;
    const bool dyn = kind != kSchurPlain;
    const Out outs[4] = {{lead_cov, dyn ? Q.state : Q.pose, dyn ? n * 81 : n * 36}, {edge_cov, Q.edge, dyn ? (n - 1) * 81 : 0},
                         {pair_cov, Q.pair, (size_t)V.nblk * 36}, {lm_cov, Q.lm, (size_t)V.L * 9}};
    return schur_outputs_finish(Q.sc, h->stream, bad, outs, 4);
}

extern "C" {

int vba_schur_covariance_dyn(vba_schur_handle h, double lamda, double* state_cov, double* edge_cov, double* pair_cov, double* lm_cov, int* info) {
    if (!h || !info || !state_cov || !edge_cov) return sfail(VBA_EINVAL, "null argument");
    if (!(lamda >= 0.0)) return sfail(VBA_EINVAL, "lamda must be >= 0");
    return schur_cov_call(h, kSchurDyn, lamda, state_cov, edge_cov, pair_cov, lm_cov, info);
}

int vba_schur_last_covariance_dyn_ms(vba_schur_handle h, float* ms) { return schur_last_ms(h, &vba_schur_context::q, ms); }

int vba_schur_covariance(vba_schur_handle h, double lamda, double* pose_cov, double* pair_cov, double* lm_cov, int* info) {
    if (!h || !info) return sfail(VBA_EINVAL, "null argument");
    if (int rc = schur_kind_check(kSchurPlain, h, "vba_schur_covariance")) return rc;
    if (!(lamda >= 0.0)) return sfail(VBA_EINVAL, "lamda must be >= 0");
    return schur_cov_call(h, kSchurPlain, lamda, pose_cov, nullptr, pair_cov, lm_cov, info);
}

int vba_schur_last_covariance_ms(vba_schur_handle h, float* ms) { return schur_last_ms(h, &vba_schur_context::q, ms); }

}  // extern "C"
