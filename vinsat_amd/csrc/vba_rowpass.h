// vba_rowpass.h -- the row pass behind the covariance step, defined once (device only): what k_reliability (vba_rel.hip) and
// k_outlier_power (vba_power.hip) do before their own per-row tails, stores and pose summaries.
//
// Mapping: one pass over the pose-sorted SoA observation block of every window, with the row-to-lane mapping of the accumulation
// (k_obs_accumulate<16>): 16 lanes -- one DPP row -- per pose, 16 poses per block of 256, lane `sub` takes rows beg + sub, + 16, ...
// of the pose's CSR segment, so a group reads 128 contiguous bytes of each stream per step.  S_i (21 unique doubles) is loaded once
// per lane into registers: the 16 lanes of a group read the same addresses (one request, broadcast) and keep the block for all
// their rows.  Reads per row: six observation doubles, wraw, the 4-byte input position; the next row is requested one step ahead.
// Per pose the 16 partial results meet in a butterfly of four DPP exchanges whose shape does not depend on anything (group16_sum,
// group16_max) -- no atomics, equal settings give equal bits, and no setting of the handle changes the mapping: a window has the
// same bits alone and in any batch.
//
// Arithmetic: J_k in fp64 by the closed forms of vba_math.h, T = S_i J_k^T, the symmetric part of J_k T, and from it the leverage
// and the w-test of a row of non-zero weight.  The last is written operation by operation with contraction off, so its bits do
// not depend on which products a compiler would fold into an fma.
#pragma once
#include "vba_device.h"

namespace vba {

constexpr int kRowLanes = 16;                           // lanes per pose: one DPP row
constexpr int kRowPosesPerBlock = 256 / kRowLanes;

inline dim3 rowpass_grid(int n_max, int W) { return dim3((n_max + kRowPosesPerBlock - 1) / kRowPosesPerBlock, W); }

// What the 16 lanes of a pose share.  diag [W][n_max][81] Sigma_ii, flags [W] of the covariance step; perm [W][m_max] sorted
// position -> input row.
struct RowGroup {
    int i, sub, m, beg, end;
    bool live;              // (uniform over the 16 lanes of a group: the exchanges of the summary stay inside one)
    bool no_sigma;          // the covariance step flagged the window: it has no Sigma
    size_t ob, mb, pb;      // the window's observation block and row arrays, the pose's index in [W][n_max] arrays
    double inv_wmax;
    const int* pw;          // perm of the window
    PoseCam pc;
    double S[21];           // upper triangle of S_i = Sigma_ii[:6, :6], packed as sym6
};

struct Row { double x, y, z, u, v, c, wr; int p; };

__device__ __forceinline__ Row row_load(const DevView& V, const RowGroup& g, int k) {
    Row o;
    o.x = V.ox[g.ob + k]; o.y = V.oy[g.ob + k]; o.z = V.oz[g.ob + k];
    o.u = V.ou[g.ob + k]; o.v = V.ov[g.ob + k]; o.c = V.oconf[g.ob + k];
    o.wr = V.wraw[g.mb + k];
    o.p = g.pw[k];
    return o;
}

// Row k of the lane (held in nxt), and the request for row k + 16
__device__ __forceinline__ Row row_take(const DevView& V, const RowGroup& g, int k, Row& nxt) {
    const Row o = nxt;
    if (k + kRowLanes < g.end) nxt = row_load(V, g, k + kRowLanes);
    return o;
}

// The mapping alone: the group of this thread, its rows and the window's scalars -- all a pass needs that reads stored row
// results and no Sigma (k_snoop_pick, vba_snoop.hip); pc and S stay unset.  False for a block beyond the window's poses.
__device__ __forceinline__ bool rowpass_rows(const DevView& V, const unsigned* __restrict__ flags, const int* __restrict__ perm,
                                             RowGroup& g) {
    const int w = blockIdx.y;
    const int n = V.n[w];
    g.m = V.m[w];
    if (blockIdx.x * kRowPosesPerBlock >= n) return false;
    g.i = blockIdx.x * kRowPosesPerBlock + threadIdx.x / kRowLanes;
    g.sub = threadIdx.x % kRowLanes;
    g.live = g.i < n;
    g.ob = (size_t)w * V.obs_stride;
    g.mb = (size_t)w * V.m_max;
    g.pb = (size_t)w * V.n_max + (g.live ? g.i : 0);
    const int* ptr = V.pose_ptr + 2 * g.ob;
    g.beg = g.live ? ptr[g.i] : 0;
    g.end = g.live ? min(ptr[g.i + 1], g.m) : 0;
    g.no_sigma = (flags[w] & (VBA_FLAG_ZERO_PIVOT | VBA_FLAG_NONFINITE)) != 0u;
    g.inv_wmax = 1.0 / bits_f64(V.sc[w].wmax_bits[V.par]);
    g.pw = perm + g.mb;
    return true;
}

// The group of this thread and its first row.  False for a block beyond the window's poses (block uniform).
__device__ __forceinline__ bool rowpass_begin(const DevView& V, const double* __restrict__ diag, const unsigned* __restrict__ flags,
                                              const int* __restrict__ perm, RowGroup& g, Row& nxt) {
    if (!rowpass_rows(V, flags, perm, g)) return false;
    // the first row is requested before the pose's camera and covariance block: independent round trips side by side
    nxt = Row{};
    if (g.beg + g.sub < g.end) nxt = row_load(V, g, g.beg + g.sub);
    g.pc = PoseCam{};
#pragma unroll
    for (int q = 0; q < 21; ++q) g.S[q] = 0.0;
    if (g.live) {
        pose_camera(V.states + g.pb * 10, V.intr + g.pb * 4, g.pc);
        const double* Sp = diag + g.pb * 81;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b) g.S[sym6(a, b)] = Sp[a * 9 + b];
    }
    return true;
}

// Residual r = uv - est, final robust weight w = (w_raw / w_max) conf, T = S J^T (6x2, columns t0 / t1; written only with KEEP_T)
// and q = J T (2x2, its symmetric part; P = w q) of one row
template <bool KEEP_T>
__device__ __forceinline__ void row_projector(const RowGroup& g, const Row& o, double& ru, double& rv, double& wk, double* t0 /*[6]*/,
                                              double* t1 /*[6]*/, double& q00, double& q01, double& q11) {
    double u, v, cam[3], d, J[12];
    project(g.pc, o.x, o.y, o.z, u, v, cam, d);
    project_jacobian(g.pc, cam, d, J);
    ru = o.u - u; rv = o.v - v;
    wk = (o.wr * g.inv_wmax) * o.c;
    q00 = 0.0; q01 = 0.0; q11 = 0.0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        double s0 = 0.0, s1 = 0.0;
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            const double s = g.S[sym6(a, b)];
            s0 = fma(s, J[b], s0);
            s1 = fma(s, J[6 + b], s1);
        }
        q00 = fma(J[a], s0, q00);
        q01 = fma(J[a], s1, q01);
        q11 = fma(J[6 + a], s1, q11);
        if (KEEP_T) { t0[a] = s0; t1[a] = s1; }
    }
}

// A row of non-zero weight: leverage, w-test, and I - P = [m00, -p01; -p01, m11] with its determinant
__device__ __forceinline__ void row_lev_wtest(double wk, double q00, double q01, double q11, double ru, double rv, bool no_sigma,
                                              double& lv, double& ts, double& m00, double& m11, double& p01, double& det) {
#pragma clang fp contract(off)
    lv = fma(wk, q00, wk * q11);
    m00 = fma(-wk, q00, 1.0);
    m11 = fma(-wk, q11, 1.0);
    p01 = wk * q01;
    det = fma(m00, m11, -(p01 * p01));
    // r^T (I - P)^-1 r with (I - P)^-1 = [m11, p01; p01, m00] / det
    const double ruv = ru * rv;
    const double qf = fma(rv * rv, m00, fma(ruv + ruv, p01, (ru * ru) * m11)) / det;
    const double t2 = wk * qf;
    // (no_sigma, uniform over the window, is applied apart from the row's own conditions: in one condition with them the compiler
    // branches around the square root, which costs k_reliability 10 registers and with them a wave per SIMD)
    ts = (det > 0.0 && t2 >= 0.0 && t2 <= 1.79e308) ? sqrt(t2) : __builtin_nan("");
    if (no_sigma) ts = __builtin_nan("");
}

// The 16 partial results of a pose: a butterfly inside the DPP row, the same shape for every pose
__device__ __forceinline__ double group16_sum(double v) {
    v += shfl_xor_f64_c<1>(v); v += shfl_xor_f64_c<2>(v); v += shfl_xor_f64_c<4>(v); v += shfl_xor_f64_c<8>(v);
    return v;
}
__device__ __forceinline__ double group16_max(double v) {
    v = fmax(v, shfl_xor_f64_c<1>(v)); v = fmax(v, shfl_xor_f64_c<2>(v));
    v = fmax(v, shfl_xor_f64_c<4>(v)); v = fmax(v, shfl_xor_f64_c<8>(v));
    return v;
}

}  // namespace vba
