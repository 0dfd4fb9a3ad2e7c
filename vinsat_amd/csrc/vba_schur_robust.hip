// vba_schur_robust.hip -- the passes of the free-landmark fit's robust re-weighting (vba_schur_reweight; include/vinsat_ba.h carries
// the contract, the entry points and the handle live in vba_schur.hip) and the exact radix select behind it, which
// vba_schur_median runs on caller keys.  The reference's weights (BA_filtering.py:21-25): c = the lower median of the 2 m values
// |r|, q_k = mean over the two components of ((r / c)^2 / |alpha - 2| + 1)^(alpha / 2 - 1) / c^2, rho_k = q_k / max q, and
// row_w[k] = rho_k * base_k.
//
//   k_schur_robust_capture thread per row: base[k] = the weight the row was uploaded with (the saved one of a rejected row)
//   k_schur_robust_keys    thread per row: the reprojection of the cost kernel at the resident state, |ru|, |rv| as one 16-byte store
//   k_schur_select_small   up to kSelSmallMax keys: one workgroup runs the eight passes below back to back, histogram in LDS
//   k_schur_select_pass    pass p of the select on the bit patterns (non-negative doubles order as unsigned integers): the head
//                          turns the histogram of pass p - 1 into (prefix, rank) of this pass -- 256 bins, one scan, every workgroup
//                          for itself, workgroup 0 records it --, the body counts digit p of the keys that carry the prefix: two keys
//                          per 16-byte load, LDS histogram, one integer atomic per non-empty bin and workgroup.  Launch kSelPasses
//                          is the head alone and writes the key.
//   k_schur_robust_raw     grid-stride over the rows, at most kRobustMaxBlocks workgroups: q_k, the workgroup's largest
//   k_schur_robust_scale   every workgroup reduces the partial maxima in one fixed tree (one per thread), then rho_k * base_k into
//                          row_w, or into the saved weight of a row the snoop rejected; nothing is written unless c and max q are
//                          positive and finite
// Integer atomics only (histogram counts are exact in any order), a maximum for the one reduction: equal problems give equal bits.
#include <algorithm>

#include <hip/hip_runtime.h>

#include "vba_math.h"
#include "vba_schur_robust.h"

namespace vba {

namespace {

typedef unsigned long long u64;

static_assert(kSelThreads == kSelBins, "one thread per histogram bin");
static_assert(kRobustMaxBlocks <= 256, "the scaling pass reduces one partial maximum per thread");

__device__ __forceinline__ int sel_shift(int p) { return 64 - kSelDigitBits * (p + 1); }

// does key a carry the digits 0 .. p - 1 of prefix?
__device__ __forceinline__ bool sel_match(u64 a, int p, u64 prefix) { return p == 0 || ((a ^ prefix) >> (64 - kSelDigitBits * p)) == 0; }

// digit p of the keys [t0, t0 + kSelTile) that carry the prefix, counted into lh; thread t reads the pairs at t0 + j * 2 * kSelThreads + 2 t
__device__ __forceinline__ void sel_count_tile(const u64* keys, int64_t count, int64_t t0, int p, u64 prefix, unsigned* lh) {
    const int shift = sel_shift(p);
#pragma unroll
    for (int j = 0; j < kSelKeysPerThread / 2; ++j) {
        const int64_t i = t0 + (int64_t)j * (2 * kSelThreads) + 2 * (int64_t)threadIdx.x;       // even: a 16-byte boundary
        u64 a = 0, b = 0;
        const bool ha = i < count, hb = i + 1 < count;
        if (hb) {
            const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(keys + i);
            a = v.x; b = v.y;
        } else if (ha) {
            a = keys[i];
        }
        if (ha && sel_match(a, p, prefix)) atomicAdd(&lh[(a >> shift) & (kSelBins - 1)], 1u);
        if (hb && sel_match(b, p, prefix)) atomicAdd(&lh[(b >> shift) & (kSelBins - 1)], 1u);
    }
}

// (prefix, rank) of pass p + 1 from the counts of pass p (cnt = the count of bin threadIdx.x): the bin that holds the rank
__device__ __forceinline__ void sel_pick(u64 cnt, int p, u64& prefix, u64& rank, u64* sc, u64* pick) {
    const int t = threadIdx.x;
    sc[t] = cnt;
    if (t == 0) { pick[0] = prefix; pick[1] = 0; }
    __syncthreads();
    for (int o = 1; o < kSelBins; o <<= 1) {
        const u64 v = t >= o ? sc[t - o] : 0;
        __syncthreads();
        sc[t] += v;
        __syncthreads();
    }
    const u64 incl = sc[t], excl = incl - cnt;
    if (excl <= rank && rank < incl) {
        pick[0] = prefix | ((u64)t << sel_shift(p));
        pick[1] = rank - excl;
    }
    __syncthreads();
    prefix = pick[0];
    rank = pick[1];
    __syncthreads();
}

__global__ __launch_bounds__(kSelThreads) void k_schur_select_small(SchurSelectView W) {
    __shared__ unsigned lh[kSelBins];
    __shared__ u64 sc[kSelBins];
    __shared__ u64 pick[2];
    const int t = threadIdx.x;
    u64 prefix = 0, rank = (u64)((W.count - 1) / 2);
    for (int p = 0; p < kSelPasses; ++p) {
        lh[t] = 0;
        __syncthreads();
        for (int64_t t0 = 0; t0 < W.count; t0 += kSelTile) sel_count_tile(W.keys, W.count, t0, p, prefix, lh);
        __syncthreads();
        sel_pick((u64)lh[t], p, prefix, rank, sc, pick);
    }
    if (t == 0) W.out[0] = __longlong_as_double((long long)prefix);
}

__global__ __launch_bounds__(kSelThreads) void k_schur_select_pass(SchurSelectView W, int p) {
    __shared__ unsigned lh[kSelBins];
    __shared__ u64 sc[kSelBins];
    __shared__ u64 pick[2];
    const int t = threadIdx.x;
    u64 prefix = 0, rank = (u64)((W.count - 1) / 2);
    if (p > 0) {
        prefix = W.state[2 * (p - 1)];
        rank = W.state[2 * (p - 1) + 1];
        sel_pick(W.hist[(size_t)(p - 1) * kSelBins + t], p - 1, prefix, rank, sc, pick);
    }
    if (blockIdx.x == 0 && t == 0) {
        W.state[2 * p] = prefix;
        W.state[2 * p + 1] = rank;
        if (p == kSelPasses) W.out[0] = __longlong_as_double((long long)prefix);
    }
    if (p == kSelPasses) return;
    lh[t] = 0;
    __syncthreads();
    for (int64_t t0 = (int64_t)blockIdx.x * kSelTile; t0 < W.count; t0 += (int64_t)gridDim.x * kSelTile)
        sel_count_tile(W.keys, W.count, t0, p, prefix, lh);
    __syncthreads();
    if (lh[t] != 0) atomicAdd(&W.hist[(size_t)p * kSelBins + t], (u64)lh[t]);
}

__global__ __launch_bounds__(256) void k_schur_robust_capture(SchurRobustView V) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= V.m) return;
    V.base[k] = (V.row_mask && V.row_mask[k]) ? V.saved[k] : V.row_w[k];
}

__global__ __launch_bounds__(256) void k_schur_robust_keys(SchurRobustView V) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= V.m) return;
    const int i = V.row_pose[k], l = V.row_lm[k];
    PoseCam pc;
    pose_camera(V.states + (size_t)i * 10, V.intr + (size_t)i * 4, pc);
    double u, v, d, cam[3];
    project(pc, V.X[3 * (size_t)l], V.X[3 * (size_t)l + 1], V.X[3 * (size_t)l + 2], u, v, cam, d);
    double2 a;
    a.x = fabs(V.row_u[k] - u);
    a.y = fabs(V.row_v[k] - v);
    *reinterpret_cast<double2*>(V.keys + 2 * k) = a;
}

// the larger of two, a NaN if either is one (numpy's max)
__device__ __forceinline__ double nan_max(double a, double b) { return (a != a || b != b) ? __builtin_nan("") : (a > b ? a : b); }

// nan_max over the workgroup (256 threads), the same value in every thread
__device__ __forceinline__ double block_nan_max(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = nan_max(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return nan_max(nan_max(red[0], red[1]), nan_max(red[2], red[3]));
}

__global__ __launch_bounds__(256) void k_schur_robust_raw(SchurRobustView V, double alpha) {
    __shared__ double red[4];
    const double c = V.res[0], c2 = vba_mul(c, c);
    const double am2 = fabs(alpha - 2.0), e = alpha / 2.0 - 1.0;
    double mx = -__builtin_inf();
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < V.m; k += (int64_t)gridDim.x * 256) {
        double q;
        if (alpha == 2.0) {             // the reference's inf ** 0 == 1: no power
            q = 1.0 / c2;
        } else {
            const double2 a = *reinterpret_cast<const double2*>(V.keys + 2 * k);
            const double zu = a.x / c, zv = a.y / c;
            const double pu = pow(vba_add(vba_mul(zu, zu) / am2, 1.0), e) / c2;
            const double pv = pow(vba_add(vba_mul(zv, zv) / am2, 1.0), e) / c2;
            q = vba_mul(vba_add(pu, pv), 0.5);
        }
        V.q[k] = q;
        mx = nan_max(mx, q);
    }
    mx = block_nan_max(mx, red);
    if (threadIdx.x == 0) V.part[blockIdx.x] = mx;
}

__global__ __launch_bounds__(256) void k_schur_robust_scale(SchurRobustView V, double alpha, int nparts) {
    __shared__ double red[4];
    const double qmax = block_nan_max((int)threadIdx.x < nparts ? V.part[threadIdx.x] : -__builtin_inf(), red);
    if (blockIdx.x == 0 && threadIdx.x == 0) V.res[1] = qmax;
    const double c = V.res[0];
    const double inf = __builtin_inf();
    if (!(c > 0.0 && c < inf && qmax > 0.0 && qmax < inf)) return;      // status 1: weights and saved values untouched
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= V.m) return;
    const double rho = alpha == 2.0 ? 1.0 : V.q[k] / qmax;
    const double w = vba_mul(rho, V.base[k]);
    if (V.row_mask && V.row_mask[k]) V.saved[k] = w;
    else V.row_w[k] = w;
}

}  // namespace

void schur_select_launch(const SchurSelectView& W, hipStream_t s, int* launches) {
    (void)hipMemsetAsync(W.hist, 0, (size_t)kSelPasses * kSelBins * 8, s);
    int cnt = 0;
    if (W.count <= kSelSmallMax) {
        hipLaunchKernelGGL(k_schur_select_small, dim3(1), dim3(kSelThreads), 0, s, W);
        cnt = 1;
    } else {
        const unsigned grid = (unsigned)std::min<int64_t>(kSelMaxBlocks, (W.count + kSelTile - 1) / kSelTile);
        for (int p = 0; p < kSelPasses; ++p) hipLaunchKernelGGL(k_schur_select_pass, dim3(grid), dim3(kSelThreads), 0, s, W, p);
        hipLaunchKernelGGL(k_schur_select_pass, dim3(1), dim3(kSelThreads), 0, s, W, kSelPasses);
        cnt = kSelPasses + 1;
    }
    if (launches) *launches = cnt;
}

void schur_robust_capture_launch(const SchurRobustView& V, hipStream_t s) {
    hipLaunchKernelGGL(k_schur_robust_capture, dim3((unsigned)((V.m + 255) / 256)), dim3(256), 0, s, V);
}

int schur_robust_launch(const SchurRobustView& V, double alpha, hipStream_t s) {
    const unsigned rows = (unsigned)((V.m + 255) / 256);
    const int nparts = (int)std::min<unsigned>(rows, kRobustMaxBlocks);
    int sel = 0;
    hipLaunchKernelGGL(k_schur_robust_keys, dim3(rows), dim3(256), 0, s, V);
    schur_select_launch(V.sel, s, &sel);
    hipLaunchKernelGGL(k_schur_robust_raw, dim3(nparts), dim3(256), 0, s, V, alpha);
    hipLaunchKernelGGL(k_schur_robust_scale, dim3(rows), dim3(256), 0, s, V, alpha, nparts);
    return 3 + sel;
}

}  // namespace vba
