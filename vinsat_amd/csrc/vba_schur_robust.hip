// vba_schur_robust.hip -- the free-landmark fit's robust re-weighting (vba_schur_reweight, vba_schur_get_weights; include/vinsat_ba.h
// carries the contract, vba_schur_context.h the handle, vba_schur.hip the map of the units) and the exact radix select behind it, which
// vba_schur_median runs on caller keys: the passes, then the entry points.  The reference's weights (BA_filtering.py:21-25):
// c = the lower median of the 2 m values |r|, q_k = mean over the two components of ((r / c)^2 / |alpha - 2| + 1)^(alpha / 2 - 1) / c^2,
// rho_k = q_k / max q, and row_w[k] = rho_k * base_k.
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
#include <mutex>

#include <hip/hip_runtime.h>

#include "vba_math.h"
#include "vba_schur_context.h"
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

namespace {

// one grow-only workspace per process for vba_schur_median (keys, the select's scratch, the result)
struct MedianWorkspace {
    std::mutex m;
    int device = -1;
    char* base = nullptr;
    size_t size = 0;
    hipStream_t stream = nullptr;
} g_median_ws;

}  // namespace

// first re-weighting of a handle: its state and its two timing events
static int schur_robust_alloc(vba_schur_handle h) {
    SchurRobust& Z = h->robust;
    if (Z.sc.arena) return VBA_OK;
    const size_t m = (size_t)h->V.m;
    SchurLayout lay;
    const size_t o_b = lay.need(m * 8), o_k = lay.need(m * 16), o_q = lay.need(m * 8), o_p = lay.need((size_t)kRobustMaxBlocks * 8), o_r = lay.need(16),
                 o_s = lay.need(schur_select_scratch_bytes());
    if (int rc = schur_scratch_alloc(Z.sc, lay.bytes, "re-weighting state")) return rc;
    char* A = Z.sc.arena;
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
    W.saved = h->snoop.sc.arena ? h->snoop.saved : nullptr;
    W.row_mask = h->snoop.sc.arena ? h->snoop.row_mask : nullptr;
    W.base = Z.base; W.keys = Z.keys; W.q = Z.q; W.part = Z.part; W.res = Z.res;
    W.sel.keys = reinterpret_cast<const unsigned long long*>(Z.keys); W.sel.count = 2 * V.m;
    W.sel.hist = Z.hist; W.sel.state = Z.state; W.sel.out = Z.res;
    return W;
}

extern "C" {

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
    SCHK(hipEventRecord(Z.sc.ev[0], s));
    Z.launches = schur_robust_launch(W, alpha, s);
    double res[2] = {0.0, 0.0};
    const int rc = schur_scratch_finish(Z.sc, s, [&]() -> int {
        SCHK(hipGetLastError());
        SCHK(hipMemcpyAsync(res, Z.res, 16, hipMemcpyDeviceToHost, s));
        return VBA_OK;
    });
    if (rc) return rc;
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
    if (h->robust.sc.arena && h->robust.captured) {
        SCHK(hipMemcpy(base, h->robust.base, m * 8, hipMemcpyDeviceToHost));
        return VBA_OK;
    }
    SCHK(hipMemcpy(base, h->V.row_w, m * 8, hipMemcpyDeviceToHost));
    if (h->snoop.sc.arena) {        // never re-weighted: the weights in place, a rejected row by its saved value
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
    *ms = h->robust.sc.ms;
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

}  // extern "C"
