// vba_solve_chunks.hip -- the partitioned solve: chunk elimination kernels (level 1 and 2), the sequential walk of the reduced
// system, and the recovery of the interiors.  Device bodies: vba_solve_chunk_body.h; the reduced system by cyclic reduction:
// vba_solve_cr.hip.
#include "vba_solve_chunk_body.h"

namespace vba {

#ifdef VBA_RESIDENT_STAMPS
VBA_KSTAMP_FETCH(fetch_kstamps_chunks)
#endif

// level 1: chunks of the window's own chain
template <bool PIVOT>
__global__ __launch_bounds__(64) void k_solve_chunks(DevView V, int s) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int w = blockIdx.y, c = blockIdx.x;
    VBA_SKIP_CALL(V, w);
    WinScalars& sc = V.sc[w];
    if (sc.done || !solver_mine<PIVOT>(V, sc)) return;
    const int n = V.n[w];
    if (c * s >= n) return;
    const int lane = threadIdx.x;
    const size_t sb = (size_t)w * V.n_max;
    const size_t rb = (size_t)w * V.p_max;
    const double lam32 = (double)(float)sc.lam[V.par];
    if (c == 0 && lane == 0) {
        sc.lam32 = lam32;
        if (PIVOT) atomicAnd(&sc.fl[V.par], ~8u);
    }
    bool bad = false;
    const BandSource src{V.bands + sb * 243, V.rhs + sb * 9};
    chunk_eliminate<PIVOT, true>(src, n, s, c, lam32, V.csol + sb * 171, V.cL + rb * 171, V.cR + rb * 171, smem, lane, bad);
    report_pivot<PIVOT>(bad, sc, lane, V.par);
}

template <bool PIVOT>
__global__ __launch_bounds__(128) void k_solve_chunks_ts(DevView V, int s) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int w = blockIdx.y, c = blockIdx.x;
    VBA_SKIP_CALL(V, w);
    WinScalars& sc = V.sc[w];
    if (sc.done || !solver_mine<PIVOT>(V, sc)) return;
    const int n = V.n[w];
    if (c * s >= n) return;
    const int tid = threadIdx.x;
    const size_t sb = (size_t)w * V.n_max;
    const size_t rb = (size_t)w * V.p_max;
    const double lam32 = (double)(float)sc.lam[V.par];
    if (c == 0 && tid == 0) {
        sc.lam32 = lam32;
        if (PIVOT) atomicAnd(&sc.fl[V.par], ~8u);
    }
    bool bad = false;
    const BandSource src{V.bands + sb * 243, V.rhs + sb * 9};
    chunk_eliminate_twosided<PIVOT, true>(src, n, s, c, lam32, V.csol + sb * 171, V.cL + rb * 171, V.cR + rb * 171, smem, tid, bad);
    report_pivot<PIVOT>(bad, sc, tid & 63, V.par);
}

// Latency mode: the chunk's wave(s) build the blocks of the chunk themselves (no assembly launch, no round trip of the
// bands through memory).  The 256 threads of the block stage the per-pose inputs of the chunk and of its two
// neighbours in LDS and form the (at most s + 1) blocks  a - 1 .. b + 1  there; the first wave then eliminates the chunk
// exactly as k_solve_chunks does, reading blocks from LDS.  What the later kernels need from the system itself -- the
// diagonal block and right-hand side of the chunk's right separator (reduced system), the last pose's diagonal block
// (last_hessian) -- is written out on the way.
template <bool PIVOT, bool REG>
__global__ __launch_bounds__(256) void k_solve_chunks_fused(DevView V, int s) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int kAsmIn = kAsmBase + (REG ? kAsmPrior : 0);
    const int w = blockIdx.y, c = blockIdx.x;
    VBA_SKIP_CALL(V, w);
    WinScalars& sc = V.sc[w];
    if (sc.done || !solver_mine<PIVOT>(V, sc)) return;
    const int n = V.n[w];
    if (c * s >= n) return;
    const int tid = threadIdx.x;
    const size_t sb = (size_t)w * V.n_max;
    const size_t rb = (size_t)w * V.p_max;
    const double lam32 = (double)(float)sc.lam[V.par];
    if (c == 0 && tid == 0) {
        sc.lam32 = lam32;
        if (PIVOT) atomicAnd(&sc.fl[V.par], ~8u);
    }
    int a0, b0;
    bool has_sep;
    chunk_range(c, s, n, a0, b0, has_sep);
    const int j0 = a0 > 0 ? a0 - 1 : 0, j1 = has_sep ? b0 + 1 : b0;         // blocks formed here
    const int nblk = j1 - j0 + 1;
    double* elim = smem;                                                     // scratch of chunk_eliminate
    double* blocks = smem + (512 + (size_t)s * 252 + 162);                   // [s + 1][252]
    double* in = blocks + (size_t)(s + 1) * 252;                             // [s + 2][kAsmIn]: poses j0 - 1 .. j1
    asm_stage<REG>(V, w, n, true, j0 - 1, nblk + 1, in, tid, 256);
    __syncthreads();
    const double inv_wmax = 1.0 / bits_f64(sc.wmax_bits[V.par]);
    // thread t forms entry t of every block of the chunk: which band / row / column it is is decoded once (as in k_assemble)
    if (tid < 252) {
        const int e = tid;
        const bool is_rhs = e >= 243;
        const int which = e / 81, a = is_rhs ? e - 243 : (e % 81) / 9, b = e % 9;
        for (int q = 0; q < nblk; ++q) {
            const int i = j0 + q;
            const AsmRow R = asm_row<REG>(in + (size_t)(q + 1) * kAsmIn, in + (size_t)q * kAsmIn, i, n, true, V.prm.sigma, inv_wmax);
            double v;
            if (is_rhs) {
                v = rhs_entry(R, a);
                if (has_sep && i == j1) V.rhs[(sb + i) * 9 + a] = v;
            } else {
                v = band_entry(R, which, a, b);
                if (which == 1) {
                    if (has_sep && i == j1) V.bands[(sb + i) * 243 + e] = v;
                    if (i == n - 1) V.lastD[(size_t)w * 81 + (e - 81)] = v;
                }
            }
            blocks[(size_t)q * 252 + e] = v;
        }
    }
    __syncthreads();
    if (tid >= 64) return;      // the elimination is one wave's work (its barriers count the surviving wave only)
    bool bad = false;
    const LdsBlockSource src{blocks, j0};
    chunk_eliminate<PIVOT, true>(src, n, s, c, lam32, V.csol + sb * 171, V.cL + rb * 171, V.cR + rb * 171, elim, tid, bad);
    report_pivot<PIVOT>(bad, sc, tid, V.par);
}

template <bool PIVOT, bool REG>
__global__ __launch_bounds__(256) void k_solve_chunks_ts_fused(DevView V, int s) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    chunks_ts_fused_body<PIVOT, REG>(V, s, blockIdx.y, blockIdx.x, smem);
}

// level 2: the reduced system over the level-1 separators is itself cut into chunks of s2
template <bool PIVOT>
__global__ __launch_bounds__(64) void k_solve_chunks2(DevView V, int s, int s2) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int w = blockIdx.y, c = blockIdx.x;
    VBA_SKIP_CALL(V, w);
    WinScalars& sc = V.sc[w];
    if (sc.done || !solver_mine<PIVOT>(V, sc)) return;
    const int n1 = n_separators(V.n[w], s);
    if (n1 <= 0 || c * s2 >= n1) return;
    const int lane = threadIdx.x;
    const size_t sb = (size_t)w * V.n_max;
    const size_t rb = (size_t)w * V.p_max;
    const double lam32 = (double)(float)sc.lam[V.par];
    bool bad = false;
    const ReducedSource<BandSource> src{BandSource{V.bands + sb * 243, V.rhs + sb * 9}, V.cL + rb * 171, V.cR + rb * 171, s};
    chunk_eliminate<PIVOT, false>(src, n1, s2, c, lam32, V.csol2 + rb * 171, V.cL2 + rb * 171, V.cR2 + rb * 171, smem, lane, bad);
    report_pivot<PIVOT>(bad, sc, lane, V.par);
}

// Solves the last reduced block-tridiagonal system (one wave per window): over the level-1 separators (s2 == 0)
// or over the level-2 separators.
template <bool PIVOT>
__global__ __launch_bounds__(64) void k_solve_reduced(DevView V, int s, int s2) {
    __shared__ double blk[2][256];
    const int w = blockIdx.x;
    VBA_SKIP_CALL(V, w);
    WinScalars& sc = V.sc[w];
    if (sc.done || !solver_mine<PIVOT>(V, sc)) return;
    const int n1 = n_separators(V.n[w], s);
    if (n1 <= 0) return;
    const int lane = threadIdx.x;
    const size_t sb = (size_t)w * V.n_max;
    const size_t rb = (size_t)w * V.p_max;
    const double lam32 = (double)(float)sc.lam[V.par];
    const ReducedSource<BandSource> src1{BandSource{V.bands + sb * 243, V.rhs + sb * 9}, V.cL + rb * 171, V.cR + rb * 171, s};
    bool zero_pivot = false;
    if (s2 == 0) {
        chain_solve<PIVOT, false>(src1, n1, lam32, V.rXs + rb * 81, V.rzs + rb * 9, V.rx + rb * 9, blk, lane, zero_pivot);
    } else {
        const int n2 = n_separators(n1, s2);
        if (n2 > 0) {
            const ReducedSource<ReducedSource<BandSource>> src2{src1, V.cL2 + rb * 171, V.cR2 + rb * 171, s2};
            chain_solve<PIVOT, false>(src2, n2, lam32, V.rXs + rb * 81, V.rzs + rb * 9, V.rx2 + rb * 9, blk, lane, zero_pivot);
        }
    }
    report_pivot<PIVOT>(zero_pivot, sc, lane, V.par);
}

// Recovery of a partitioned chain: x_i = yhat_i - Vhat_i x_left - What_i x_right for interior blocks, separators
// copied from the reduced solution.
__device__ __forceinline__ void recover_block(int i, int n, int s, const double* csol, const double* xsep, double (&d9)[9]) {
    const int c = i / s;
    const int P = (n + s - 1) / s;
    const bool is_sep = (c < P - 1) && (i == (c + 1) * s - 1);
    if (is_sep) {
#pragma unroll
        for (int r = 0; r < 9; ++r) d9[r] = xsep[(size_t)c * 9 + r];
        return;
    }
    const double* so = csol + (size_t)i * 171;
    double xl[9], xr[9];
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        xl[r] = c > 0 ? xsep[(size_t)(c - 1) * 9 + r] : 0.0;
        xr[r] = c < P - 1 ? xsep[(size_t)c * 9 + r] : 0.0;
    }
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        double v = so[r];
#pragma unroll
        for (int k = 0; k < 9; ++k) v -= so[(1 + k) * 9 + r] * xl[k] + so[(10 + k) * 9 + r] * xr[k];
        d9[r] = v;
    }
}

// level 2 -> level 1: the solution of every level-1 separator
__global__ __launch_bounds__(64) void k_solve_recover2(DevView V, int s, int s2) {
    const int w = blockIdx.y;
    VBA_SKIP_CALL(V, w);
    WinScalars& sc = V.sc[w];
    if (sc.done) return;
    const int n1 = n_separators(V.n[w], s);
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= n1) return;
    const size_t rb = (size_t)w * V.p_max;
    double d9[9];
    recover_block(q, n1, s2, V.csol2 + rb * 171, V.rx2 + rb * 9, d9);
#pragma unroll
    for (int r = 0; r < 9; ++r) V.rx[(rb + q) * 9 + r] = d9[r];
}

// x_i for every block of the window (s == 0: dpose already holds the solution, block-diagonal phase), then the
// retraction (BA_filtering.py:56-60).
__global__ __launch_bounds__(256) void k_solve_recover(DevView V, int s) {
    // 16 lanes per pose, lane r < 9 forms row r of the step (for a fixed column of csol the nine lanes read nine
    // consecutive doubles); lane 0 of the group gathers the rows and retracts
    const int w = blockIdx.y;
    VBA_SKIP_CALL(V, w);
    WinScalars& sc = V.sc[w];
    if (sc.done) return;
    const int n = V.n[w];
    const int r = threadIdx.x & 15;
    const int i = blockIdx.x * 16 + (threadIdx.x >> 4);
    const size_t sb = (size_t)w * V.n_max;
    const size_t rb = (size_t)w * V.p_max;
    bool bad = false;
    double v = 0.0;
    if (i < n && r < 9) {
        if (s == 0) {
            v = V.dpose[(sb + i) * 9 + r];
        } else {
            const int c = i / s;
            const int P = (n + s - 1) / s;
            const double* xsep = V.rx + rb * 9;
            if ((c < P - 1) && (i == (c + 1) * s - 1)) {
                v = xsep[(size_t)c * 9 + r];            // a separator: copied from the reduced solution
            } else {
                const double* so = V.csol + (sb + i) * 171;
                v = so[r];
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    const double xl = c > 0 ? xsep[(size_t)(c - 1) * 9 + k] : 0.0;
                    const double xr = c < P - 1 ? xsep[(size_t)c * 9 + k] : 0.0;
                    v -= so[(1 + k) * 9 + r] * xl + so[(10 + k) * 9 + r] * xr;
                }
            }
            V.dpose[(sb + i) * 9 + r] = v;
        }
        bad = !(fabs(v) <= 1.79e308);
    }
    double d9[9];
    const int base = (threadIdx.x & 63) & ~15;
#pragma unroll
    for (int q = 0; q < 9; ++q) d9[q] = __shfl(v, base + q, kWave);
    if (i < n && r == 0) {
        double o[10];
        retract(V.states + (sb + i) * 10, d9, o);
#pragma unroll
        for (int q = 0; q < 10; ++q) V.states_new[(sb + i) * 10 + q] = o[q];
        if (V.host_states) {        // (one-window handles: sb == 0; a pipelined call reads its result from host memory)
#pragma unroll
            for (int q = 0; q < 10; ++q) V.host_states[((size_t)V.par * V.n_max + i) * 10 + q] = o[q];
        }
    }
    const unsigned long long anybad = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && anybad) atomicOr(&sc.fl[V.par], 2u);
}

// Dynamic LDS of the chunk kernels: chunk_lds_doubles (one wave), twosided_lds_doubles (two waves), and with the blocks and the
// staged inputs on top for the kernels that form their blocks.  The limits: chunks above ~30 poses exceed the default 64 KiB
// (up to 60 are allowed); the forming kernels up to kFusedChunkMax.
template <bool PIVOT>
static void launch_chunks_t(const DevView& V, bool forms, hipStream_t s) {
    const int cs = V.chunk, cs2 = V.chunk2;
    const int P = (V.n_max + cs - 1) / cs;
    const bool reg = V.reg != 0;
    const dim3 grid(P, V.W);
    if (forms && V.chunk_waves == 2 && cs >= 4) {
        const size_t lds = (size_t)twosided_fused_lds_doubles(cs, reg) * sizeof(double);
        if (reg) hipLaunchKernelGGL((k_solve_chunks_ts_fused<PIVOT, true>), grid, dim3(256), lds, s, V, cs);
        else hipLaunchKernelGGL((k_solve_chunks_ts_fused<PIVOT, false>), grid, dim3(256), lds, s, V, cs);
    } else if (forms) {
        const size_t lds = (size_t)chunk_fused_lds_doubles(cs, reg) * sizeof(double);
        if (reg) hipLaunchKernelGGL((k_solve_chunks_fused<PIVOT, true>), grid, dim3(256), lds, s, V, cs);
        else hipLaunchKernelGGL((k_solve_chunks_fused<PIVOT, false>), grid, dim3(256), lds, s, V, cs);
    } else if (V.chunk_waves == 2 && cs >= 4) {
        hipLaunchKernelGGL(k_solve_chunks_ts<PIVOT>, grid, dim3(128), (size_t)twosided_lds_doubles(cs) * sizeof(double), s, V, cs);
    } else {
        hipLaunchKernelGGL(k_solve_chunks<PIVOT>, grid, dim3(64), (size_t)chunk_lds_doubles(cs) * sizeof(double), s, V, cs);
    }
    if (cs2 > 0) {      // second level over the P-1 separators
        const int P2 = (P - 1 + cs2 - 1) / cs2;
        hipLaunchKernelGGL(k_solve_chunks2<PIVOT>, dim3(P2 > 0 ? P2 : 1, V.W), dim3(64), (size_t)chunk_lds_doubles(cs2) * sizeof(double), s, V, cs, cs2);
    }
    if (cs2 >= 0) hipLaunchKernelGGL(k_solve_reduced<PIVOT>, dim3(V.W), dim3(64), 0, s, V, cs, cs2);
}
void launch_solve_chunks(const DevView& V, bool pivot, bool forms, hipStream_t s) {
    if (pivot) launch_chunks_t<true>(V, forms, s);
    else launch_chunks_t<false>(V, forms, s);
}

void launch_solve_recover2(const DevView& V, hipStream_t s) {
    hipLaunchKernelGGL(k_solve_recover2, dim3((V.p_max + 63) / 64, V.W), dim3(64), 0, s, V, V.chunk, V.chunk2);
}
void launch_solve_recover(const DevView& V, int chunk, hipStream_t s) {
    hipLaunchKernelGGL(k_solve_recover, dim3((V.n_max + 15) / 16, V.W), dim3(256), 0, s, V, chunk);
}

hipError_t configure_chunks_device() {
    const int cap = chunk_lds_doubles(60) * 8, cap_ts = twosided_lds_doubles(60) * 8;
    const int cap_f = chunk_fused_lds_doubles(kFusedChunkMax, true) * 8, cap_tsf = twosided_fused_lds_doubles(kFusedChunkMax, true) * 8;
    const LdsLimit set[] = {
        {reinterpret_cast<const void*>(k_solve_chunks_fused<false, false>), cap_f}, {reinterpret_cast<const void*>(k_solve_chunks_fused<true, false>), cap_f},
        {reinterpret_cast<const void*>(k_solve_chunks_fused<false, true>), cap_f}, {reinterpret_cast<const void*>(k_solve_chunks_fused<true, true>), cap_f},
        {reinterpret_cast<const void*>(k_solve_chunks_ts_fused<false, false>), cap_tsf}, {reinterpret_cast<const void*>(k_solve_chunks_ts_fused<true, false>), cap_tsf},
        {reinterpret_cast<const void*>(k_solve_chunks_ts_fused<false, true>), cap_tsf}, {reinterpret_cast<const void*>(k_solve_chunks_ts_fused<true, true>), cap_tsf},
        {reinterpret_cast<const void*>(k_solve_chunks<false>), cap}, {reinterpret_cast<const void*>(k_solve_chunks<true>), cap},
        {reinterpret_cast<const void*>(k_solve_chunks_ts<false>), cap_ts}, {reinterpret_cast<const void*>(k_solve_chunks_ts<true>), cap_ts},
        {reinterpret_cast<const void*>(k_solve_chunks2<false>), cap}, {reinterpret_cast<const void*>(k_solve_chunks2<true>), cap}};
    return set_lds_limits(set);
}

}  // namespace vba
