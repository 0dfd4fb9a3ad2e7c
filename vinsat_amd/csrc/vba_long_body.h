// vba_long_body.h -- the device bodies of the parallel-in-time propagation of a long gap, shared by the kernels of the
// fixed-landmark path (vba_long.hip, which carries the account of the method) and those of the free-landmark mode
// (vba_schur_dyn_long.hip): the coarse propagator, the parareal iteration of one wavefront (long_states), the layout of a slot of
// the chain pool, the tangent pass over the sub-chunks of one workgroup and the fixed pairwise ordered-product tree.  Device code
// only; the cutting rule (long_plan) and the size of a slot (long_pool_states) are host/device functions of vba_math.h.  Internal.
#pragma once

#include "vba_device.h"

namespace vba {

// the coarse propagator: one RK4 step of length h (hh = h / 2, h6 = h / 6 precomputed: an IEEE division per step would sit on
// the critical path of the sweep)
__device__ __forceinline__ void rk4_coarse(const double* x, double h, double hh, double h6, double* o) {
    double k1[3], k2[3], k3[3], k4[3], p[3], v2[3], v3[3], v4[3];
    accel_jvp(x, nullptr, k1, nullptr, false);
#pragma unroll
    for (int i = 0; i < 3; ++i) { p[i] = x[i] + hh * x[3 + i]; v2[i] = x[3 + i] + hh * k1[i]; }
    accel_jvp(p, nullptr, k2, nullptr, false);
#pragma unroll
    for (int i = 0; i < 3; ++i) { p[i] = x[i] + hh * v2[i]; v3[i] = x[3 + i] + hh * k2[i]; }
    accel_jvp(p, nullptr, k3, nullptr, false);
#pragma unroll
    for (int i = 0; i < 3; ++i) { p[i] = x[i] + h * v3[i]; v4[i] = x[3 + i] + h * k3[i]; }
    accel_jvp(p, nullptr, k4, nullptr, false);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        o[i] = x[i] + h6 * (x[3 + i] + 2 * v2[i] + 2 * v3[i] + v4[i]);
        o[3 + i] = x[3 + i] + h6 * (k1[i] + 2 * k2[i] + 2 * k3[i] + k4[i]);
    }
}

// The chain is converged when every chunk's fine end state and the next chunk's start state agree to kLongTight, relative (the
// defects of up to 64 chunks add up along the gap: 2^-48 each keeps the end state within ~1e-13) -- or, a few units of rounding above
// that, when another sweep no longer reduces the defect (a chunk of ~50 fine steps carries ~1e-15 of rounding of its own).
constexpr double kLongTight = 0x1p-48, kLongLoose = 0x1p-45;

// One wavefront.  x0: the state at the start of the gap (the same in every lane), s: its steps.  Lane j < P ends up with the
// converged chunk-start state U_j in `U`; xh (every lane) = the state at the end of the gap, the last chunk's fine end state
// F_{P-1}(U_{P-1}).  Everything lives in registers: a lane keeps what concerns its chunk (its start state U, its end state N = the
// next chunk's start).
// The correction sweep is LINEARISED: with A_j the Jacobian of the coarse step at U_j (every lane forms its own, six tangents
// through one RK4 step) the parareal update G_j(U_j') - G_j(U_j) becomes A_j c_j and the sweep the affine recurrence
//     c_0 = 0,  c_{j+1} = (F_j(U_j) - U_{j+1}) + A_j c_j,   U_j' = U_j + c_j
// -- a matrix-vector product and six v_readlane per chunk instead of a nonlinear RK4 step (66 instead of 250 instructions on the
// serial path).  What the linearisation drops is second order in c (~1e-8 relative after the coarse chain: 1e-16), and the first
// k chunks are still the serial chain bit for bit after k sweeps (c_1 = F_0 - U_1 exactly, and so on).
// The iteration ends when the DEFECT of the chain is below tolerance: every chunk's fine propagation from its start state
// lands on the next chunk's start state, i.e. the U_j are the serial chain up to that tolerance -- checked right behind the
// fine pass, so a converged iterate costs no sweep of its own (one sweep, two fine passes for gaps up to ~1000 s).  Whatever the
// sweep does, that check is what the result answers to.
// subs: receives the states at the sub-chunk starts of the LAST fine pass -- subs[g * 6 .. ], g in chain order.
__device__ __forceinline__ void long_states(const double* x0, int s, const LongPlan pl, int lane, double* U /*[6]*/, double* xh /*[6]*/,
                                            double* subs) {
    const int P = pl.P;
    const int last_len = s - (P - 1) * pl.L;
    const int my_len = lane < P - 1 ? pl.L : (lane == P - 1 ? last_len : 0);
    const double hL = (double)pl.L, hhL = 0.5 * hL, h6L = hL / 6.0;
    const double hT = (double)last_len, hhT = 0.5 * hT, h6T = hT / 6.0;
    double F[6], N[6], u[6];
    double worst_prev = 1.0;
#pragma unroll
    for (int c = 0; c < 6; ++c) { u[c] = x0[c]; U[c] = x0[c]; N[c] = x0[c]; }
    // the coarse chain (serial, the same in every lane)
    for (int j = 0; j < P; ++j) {
        const bool tail = j == P - 1;
        double g[6];
        rk4_coarse(u, tail ? hT : hL, tail ? hhT : hhL, tail ? h6T : h6L, g);
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            if (lane == j) N[c] = g[c];
            if (lane == j + 1) U[c] = g[c];
            u[c] = g[c];
        }
    }
    for (int it = 0; it <= P; ++it) {
        // fine: every chunk from its current start state, in parallel
#pragma unroll
        for (int c = 0; c < 6; ++c) F[c] = U[c];
        {
            double* rec = it > 0 ? subs + (size_t)lane * pl.nsubL * 6 : nullptr;    // (the pass behind the coarse chain is never the last)
            int until = 0;
            for (int q = 0; q < my_len; ++q) {
                if (rec && q == until) {
#pragma unroll
                    for (int c = 0; c < 6; ++c) rec[c] = F[c];
                    rec += 6;
                    until += pl.sub;
                }
                rk4_step<false>(F, nullptr, 1.0);
            }
        }
        if (it > 0) {       // (the coarse chain alone is never close enough)
            const double np = fmax(fmax(fabs(N[0]), fabs(N[1])), fabs(N[2])), nv = fmax(fmax(fabs(N[3]), fabs(N[4])), fabs(N[5]));
            const double dp = fmax(fmax(fabs(F[0] - N[0]), fabs(F[1] - N[1])), fabs(F[2] - N[2]));
            const double dv = fmax(fmax(fabs(F[3] - N[3]), fabs(F[4] - N[4])), fabs(F[5] - N[5]));
            const double rel = lane < P ? fmax(dp / np, dv / nv) : 0.0;
            if (__any(rel != rel)) break;               // non-finite states: nothing to converge to (the residual carries the NaN on)
            const double worst = wave_max(rel);
            if (worst <= kLongTight || (it >= 2 && worst <= kLongLoose && worst > 0.25 * worst_prev)) break;
            worst_prev = worst;
        }
        // the Jacobian of this lane's coarse step at its start state: A[r][k] = T[k][r] (two passes of three tangents: the registers)
        double T[6][6];
        {
            const double h = lane == P - 1 ? hT : hL;
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                double xs[6], t3[3][6];
#pragma unroll
                for (int c = 0; c < 6; ++c) xs[c] = U[c];
#pragma unroll
                for (int k = 0; k < 3; ++k)
#pragma unroll
                    for (int c = 0; c < 6; ++c) t3[k][c] = (c == 3 * half + k) ? 1.0 : 0.0;
                rk4_step_multi<3>(xs, t3, h);
#pragma unroll
                for (int k = 0; k < 3; ++k)
#pragma unroll
                    for (int c = 0; c < 6; ++c) T[3 * half + k][c] = t3[k][c];
            }
        }
        double d[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) d[c] = F[c] - N[c];
        // sweep: c_{j+1} = d_j + A_j c_j; every lane evaluates it with its own A and d, lane j's value is the one that counts
        double cc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int j = 0; j < P; ++j) {
            double cn[6];
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                double a = d[r];
#pragma unroll
                for (int k = 0; k < 6; ++k) a = fma(T[k][r], cc[k], a);
                cn[r] = readlane_f64(a, j);
            }
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                if (lane == j) N[c] += cn[c];
                if (lane == j + 1) U[c] += cn[c];
                cc[c] = cn[c];
            }
        }
    }
    // the end of the gap is where the last chunk's FINE pass landed (F of lane P - 1), not the corrected coarse state N: the loose
    // stop rule leaves the two up to 2^-45 apart
#pragma unroll
    for (int c = 0; c < 6; ++c) xh[c] = readlane_f64(F[c], P - 1);
}

// A slot of the pool, in states of six doubles: [0] x_hat, [1] the start state the chain belongs to, [2] spare, [3, 3 + G) the
// sub-chunk start states, then kLongSplit partial products of the transition matrix (36 doubles each).
constexpr int kLongHead = 3;
constexpr int kLongSplit = 8;           // workgroups that share the tangent pass of one edge (16 sub-chunks each)
constexpr int kLongSubs = 16;           // sub-chunks of one such workgroup
static_assert(kLongHead == 3 && kLongSplit * 36 == 48 * 6, "long_pool_states (vba_math.h) sizes the slot the upload reserves");

// The tangent pass of ONE of the kLongSplit workgroups of 128 of an edge of s steps: sub-chunks g0 .. g0 + 15 of the chain in the
// slot `chain`, 8 lanes each, six at work with one tangent column each (as dynamics_block), ~10 steps from the sub-chunk's start
// state; M[g - g0] receives the transition matrix of sub-chunk g, row major.  The caller synchronises behind it.
__device__ __forceinline__ void long_tangent_subchunks(const double* chain, int s, const LongPlan& pl, int g0, int tid, double (*M)[36]) {
    const int g = g0 + (tid >> 3), c = tid & 7;
    if (g < pl.G && c < 6) {
        const int j = g / pl.nsubL < pl.P - 1 ? g / pl.nsubL : pl.P - 1;      // the chunk of this sub-chunk (the tail chunk may hold fewer)
        const int q = g - j * pl.nsubL;
        const int clen = j < pl.P - 1 ? pl.L : s - (pl.P - 1) * pl.L;
        const int len = clen - q * pl.sub < pl.sub ? clen - q * pl.sub : pl.sub;
        const double* sg = chain + (size_t)(kLongHead + g) * 6;
        double x[6], t[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int r = 0; r < 6; ++r) x[r] = sg[r];
        t[c] = 1.0;
        for (int e = 0; e < len; ++e) rk4_step<true>(x, t, 1.0);
#pragma unroll
        for (int r = 0; r < 6; ++r) M[tid >> 3][6 * r + c] = t[r];
    }
}

// The ordered product M[cnt - 1] ... M[1] M[0] of cnt 6x6 matrices in LDS by a workgroup of NT threads, in place, pairwise in a fixed
// tree: at stride d the matrix at 2 a d takes M[2 a d + d] * M[2 a d] (a matrix without a partner stays); the product ends up in
// M[0].  The caller has synchronised in front of it; it leaves the workgroup synchronised.
template <int NT>
__device__ __forceinline__ void long_ordered_product(double (*M)[36], int cnt, int tid) {
    for (int d = 1; d < cnt; d <<= 1) {
        const int pairs = (cnt + 2 * d - 1) / (2 * d);
        double v[3];
        int n = 0;
        for (int e = tid; e < pairs * 36; e += NT, ++n) {
            const int a = e / 36, rc = e % 36, r = rc / 6, c = rc % 6;
            const int lo = 2 * a * d, hi = lo + d;
            if (hi < cnt) {
                double acc = M[hi][6 * r] * M[lo][c];
#pragma unroll
                for (int q = 1; q < 6; ++q) acc = fma(M[hi][6 * r + q], M[lo][6 * q + c], acc);
                v[n] = acc;
            } else {
                v[n] = M[lo][rc];
            }
        }
        __syncthreads();
        n = 0;
        for (int e = tid; e < pairs * 36; e += NT, ++n) M[2 * (e / 36) * d][e % 36] = v[n];
        __syncthreads();
    }
}

}  // namespace vba
