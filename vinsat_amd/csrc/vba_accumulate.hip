// vba_accumulate.hip -- A2 + A3a + A3b of the BA iteration (gfx950).
//
//   k_obs_accumulate<G> Jacobian, robust weight, per-pose 6x6 / 6 accumulation (G lanes per pose).  Latency mode: starts the
//                      call -- inline select on the bin buckets of the trial in front, and one extra block that takes the
//                      accept test of the call in front (vba_select_body.h, vba_decide.h); few windows: the dynamics factor
//                      rides in its grid (vba_dyn_body.h)
//
// It streams the observation arrays once, coalesced (SoA, 8 B per lane per array); the pose state is gathered through
// L1/L2 (observations are pose sorted, so a wave touches one or two poses).
#include <cstdlib>
#include "vba_dyn_body.h"
#include "vba_launch.h"
#include "vba_select_body.h"

// Build-time knobs of this unit:
#ifndef VBA_ACC_DEPTH
#define VBA_ACC_DEPTH 2         // observations in flight per lane (not PAIR)
#endif
#ifndef VBA_ACC_PAIR
#define VBA_ACC_PAIR 1          // G = 4, 8: two consecutive observations per step (PAIR below)
#endif
#ifndef VBA_ACC_PAIR_DEPTH
#define VBA_ACC_PAIR_DEPTH 1    // 2: two pairs in flight per lane (BATCH, PAIR; 24 more VGPRs)
#endif
#ifndef VBA_ACC_GROUPS
#define VBA_ACC_GROUPS 4        // BATCH: groups of poses a block walks (launch_obs_accumulate; run time: VBA_X_ACCGROUPS)
#endif

namespace vba {

constexpr int kAccDepth = VBA_ACC_DEPTH;
constexpr bool kPair = VBA_ACC_PAIR != 0;
// VBA_X_ACCGROUPS (sweeps): overrides the number of groups; read at the first batched launch
static int acc_groups_env() {
    static const int v = std::getenv("VBA_X_ACCGROUPS") ? std::atoi(std::getenv("VBA_X_ACCGROUPS")) : 0;
    return v;
}

// Diagnostic builds (-DVBA_RESIDENT_STAMPS; tools/attic/trial_stamps.py): 100 MHz wall-clock stamps of thread 0 of block 60
// along k_obs_accumulate; words 16 .. 63 of what vba_debug_fetch(h, 0, 102, ...) returns (fetch_ostamps, vba_trial.hip).
#ifdef VBA_RESIDENT_STAMPS
__device__ unsigned long long g_astamps[48];
#define VBA_ASTAMP(slot) do { if (threadIdx.x == 0 && blockIdx.x == 60 && blockIdx.y == 0) g_astamps[slot] = wall_clock64(); } while (0)
void fetch_astamps(unsigned long long* out) { (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_astamps), sizeof(g_astamps)); }
#else
#define VBA_ASTAMP(slot) do {} while (0)
#endif

// The steps of the recursive-halving reduction of k_obs_accumulate (see there), unrolled over a compile-time mask so that the
// first two exchanges (24 of the 31 values that travel) are quad permutations instead of LDS-crossbar shuffles.
template <int G, int CNT, int MASK>
__device__ __forceinline__ void halving_steps(double (&acc)[32], int sub, int& own) {
    if constexpr (MASK < G && CNT > 1) {
        const bool up = (sub & MASK) != 0;
        constexpr int half = CNT >> 1;
#pragma unroll
        for (int j = 0; j < half; ++j) {
            const double lo = acc[j], hi = acc[half + j];
            acc[j] = (up ? hi : lo) + shfl_xor_f64_c<MASK>(up ? lo : hi);
        }
        if (up) own += half;
        halving_steps<G, (CNT >> 1), (MASK << 1)>(acc, sub, own);
    }
}

// ---------------------------------------------------------------------------------------------- A2 + A3
// G lanes per pose (power of two): every lane strides over its share of the pose's observation segment and
// keeps the 21 + 6 unique entries of sum(w J^T J), sum(w J^T r) in registers; a log2(G)-step xor butterfly
// then gives the lanes of the group the totals.  The shape of the reduction is fixed, so results are bit
// reproducible (no float atomics).  The raw (un-normalised) weight is stored per observation for the trials.
// PAIR: a lane takes two consecutive observations per step with 16-byte loads, so that the G lanes of a pose read
// whole 128-byte lines (G = 8) instead of half lines whose other half is fetched again by the next step.
// BATCH: the variant of handles with many windows -- the median is in sc.c_obs already (k_select_finish), nothing rides in
// the grid and nothing is selected inline, so none of that code (nor its registers: the rider alone needs ~195) is compiled in.
// F32 (VBA_OPT_JACOBIAN_F32): the camera-frame Jacobian terms in fp32 (cam_jacobian_f32), their products and sums in fp64;
// every G takes the camera-frame form then (include/vinsat_ba.h: the precision contract).
template <int G, bool PAIR, bool BATCH, bool F32 = false>
__global__ __launch_bounds__(256) void k_obs_accumulate(DevView V) {
    __shared__ double wmx[4];
    __shared__ unsigned sel_lh[BATCH ? 1 : kSelBins];
    __shared__ unsigned sel_u[BATCH ? 1 : 260];
    __shared__ unsigned long long sel_keys[BATCH ? 1 : 1025];
    __shared__ double dec_red[BATCH ? 1 : 5][4];
    constexpr int PPB = 256 / G;            // poses per block
    const int w = blockIdx.y;
    WinScalars& sc = V.sc[w];
    if (BATCH) { V.sel_inline = 0; V.dyn_in_acc = 0; V.median_ready = 1; }
    // The row range of this thread's pose, requested FIRST of all (its address needs the block and thread index only; the
    // index is clamped into the window's n_max + 1 entries): the range is a dependent round trip in front of the first
    // observation loads, and this way it runs beside the call snapshot's instead of behind it.
    int early_beg = 0, early_end = 0;
    if (!BATCH) {
        const int ie = min((int)(blockIdx.x * PPB + threadIdx.x / G), V.n_max - 1);
        const int* ptr0 = V.pose_ptr + 2 * (size_t)w * V.obs_stride;
        early_beg = ptr0[ie];
        early_end = ptr0[ie + 1];
    }
    // Inline select (V.sel_inline: latency mode, carried keys in bin buckets): this kernel STARTS the call -- no select
    // kernel in front of it.  In a chained schedule the accept test of the call in front is evaluated here too, beside the
    // accumulation (the in-order form, accept test first, is k_select_warm).
    // One relaxed atomic read of the two words, once per block.  The extra block of THIS grid (below) commits the call in front
    // and writes call_idx = V.call while other blocks may not have started yet -- an intra-grid race that is benign because
    // both outcomes let a block proceed: a block that still sees (pending, call_idx) = (call - 1, call - 1) takes fold_here,
    // one that already sees call_idx = V.call passes the ordinary "window is at this call" test; no other value can be seen
    // (the commit block is the only writer during this kernel, and it writes only after a clean accept).
    const int seen_call = __atomic_load_n(&sc.call_idx, __ATOMIC_RELAXED);
    const int seen_pending = __atomic_load_n(&sc.pending, __ATOMIC_RELAXED);
    const bool fold_here = V.sel_inline && V.call >= 0 && V.fold && seen_pending == V.call - 1 && seen_call == V.call - 1;
    if (!fold_here && !((V.call < 0 || seen_call == V.call) && (V.redo == 2 || (sc.miss != 0) == (V.redo != 0)))) return;     // VBA_SKIP_CALL on the snapshot
    // The accept test only GATES: nothing this kernel computes depends on it, and a trial that turns out not to be clean just
    // leaves no trace -- what this kernel writes on the way (weights, per-pose sums, the pose-chain factor of its rider
    // blocks) lives per call parity, the later trials of the call in front still find theirs.
    const int nb_acc = (V.n_max * G + 255) / 256;
    // ... and it is evaluated by ONE extra block of the grid (the last one), which also leaves what the start of this call
    // leaves in the scalars: off the critical path of the blocks that accumulate.  Those need no gate at all: their
    // maximum goes into a slot that the trial kernel of the call in front clears whenever it runs again.
    if (V.sel_inline && blockIdx.x == gridDim.x - 1) {
        unsigned hl[8];
        select_load(hist0_of(V, w, V.par), kSelBins, hl);
        DecideIn fin = {};
        if (fold_here) fin = fold_load(V, w);
        unsigned bin, in_bin;
        long long rank;
        const bool hit = front_resolve(V, w, hl, V.bucket_cap, sel_u, bin, rank, in_bin);
        double c = 0.0;
        if (hit) {
            const double* bucket = V.wbucket + (((size_t)w * 2 + V.par) * kSelBins + bin) * (size_t)V.bucket_cap;
            c = select_finish_list(V, w, bucket, V.bucket_cap, in_bin, rank, 1, sc.warm_lo[V.par] + ((unsigned long long)(bin - 1u) << V.warm_shift),
                                   false, sel_lh, sel_u, sel_keys);
        }
        DecideOut d;
        if (fold_here && !fold_decide_loaded(V, w, fin, dec_red, d)) return;    // not clean: no trace (the window stalls at the call in front)
        if (fold_here) fold_commit(V, w, d);
        if (threadIdx.x == 0) {
            front_commit(V, w, hit, bin, rank, in_bin, true);
            if (hit) sc.c_obs = c;
        }
        return;
    }
    if (!BATCH && (int)blockIdx.x >= nb_acc) {        // few windows: the dynamics factor rides in this grid (vba_dyn_body.h)
        // (a function of the input states only: neither a missed select nor the accept test concerns it -- what it writes
        // is read by this call's own assembly, which runs only if the window has moved on)
        dynamics_block(V, w, blockIdx.x - nb_acc);
        return;
    }
    const int n = V.n[w];
    if (blockIdx.x * PPB >= n) return;
    VBA_ASTAMP(0);
    const StepParams& prm = V.prm;
    const int sub = threadIdx.x % G;
    const size_t ob = (size_t)w * V.obs_stride;
    const size_t mb = (size_t)w * V.m_max;
    double wmax_l = 0.0;
    // BATCH: a block walks several groups of PPB poses (grid = a quarter of the groups) and requests the row range of its
    // NEXT group while it works on the current one -- the range is a dependent round trip in front of the first
    // observation loads, and at two waves per SIMD nobody covers it.  Otherwise: one group per block, one pass.
    const int gstride = BATCH ? (int)gridDim.x : 0;
    int pf_beg = 0, pf_end = 0;
    if (BATCH) {
        const int i0 = blockIdx.x * PPB + threadIdx.x / G;
        if (i0 < n) {
            const int* ptr0 = V.pose_ptr + 2 * ob;
            pf_beg = ptr0[i0];
            pf_end = ptr0[i0 + 1];
        }
    }
    for (int grp = blockIdx.x; grp * PPB < n; grp += gstride) {
    const int i = grp * PPB + threadIdx.x / G;
    const size_t pb = (size_t)w * V.n_max + (i < n ? i : 0);

    struct Obs { double x, y, z, u, v, c; };
    struct alignas(8) D2 { double a, b; };
    struct Obs2 { D2 x, y, z, u, v, c; };
    auto load = [&](int k) {
        Obs o;
        o.x = V.ox[ob + k]; o.y = V.oy[ob + k]; o.z = V.oz[ob + k];
        o.u = V.ou[ob + k]; o.v = V.ov[ob + k]; o.c = V.oconf[ob + k];
        return o;
    };
    auto load2 = [&](int k) {       // observations k, k + 1 (the second may belong to the next pose: masked below)
        Obs2 o;
        o.x = *reinterpret_cast<const D2*>(V.ox + ob + k); o.y = *reinterpret_cast<const D2*>(V.oy + ob + k);
        o.z = *reinterpret_cast<const D2*>(V.oz + ob + k); o.u = *reinterpret_cast<const D2*>(V.ou + ob + k);
        o.v = *reinterpret_cast<const D2*>(V.ov + ob + k); o.c = *reinterpret_cast<const D2*>(V.oconf + ob + k);
        return o;
    };

    // Phase 1: everything that does not need the median is started first (the pose's camera, its row range and the
    // first observations), so that those round trips overlap with the select finish below.
    // Software pipelined: the loads of the next observations are in flight while the current ones are processed (the
    // kernel sits at 2 waves per SIMD because of its accumulators either way; the registers between that and the next
    // occupancy step are spent on memory-level parallelism).
    // (inline select: the histogram is requested first of all -- it depends on nothing, the row range below is a dependent
    // round trip)
    unsigned hloc[8] = {};
    if (V.sel_inline) select_load(hist0_of(V, w, V.par), kSelBins, hloc);
    PoseCam pc{};
    int beg = 0, end = 0;
    Obs ring[kAccDepth]{};
    Obs2 nxt{}, nxt2{};
    constexpr bool kPairDepth2 = BATCH && PAIR && VBA_ACC_PAIR_DEPTH == 2;     // two pairs in flight per lane (24 more VGPRs)
    if (i < n) {
        pose_camera(V.states + pb * 10, V.intr + pb * 4, pc);
        if (BATCH) {
            beg = pf_beg;
            end = pf_end;
        } else {
            beg = early_beg;
            end = early_end;
        }
        if (PAIR) {
            if (beg + 2 * sub < end) nxt = load2(beg + 2 * sub);
            if (kPairDepth2 && beg + 2 * sub + 2 * G < end) nxt2 = load2(beg + 2 * sub + 2 * G);
        } else {
#pragma unroll
            for (int d = 0; d < kAccDepth; ++d)
                if (beg + sub + d * G < end) ring[d] = load(beg + sub + d * G);
        }
    }
    if (BATCH) {        // the row range of this thread's pose in the block's next group
        const int in = i + gstride * PPB;
        pf_beg = pf_end = 0;
        if (in < n) {
            const int* ptr = V.pose_ptr + 2 * ob;
            pf_beg = ptr[in];
            pf_end = ptr[in + 1];
        }
    }

    // Phase 2: the median (every block of the window finishes the select itself, see select_finish)
    VBA_ASTAMP(1);
    RobustParams rp;
    if (BATCH) {
        rp.c = sc.c_obs;        // k_select_finish
    } else if (V.sel_inline) {
        // the trial kernel of the call in front dropped every key into the bucket of its warm bin: resolve the histogram,
        // rank the wanted bin's bucket.  Every block does this redundantly (a few hundred keys), nothing is compacted.
        unsigned bin, in_bin;
        long long rank;
        if (!front_resolve(V, w, hloc, V.bucket_cap, sel_u, bin, rank, in_bin)) return;    // a miss (the last block records it)
        const unsigned long long lo = sc.warm_lo[V.par];
        const double* bucket = V.wbucket + (((size_t)w * 2 + V.par) * kSelBins + bin) * (size_t)V.bucket_cap;
        rp.c = select_finish_list(V, w, bucket, V.bucket_cap, in_bin, rank, 1, lo + ((unsigned long long)(bin - 1u) << V.warm_shift), false,
                                  sel_lh, sel_u, sel_keys);
        // (the histogram is still being read by the other blocks: the trial kernel of this call clears it)
    } else if (V.median_ready) {
        rp.c = sc.c_obs;        // k_select_finish
    } else {
        rp.c = select_finish(V, w, sel_lh, sel_u, sel_keys);
        if (blockIdx.x == 0) {
            if (threadIdx.x == 0) sc.c_obs = rp.c;      // the trial kernel centres the next call's warm bins on it
            // the select of this call is over (its last reader of the digit-0 histogram was the kernel in front): clean for
            // the call after next, which shares the parity
            unsigned* h0 = hist0_of(V, w, V.par);
            for (int b = threadIdx.x; b < kSelBins; b += 256) h0[b] = 0u;
        }
    }
    VBA_ASTAMP(2);
    rp.inv_c = 1.0 / rp.c;
    rp.inv_c2 = 1.0 / (rp.c * rp.c);
    rp.am2 = prm.am2;
    rp.inv_am2 = 1.0 / prm.am2;
    rp.expo = prm.expo;
    rp.alpha_is_2 = prm.alpha_is_2;
    rp.expo_is_mhalf = prm.expo == -0.5;

    // Phase 3: weights and accumulation.
    // J_k = [ -A R^T | 2 A hat(p_c) ] with A = d uv / d p_c (four non-zeros) and R the pose's rotation, the same for every row
    // of the pose.  CAM (groups of <= 16 lanes: a lane sees a dozen rows or more): the lane sums in the CAMERA frame --
    // G_k = [ -A | 2 A hat(p_c) ], whose translation part is the sparse A itself -- and rotates its sums once at the end
    // (J^T J = T G^T G T^T, T = diag(R, I)): ~130 VALU instructions per row instead of ~215.  Few rows per lane (latency
    // mode, 32 / 64 lanes per pose): the rotation per lane would cost what it saves, J is formed per row.
    constexpr bool CAM = G <= 16 || F32;
    double acc[32];         // 21 + 6 sums, padded to a power of two for the halving reduction
#pragma unroll
    for (int q = 0; q < 32; ++q) acc[q] = 0.0;
    // CAM sums: M = sum wc A^T A (00, 02, 11, 12, 22; 01 = 0), T[j][c] = sum wc A[:,j] . Gr[:,c], Crr = sum wc Gr^T Gr (upper),
    // st = sum wc A^T r, gr = sum wc Gr^T r
    double cM[5] = {0, 0, 0, 0, 0}, cT[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, cS[3] = {0, 0, 0};
    if (i < n) {
        auto process = [&](double ox_, double oy_, double oz_, double ou_, double ov_, double oc_, int k) {
            double u, v, cam[3], d;
            project(pc, ox_, oy_, oz_, u, v, cam, d);
            const double ru = ou_ - u, rv = ov_ - v;
            const double wr = robust_weight_raw(rp, ru, rv);
            V.wraw[mb + k] = wr;
            wmax_l = fmax(wmax_l, wr);
            const double wc = wr * oc_;
            // the camera-frame sums of one row (CAM): terms of A and Gr = 2 A hat(p_c), rows (g0..g2) and (h0..h2)
            auto cam_sums = [&](double a00, double a02, double a11, double a12, double g0, double g1, double g2, double h0, double h1,
                                double h2) {
                const double w00 = wc * a00, w02 = wc * a02, w11 = wc * a11, w12 = wc * a12;
                cM[0] = fma(w00, a00, cM[0]); cM[1] = fma(w00, a02, cM[1]);
                cM[2] = fma(w11, a11, cM[2]); cM[3] = fma(w11, a12, cM[3]);
                cM[4] = fma(w02, a02, fma(w12, a12, cM[4]));
                cT[0] = fma(w00, g0, cT[0]); cT[1] = fma(w00, g1, cT[1]); cT[2] = fma(w00, g2, cT[2]);
                cT[3] = fma(w11, h0, cT[3]); cT[4] = fma(w11, h1, cT[4]); cT[5] = fma(w11, h2, cT[5]);
                cT[6] = fma(w02, g0, fma(w12, h0, cT[6])); cT[7] = fma(w02, g1, fma(w12, h1, cT[7]));
                cT[8] = fma(w02, g2, fma(w12, h2, cT[8]));
                const double wg0 = wc * g0, wg1 = wc * g1, wg2 = wc * g2, wh0 = wc * h0, wh1 = wc * h1, wh2 = wc * h2;
                // rotation-rotation block straight into its place in the packed 6x6 (rows 3..5)
                acc[15] = fma(wg0, g0, fma(wh0, h0, acc[15])); acc[16] = fma(wg0, g1, fma(wh0, h1, acc[16]));
                acc[17] = fma(wg0, g2, fma(wh0, h2, acc[17])); acc[18] = fma(wg1, g1, fma(wh1, h1, acc[18]));
                acc[19] = fma(wg1, g2, fma(wh1, h2, acc[19])); acc[20] = fma(wg2, g2, fma(wh2, h2, acc[20]));
                cS[0] = fma(w00, ru, cS[0]); cS[1] = fma(w11, rv, cS[1]); cS[2] = fma(w02, ru, fma(w12, rv, cS[2]));
                acc[24] = fma(wg0, ru, fma(wh0, rv, acc[24])); acc[25] = fma(wg1, ru, fma(wh1, rv, acc[25]));
                acc[26] = fma(wg2, ru, fma(wh2, rv, acc[26]));
            };
            if constexpr (F32) {        // the fp32 terms, widened: products and sums in fp64
                const CamJac32 j = cam_jacobian_f32(pc, cam, d);
                cam_sums(j.a00, j.a02, j.a11, j.a12, j.g0, j.g1, j.g2, j.h0, j.h1, j.h2);
            } else if (CAM) {
                const double live = cam[2] > kZMin ? 1.0 : 0.0;
                const double a00 = pc.fx * d, a11 = pc.fy * d;
                const double dl = d * live;
                const double a02 = -(a00 * (cam[0] * dl)), a12 = -(a11 * (cam[1] * dl));
                const double x = cam[0], y = cam[1], z = cam[2];
                const double b00 = 2.0 * a00, b02 = 2.0 * a02, b11 = 2.0 * a11, b12 = 2.0 * a12;
                const double g0 = -(b02 * y), g1 = fma(b02, x, -(b00 * z)), g2 = b00 * y;
                const double h0 = fma(b11, z, -(b12 * y)), h1 = b12 * x, h2 = -(b11 * x);
                cam_sums(a00, a02, a11, a12, g0, g1, g2, h0, h1, h2);
            } else {
                double J[12];
                project_jacobian(pc, cam, d, J);
                int q = 0;
#pragma unroll
                for (int a = 0; a < 6; ++a) {
                    const double ja = wc * J[a], jb = wc * J[6 + a];
#pragma unroll
                    for (int b = a; b < 6; ++b) { acc[q] = fma(ja, J[b], fma(jb, J[6 + b], acc[q])); ++q; }
                    acc[21 + a] = fma(ja, ru, fma(jb, rv, acc[21 + a]));
                }
            }
        };
        if (PAIR) {
            int k = beg + 2 * sub;
            while (k < end) {
                const int kn = k + 2 * G;
                const Obs2 cur = nxt;
                if (kPairDepth2) {
                    nxt = nxt2;
                    if (kn + 2 * G < end) nxt2 = load2(kn + 2 * G);
                } else if (kn < end) nxt = load2(kn);
                process(cur.x.a, cur.y.a, cur.z.a, cur.u.a, cur.v.a, cur.c.a, k);
                if (k + 1 < end) process(cur.x.b, cur.y.b, cur.z.b, cur.u.b, cur.v.b, cur.c.b, k + 1);
                k = kn;
            }
        } else {
            int k = beg + sub;
            while (k < end) {
                const int kn = k + G;
                const Obs cur = ring[0];
#pragma unroll
                for (int d = 0; d + 1 < kAccDepth; ++d) ring[d] = ring[d + 1];
                if (k + kAccDepth * G < end) ring[kAccDepth - 1] = load(k + kAccDepth * G);
                process(cur.x, cur.y, cur.z, cur.u, cur.v, cur.c, k);
                k = kn;
            }
        }
    }
    VBA_ASTAMP(3);
    if (CAM) {
        // the lane's camera-frame sums into the world frame (sums are linear, so before the reduction):
        //   Htt = R M R^T, Htr = -R T, bt = -R st   (Jt = -A R^T; R[c][j] = pc.R[3 c + j])
        const double* R = pc.R;
        const double M[3][3] = {{cM[0], 0.0, cM[1]}, {0.0, cM[2], cM[3]}, {cM[1], cM[3], cM[4]}};
        double Y[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int kk = 0; kk < 3; ++kk) Y[a][kk] = fma(R[3 * a], M[0][kk], fma(R[3 * a + 1], M[1][kk], R[3 * a + 2] * M[2][kk]));
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int b = a; b < 3; ++b)
                acc[sym6(a, b)] = fma(Y[a][0], R[3 * b], fma(Y[a][1], R[3 * b + 1], Y[a][2] * R[3 * b + 2]));
#pragma unroll
            for (int c = 0; c < 3; ++c)
                acc[sym6(a, 3 + c)] = -fma(R[3 * a], cT[c], fma(R[3 * a + 1], cT[3 + c], R[3 * a + 2] * cT[6 + c]));
            acc[21 + a] = -fma(R[3 * a], cS[0], fma(R[3 * a + 1], cS[1], R[3 * a + 2] * cS[2]));
        }
    }
    // Reduction over the G lanes of the pose by recursive halving: in step s (xor mask 2^s) a lane keeps the half of its
    // values that bit s of its lane index selects and receives the partner's partial sums of that half -- 16 + 8 + 4 + 2 + 1
    // shuffles for the (padded) 32 values instead of 27 per butterfly step; afterwards every lane owns the totals of
    // 32 / min(G, 32) consecutive values.  The shape is fixed by G, so the sums are bit reproducible.
    VBA_ASTAMP(4);
    int own = 0;
    halving_steps<G, 32, 1>(acc, sub, own);
    if (G == 64) acc[0] += shfl_xor_f64_c<32>(acc[0]);
    if (i < n && sub < 32) {
        double* H = V.Hraw + pb * 21;
        double* B = V.braw + pb * 6;
        constexpr int kOwn = 32 / (G < 32 ? G : 32);
#pragma unroll
        for (int j = 0; j < kOwn; ++j) {
            const int q = own + j;
            if (q < 21) H[q] = acc[j];
            else if (q < 27) B[q - 21] = acc[j];
        }
    }
    VBA_ASTAMP(5);
    if (!BATCH) break;
    }       // groups of this block
    wmax_l = wave_max(wmax_l);
    if ((threadIdx.x & 63) == 0) wmx[threadIdx.x >> 6] = wmax_l;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double mx = fmax(fmax(wmx[0], wmx[1]), fmax(wmx[2], wmx[3]));
        atomicMax(V.wmax_ext ? V.wmax_ext : &sc.wmax_bits[V.par], f64_bits(mx));     // positive doubles order like their bit patterns
    }
    VBA_ASTAMP(6);
}

template <bool F32>
static void launch_acc_batch(int G, dim3 g, dim3 b, hipStream_t s, const DevView& V) {
    if (G == 8) hipLaunchKernelGGL((k_obs_accumulate<8, kPair, true, F32>), g, b, 0, s, V);
    else hipLaunchKernelGGL((k_obs_accumulate<16, false, true, F32>), g, b, 0, s, V);
}

template <bool F32>
static void launch_acc_lanes(int G, dim3 g, dim3 b, hipStream_t s, const DevView& V) {
    switch (G) {
        case 4: hipLaunchKernelGGL((k_obs_accumulate<4, kPair, false, F32>), g, b, 0, s, V); break;
        case 8: hipLaunchKernelGGL((k_obs_accumulate<8, kPair, false, F32>), g, b, 0, s, V); break;
        case 16: hipLaunchKernelGGL((k_obs_accumulate<16, false, false, F32>), g, b, 0, s, V); break;
        case 32: hipLaunchKernelGGL((k_obs_accumulate<32, false, false, F32>), g, b, 0, s, V); break;
        default: hipLaunchKernelGGL((k_obs_accumulate<64, false, false, F32>), g, b, 0, s, V); break;
    }
}

void launch_obs_accumulate(const DevView& V, hipStream_t s) {
    const int G = V.acc_lanes;
    const int nb = (V.n_max * G + 255) / 256;
    // V.dyn_in_acc: the blocks of the dynamics factor are appended to the grid
    // V.sel_inline: one more block, which evaluates the folded accept test and records the start of the call
    const dim3 g(nb + (V.dyn_in_acc ? (V.n_max * kDynLanes + 255) / 256 : 0) + (V.sel_inline ? 1 : 0), V.W), b(256);
    if (V.median_ready && !V.dyn_in_acc && !V.sel_inline && (G == 8 || G == 16)) {      // many windows per launch
        // a block walks up to VBA_ACC_GROUPS groups of poses (its grid stride) -- fewer when the windows of the handle would
        // otherwise leave compute units without a block (the chip holds 512 of these blocks at once)
        int groups = VBA_ACC_GROUPS;
        while (groups > 1 && (int64_t)V.W * ((nb + groups - 1) / groups) < 2048) groups >>= 1;
        if (acc_groups_env() > 0) groups = acc_groups_env();
        const dim3 gb((nb + groups - 1) / groups, V.W);
        if (V.jac_f32) launch_acc_batch<true>(G, gb, b, s, V);
        else launch_acc_batch<false>(G, gb, b, s, V);
        return;
    }
    if (V.jac_f32) launch_acc_lanes<true>(G, g, b, s, V);
    else launch_acc_lanes<false>(G, g, b, s, V);
    // the long edges of the dynamics factor that rode in this grid (behind the folded accept test: the window has moved on to
    // this call, or the kernel leaves it alone as every later kernel of the call does)
    if (V.dyn_in_acc) launch_long_factor(V, s);
}

}  // namespace vba

// k_trial is compiled as part of this unit, not as one of its own.  Its pose-chain blocks and the dynamics rider above both
// inline accel_lin (vba_math.h), whose sums are left to the compiler to contract, and which products it fuses depends on the
// callers it sees in the unit: in a unit without the rider every k_trial rounds -k3 p + k7 u p the other way round
// (fma(p, -k3, k7 u p) instead of fma(k7 u, p, -(k3 p))), a last-bit change of every trial residual of the pose chain.
#include "vba_trial.hip"
