// vba_schur_snoop.hip -- the passes of free-landmark data snooping (vba_schur_snoop; include/vinsat_ba.h carries the contract, the
// entry points and the handle live in vba_schur.hip).  They run behind the device part of vba_schur_reliability on the handle's
// stream and read what it left: wtest of every row, lm_wtest of every catalogue prior, fit[5] = s0sq.  At most one rejection per
// group; the rule is vba_schur_snoop_pick.h.
//
//   k_schur_snoop_lm      thread per landmark over its contiguous rows (landmark-sorted): the effective critical value from the
//                         device's own fit, the landmark's weighted rows, its best row candidate against its prior candidate ->
//                         lm_dec[l] = marked / the proposed row / nothing
//   k_schur_snoop_pose    16 lanes per pose over pose_rows: weighted rows, weighted rows on marked landmarks and the best proposed
//                         row (largest wtest, ties to the smaller sorted row) meet in a butterfly of four DPP exchanges whose shape
//                         depends on nothing; the rule is a strict total order, so all 16 lanes end on one winner.  Position and
//                         count travel as one 64-bit word.
//   k_schur_snoop_apply   thread per pose: the owner of the pose's rejected row saves its weight, stores 0.0, sets its mask byte;
//                         thread per landmark: a marked landmark none of whose weighted rows sits in a short pose does the same
//                         for its segment and sets the landmark byte
//   k_schur_snoop_restore thread per row: the saved weight back, the mask byte cleared
// No atomics, plain vector stores, a thread writes only rows it owns (a landmark either marks or proposes, so the rows of the pose
// threads and of the landmark threads are disjoint): equal problems give equal bits.
#include <algorithm>

#include "vba_device.h"
#include "vba_schur_snoop.h"
#include "vba_schur_snoop_pick.h"

namespace vba {

__global__ __launch_bounds__(256) void k_schur_snoop_lm(SchurSnoopView V, double crit, int scaled, int min_track) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    const double c = schur_crit(crit, scaled, V.fit[5]);
    if (l == 0) V.crit_used[0] = c;
    if (l >= V.L) return;
    int cntl;
    V.lm_dec[l] = schur_lm_decide(V.lm_ptr[l], V.lm_ptr[l + 1], V.row_w, V.wt, V.lmwt[l], min_track, c, &cntl);
}

// One step of the pose butterfly: the partner's best (wtest, row) and its two counts; row and count travel as one 64-bit word
template <int MASK>
__device__ __forceinline__ void schur_snoop_exchange(double& best, int& bpos, int& cnt, int& clm) {
    const double o_val = shfl_xor_f64_c<MASK>(best);
    const unsigned long long mine = ((unsigned long long)(unsigned)cnt << 32) | (unsigned)bpos;
    const unsigned long long theirs = (unsigned long long)__double_as_longlong(shfl_xor_f64_c<MASK>(__longlong_as_double((long long)mine)));
    const unsigned long long marked = (unsigned long long)__double_as_longlong(
        shfl_xor_f64_c<MASK>(__longlong_as_double((long long)(unsigned long long)(unsigned)clm)));
    cnt += (int)(unsigned)(theirs >> 32);
    clm += (int)(unsigned)marked;
    pick(best, bpos, o_val, (int)(unsigned)theirs);
}

__global__ __launch_bounds__(256) void k_schur_snoop_pose(SchurSnoopView V, int min_rows) {
    const int i = blockIdx.x * 16 + (threadIdx.x >> 4), sub = threadIdx.x & 15;
    const bool live = i < V.n;                          // (the lanes of a group beyond n stay in the butterfly with nothing)
    const int beg = live ? V.pose_ptr[i] : 0, end = live ? V.pose_ptr[i + 1] : 0;
    double best = __builtin_nan("");
    int bpos = kSnoopNoPos, cnt = 0, clm = 0;
    for (int r = beg + sub; r < end; r += 16) {
        const int k = V.pose_rows[r];
        const bool on = V.row_w[k] > 0.0;
        const int dec = V.lm_dec[V.row_lm[k]];
        cnt += on ? 1 : 0;
        clm += (on && dec == kSchurMarked) ? 1 : 0;
        if (dec == k) pick(best, bpos, V.wt[k], k);     // (a proposed row is a candidate: positive weight, finite test)
    }
    schur_snoop_exchange<1>(best, bpos, cnt, clm); schur_snoop_exchange<2>(best, bpos, cnt, clm);
    schur_snoop_exchange<4>(best, bpos, cnt, clm); schur_snoop_exchange<8>(best, bpos, cnt, clm);
    int is_short;
    const int rej = schur_pose_decide(cnt, clm, bpos, min_rows, &is_short);
    if (live && sub == 0) {
        V.pose_pick[i] = rej;
        V.pose_short[i] = is_short;
    }
}

__global__ __launch_bounds__(256) void k_schur_snoop_apply(SchurSnoopView V) {
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id < V.n) {
        const int k = V.pose_pick[id];
        if (k >= 0 && (int64_t)k < V.m) {
            V.saved[k] = V.row_w[k];
            V.row_w[k] = 0.0;
            V.row_mask[k] = 1;
        }
        V.pose_out[id] = k >= 0 ? 1 : 0;
    }
    if (id < V.L) {
        int out = 0;
        if (V.lm_dec[id] == kSchurMarked) {
            const int beg = V.lm_ptr[id], end = V.lm_ptr[id + 1];
            bool confirmed = true;
            for (int k = beg; k < end; ++k)
                if (V.row_w[k] > 0.0 && V.pose_short[V.row_pose[k]] != 0) confirmed = false;
            if (confirmed) {
                int zeroed = 0;
                for (int k = beg; k < end; ++k) {
                    const double w = V.row_w[k];
                    if (w > 0.0) {
                        V.saved[k] = w;
                        V.row_w[k] = 0.0;
                        V.row_mask[k] = 1;
                        ++zeroed;
                    }
                }
                V.lm_mask[id] = 1;
                out = 1 + zeroed;
            }
        }
        V.lm_out[id] = out;
    }
}

__global__ __launch_bounds__(256) void k_schur_snoop_restore(SchurSnoopView V) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= V.m || !V.row_mask[k]) return;
    V.row_w[k] = V.saved[k];
    V.row_mask[k] = 0;
}

void schur_snoop_launch(const SchurSnoopView& V, double crit, int scaled, int min_rows, int min_track, hipStream_t s) {
    hipLaunchKernelGGL(k_schur_snoop_lm, dim3((V.L + 255) / 256), dim3(256), 0, s, V, crit, scaled, min_track);
    hipLaunchKernelGGL(k_schur_snoop_pose, dim3((V.n + 15) / 16), dim3(256), 0, s, V, min_rows);
    hipLaunchKernelGGL(k_schur_snoop_apply, dim3((std::max(V.L, V.n) + 255) / 256), dim3(256), 0, s, V);
}

void schur_snoop_restore_launch(const SchurSnoopView& V, hipStream_t s) {
    hipLaunchKernelGGL(k_schur_snoop_restore, dim3((unsigned)((V.m + 255) / 256)), dim3(256), 0, s, V);
}

}  // namespace vba
