// vba_schur_snoop.hip -- free-landmark data snooping (vba_schur_snoop, vba_schur_snoop_dyn, vba_schur_snoop_att, vba_schur_rejected, vba_schur_snoop_restore;
// include/vinsat_ba.h carries the contract, vba_schur_context.h the handle, vba_schur.hip the map of the units): its passes, then the
// entry points.  The passes run behind the device part of vba_schur_reliability (of vba_schur_reliability_dyn on a handle with the
// dynamics factor: the same passes on the same scratch) on the handle's
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
#include "vba_schur_context.h"
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

// first snoop of a handle: its state (masks cleared) and its two timing events
static int schur_snoop_alloc(vba_schur_handle h) {
    SchurSnoop& Z = h->snoop;
    if (Z.sc.arena) return VBA_OK;
    const SchurView& V = h->V;
    const size_t m = (size_t)V.m, L = (size_t)V.L, n = (size_t)V.n;
    SchurLayout lay;
    const size_t o_sv = lay.need(m * 8), o_cr = lay.need(8), o_rm = lay.need(m), o_lk = lay.need(L), o_ld = lay.need(L * 4), o_pp = lay.need(n * 4),
                 o_ps = lay.need(n * 4), o_po = lay.need(n * 4), o_lo = lay.need(L * 4);
    if (int rc = schur_scratch_alloc(Z.sc, lay.bytes, "snooping state")) return rc;
    char* A = Z.sc.arena;
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

// The body of vba_schur_snoop, vba_schur_snoop_dyn and vba_schur_snoop_att (kind: the handle has the dynamics factor, or the attitude
// factor too, and the tests come from the device part of vba_schur_reliability_dyn / vba_schur_reliability_att; the passes, the masks
// and the saved weights are the same -- edges of either kind are never rejected).
static int schur_snoop_call(vba_schur_handle h, SchurKind kind, double lamda, double crit, int scaled, int min_rows, int min_track, int* counts,
                            double* crit_used, int* info) {
    if (!(lamda >= 0.0)) return sfail(VBA_EINVAL, "lamda must be >= 0");
    if (!(crit >= 0.0)) return sfail(VBA_EINVAL, "crit must be >= 0 (+inf rejects nothing)");
    if (min_rows < 0 || min_track < 0) return sfail(VBA_EINVAL, "min_rows and min_track must be >= 0");
    if (int rc = schur_query_begin(h, kind, kind == kSchurPlain ? "vba_schur_snoop" : "vba_schur_snoop_dyn")) return rc;
    if (int rc = schur_rel_alloc(h)) return rc;
    if (int rc = schur_snoop_alloc(h)) return rc;
    SchurSnoop& Z = h->snoop;
    hipStream_t s = h->stream;
    SchurView V;
    int bad = 0;
    if (int rc = schur_rel_device(h, kind, lamda, Z.sc.ev[0], V, &bad)) return rc;
    *info = bad;
    if (counts) counts[0] = counts[1] = counts[2] = 0;
    if (bad != 0) {                 // no factor, no test: nothing is rejected; the critical value of a fit that does not exist
        if (int rc = schur_scratch_finish(Z.sc, s)) return rc;
        if (crit_used) *crit_used = scaled ? std::nan("") : crit;
        return VBA_OK;
    }
    const SchurSnoopView W = schur_snoop_view(h);
    schur_snoop_launch(W, crit, scaled ? 1 : 0, min_rows, min_track, s);
    std::vector<int> out;
    double c = 0.0;
    const int rc = schur_scratch_finish(Z.sc, s, [&]() -> int {
        SCHK(hipGetLastError());
        try {
            out.resize((size_t)V.n + (size_t)V.L);
        } catch (const std::bad_alloc&) {
            return sfail(VBA_ENOMEM, "host staging for the counts of vba_schur_snoop failed");
        }
        SCHK(hipMemcpyAsync(out.data(), Z.pose_out, (size_t)V.n * 4, hipMemcpyDeviceToHost, s));
        SCHK(hipMemcpyAsync(out.data() + V.n, Z.lm_out, (size_t)V.L * 4, hipMemcpyDeviceToHost, s));
        SCHK(hipMemcpyAsync(&c, Z.crit_used, 8, hipMemcpyDeviceToHost, s));
        return VBA_OK;
    });
    if (rc) return rc;
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

extern "C" {

int vba_schur_snoop(vba_schur_handle h, double lamda, double crit, int scaled, int min_rows, int min_track, int* counts, double* crit_used,
                    int* info) {
    if (!h || !info) return sfail(VBA_EINVAL, "null argument");
    if (int rc = schur_kind_check(kSchurPlain, h, "vba_schur_snoop")) return rc;
    return schur_snoop_call(h, kSchurPlain, lamda, crit, scaled, min_rows, min_track, counts, crit_used, info);
}

int vba_schur_snoop_dyn(vba_schur_handle h, double lamda, double crit, int scaled, int min_rows, int min_track, int* counts, double* crit_used,
                        int* info) {
    if (!h || !info) return sfail(VBA_EINVAL, "null argument");
    return schur_snoop_call(h, kSchurDyn, lamda, crit, scaled, min_rows, min_track, counts, crit_used, info);
}

int vba_schur_last_snoop_dyn_ms(vba_schur_handle h, float* ms) { return schur_last_ms(h, &vba_schur_context::snoop, ms); }

int vba_schur_snoop_att(vba_schur_handle h, double lamda, double crit, int scaled, int min_rows, int min_track, int* counts, double* crit_used,
                        int* info) {
    if (!h || !info) return sfail(VBA_EINVAL, "null argument");
    return schur_snoop_call(h, kSchurAtt, lamda, crit, scaled, min_rows, min_track, counts, crit_used, info);
}

int vba_schur_last_snoop_att_ms(vba_schur_handle h, float* ms) { return schur_last_ms(h, &vba_schur_context::snoop, ms); }

int vba_schur_rejected(vba_schur_handle h, unsigned char* row_mask, unsigned char* lm_mask, int* totals) {
    if (!h) return sfail(VBA_EINVAL, "null handle");
    const SchurSnoop& Z = h->snoop;
    if (totals) for (int k = 0; k < 3; ++k) totals[k] = Z.sc.arena ? Z.totals[k] : 0;
    if (!Z.sc.arena) {
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
    if (!Z.sc.arena || (Z.totals[0] == 0 && Z.totals[1] == 0 && Z.totals[2] == 0)) return VBA_OK;
    SCHK(hipSetDevice(h->device));
    schur_snoop_restore_launch(schur_snoop_view(h), h->stream);
    SCHK(hipGetLastError());
    SCHK(hipMemsetAsync(Z.lm_mask, 0, (size_t)h->V.L, h->stream));
    SCHK(hipStreamSynchronize(h->stream));
    std::fill(Z.totals, Z.totals + 3, 0);
    return VBA_OK;
}

int vba_schur_last_snoop_ms(vba_schur_handle h, float* ms) { return schur_last_ms(h, &vba_schur_context::snoop, ms); }

}  // extern "C"
