// Host build of the decision rule of vinsat_amd/csrc/vba_schur_snoop_pick.h (vba_schur_snoop) for the CPU test-suite: the three
// passes in the shape the device runs them (thread per landmark; 16 lanes per pose with strided rows and a butterfly over masks
// 1, 2, 4, 8; thread per pose and per landmark for the stores) over the sorted structure arrays of a small problem.
// Test infrastructure only: nothing in the product loads this.
#include "../../vinsat_amd/csrc/vba_schur_snoop_pick.h"
#include <cstdint>
#include <vector>
using namespace vba;

extern "C" {

// Rows sorted by landmark (lm_ptr [L+1], row_pose [m]); the rows of a pose through pose_ptr [n+1] -> pose_rows [m].  w, wt [m],
// lmwt [L].  Outputs: row_own [m] (rejected by their own test), lm_rej [L], row_via [m] (zeroed with a rejected landmark),
// *crit_used.  Returns 1 if in every pose all 16 lanes ended with the same winner and the same counts, else 0.
int hc_schur_snoop(int n, int L, int m, const int* lm_ptr, const int* row_pose, const int* row_lm, const int* pose_ptr, const int* pose_rows,
                   const double* w, const double* wt, const double* lmwt, double s0sq, int info, double crit, int scaled, int min_rows,
                   int min_track, unsigned char* row_own, unsigned char* lm_rej, unsigned char* row_via, double* crit_used) {
    for (int k = 0; k < m; ++k) row_own[k] = row_via[k] = 0;
    for (int l = 0; l < L; ++l) lm_rej[l] = 0;
    const double c = schur_crit(crit, scaled, info != 0 ? __builtin_nan("") : s0sq);
    *crit_used = c;
    if (info != 0) return 1;
    std::vector<int> lm_dec(L), pose_pick(n), pose_short(n);
    for (int l = 0; l < L; ++l) {
        int cntl;
        lm_dec[l] = schur_lm_decide(lm_ptr[l], lm_ptr[l + 1], w, wt, lmwt[l], min_track, c, &cntl);
    }
    int agree = 1;
    for (int i = 0; i < n; ++i) {
        double best[16];
        int pos[16], cnt[16], clm[16];
        for (int sub = 0; sub < 16; ++sub) {
            best[sub] = __builtin_nan("");
            pos[sub] = kSnoopNoPos;
            cnt[sub] = clm[sub] = 0;
            for (int r = pose_ptr[i] + sub; r < pose_ptr[i + 1]; r += 16) {
                const int k = pose_rows[r];
                const bool on = w[k] > 0.0;
                const int dec = lm_dec[row_lm[k]];
                cnt[sub] += on ? 1 : 0;
                clm[sub] += (on && dec == kSchurMarked) ? 1 : 0;
                if (dec == k) pick(best[sub], pos[sub], wt[k], k);
            }
        }
        for (int mask = 1; mask < 16; mask <<= 1) {
            double nb[16];
            int np[16], nc[16], nm[16];
            for (int s = 0; s < 16; ++s) {
                nb[s] = best[s];
                np[s] = pos[s];
                nc[s] = cnt[s] + cnt[s ^ mask];
                nm[s] = clm[s] + clm[s ^ mask];
                pick(nb[s], np[s], best[s ^ mask], pos[s ^ mask]);
            }
            for (int s = 0; s < 16; ++s) { best[s] = nb[s]; pos[s] = np[s]; cnt[s] = nc[s]; clm[s] = nm[s]; }
        }
        for (int s = 1; s < 16; ++s)
            if (pos[s] != pos[0] || cnt[s] != cnt[0] || clm[s] != clm[0]) agree = 0;
        pose_pick[i] = schur_pose_decide(cnt[0], clm[0], pos[0], min_rows, &pose_short[i]);
    }
    for (int i = 0; i < n; ++i)
        if (pose_pick[i] >= 0) row_own[pose_pick[i]] = 1;
    for (int l = 0; l < L; ++l) {
        if (lm_dec[l] != kSchurMarked) continue;
        bool confirmed = true;
        for (int k = lm_ptr[l]; k < lm_ptr[l + 1]; ++k)
            if (w[k] > 0.0 && pose_short[row_pose[k]] != 0) confirmed = false;
        if (!confirmed) continue;
        lm_rej[l] = 1;
        for (int k = lm_ptr[l]; k < lm_ptr[l + 1]; ++k)
            if (w[k] > 0.0) row_via[k] = 1;
    }
    return agree;
}

int hc_schur_prior_pos(void) { return kSchurPriorPos; }

}  // extern "C"
