// vba_schur_snoop_pick.h -- the decision rule of free-landmark data snooping (vba_schur_snoop, vba_schur_snoop.hip).  Plain C++
// that the device passes and a host program both compile (tests/hostcheck/hostcheck_schur_snoop.cpp,
// tests/test_schur_snoop_host.py); tests/schur_snoop_oracle.py restates it in NumPy.
//
// Candidates are (w-test value, sorted row) pairs under the strict total order of vba_snoop_pick.h (`better`: a NaN never wins,
// the larger value wins, equal values go to the smaller position).  The catalogue prior of a landmark takes part in its
// landmark's group with a position beyond every row (kSchurPriorPos), so a row beats the prior on a tie.
//   landmark pass   schur_lm_decide: the landmark is MARKED (kSchurMarked: its prior won), PROPOSES a row (the row's sorted index
//                   >= 0) or does neither (kSchurNone);
//   pose pass       a fold of `pick` over the proposed rows of the pose, then schur_pose_decide;
//   apply pass      a marked landmark is rejected iff none of the poses of its weighted rows is short.
#pragma once

#include <cmath>

#include "vba_snoop_pick.h"

namespace vba {

constexpr int kSchurNone = -2;              // the landmark neither marks nor proposes
constexpr int kSchurMarked = -1;            // the landmark's catalogue prior won its group
constexpr int kSchurPriorPos = 0x7ffffffe;  // position of the prior inside its group: after every row, before "no candidate"

// the effective critical value: crit, or crit * sqrt(s0sq) with `scaled` (the product of the correctly rounded root)
VBA_PICK_HD double schur_crit(double crit, int scaled, double s0sq) {
#if defined(__HIP_DEVICE_COMPILE__)
    return scaled ? __dmul_rn(crit, __dsqrt_rn(s0sq)) : crit;
#else
    return scaled ? crit * std::sqrt(s0sq) : crit;
#endif
}

// a critical value that can reject: finite (NaN and the infinities reject nothing)
VBA_PICK_HD bool schur_crit_live(double c) { return c - c == 0.0; }

// a test value that exceeds c: finite and larger (false for a NaN in either)
VBA_PICK_HD bool schur_exceeds(double t, double c) { return t - t == 0.0 && t > c; }

VBA_PICK_HD bool schur_row_candidate(double w, double wtest, double c) { return w > 0.0 && schur_exceeds(wtest, c); }

VBA_PICK_HD bool schur_prior_candidate(int cntl, int min_track, double lm_wtest, double c) {
    return cntl >= min_track && schur_exceeds(lm_wtest, c);
}

// Landmark pass: rows beg .. end - 1 (sorted order) of one landmark with weights w and tests wt, the test of its prior lm_wt.
// Returns kSchurNone, kSchurMarked or the proposed row; *cntl receives the rows of positive weight.
VBA_PICK_HD int schur_lm_decide(int beg, int end, const double* w, const double* wt, double lm_wt, int min_track, double c, int* cntl) {
    double best = __builtin_nan("");
    int pos = kSnoopNoPos, cnt = 0;
    const bool live = schur_crit_live(c);
    for (int k = beg; k < end; ++k) {
        const double wk = w[k];
        cnt += wk > 0.0 ? 1 : 0;
        if (live && schur_row_candidate(wk, wt[k], c)) pick(best, pos, wt[k], k);
    }
    *cntl = cnt;
    if (live && schur_prior_candidate(cnt, min_track, lm_wt, c)) pick(best, pos, lm_wt, kSchurPriorPos);
    return pos == kSnoopNoPos ? kSchurNone : (pos == kSchurPriorPos ? kSchurMarked : pos);
}

// Pose pass, after the fold: cnt weighted rows, c_lm of them on marked landmarks, bpos the best proposed row (kSnoopNoPos: none).
// *is_short: the pose cannot spare the rows of the marked landmarks.  Returns the row to reject, or -1.
VBA_PICK_HD int schur_pose_decide(int cnt, int c_lm, int bpos, int min_rows, int* is_short) {
    const int left = cnt - c_lm;
    *is_short = left < min_rows ? 1 : 0;
    return (bpos != kSnoopNoPos && left >= min_rows && left - 1 >= min_rows) ? bpos : -1;
}

}  // namespace vba
