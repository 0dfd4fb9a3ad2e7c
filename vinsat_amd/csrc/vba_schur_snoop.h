// vba_schur_snoop.h -- the arrays the passes of vba_schur_snoop (vba_schur_snoop.hip) read and write, and their launchers: what the
// entry points fill from the handle (vba_schur_context.h) and the kernels take by value.  Internal.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vba {

struct SchurSnoopView {
    int n, L;
    int64_t m;
    // structure of the handle (rows sorted by landmark)
    const int *lm_ptr, *row_pose, *row_lm, *pose_ptr, *pose_rows;
    double* row_w;                  // [m] the handle's weights: rejected rows become 0.0 in place
    // outputs of the reliability passes at this state
    const double *wt, *lmwt, *fit;  // [m], [L], [8]
    // feature state (lives from the first snoop of a handle to its next upload)
    double* saved;                  // [m] the weight a rejected row had
    unsigned char* row_mask;        // [m] cumulative
    unsigned char* lm_mask;         // [L] cumulative
    // per call
    int* lm_dec;                    // [L] kSchurNone / kSchurMarked / the proposed row
    int* pose_pick;                 // [n] the row the pose rejects, or -1
    int* pose_short;                // [n] 1: the pose cannot spare the rows of its marked landmarks
    int* pose_out;                  // [n] rows the pose lost by their own test in this call (0 / 1)
    int* lm_out;                    // [L] 0, or 1 + the rows zeroed with the rejected landmark
    double* crit_used;              // [1]
};

// the three passes of one call, on stream s
void schur_snoop_launch(const SchurSnoopView& V, double crit, int scaled, int min_rows, int min_track, hipStream_t s);
// saved weights back, row mask cleared (the landmark mask is the caller's to clear)
void schur_snoop_restore_launch(const SchurSnoopView& V, hipStream_t s);

}  // namespace vba
