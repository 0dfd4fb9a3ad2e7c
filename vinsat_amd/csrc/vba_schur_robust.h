// vba_schur_robust.h -- what the entry points of vba_schur_robust.hip fill from the handle (vba_schur_context.h) and its kernels take
// by value: the arrays the passes of vba_schur_reweight read and write, the exact radix select that vba_schur_median runs on its own, and their
// launchers.  Internal.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vba {

// Shape of the select (tests/test_gpu_schur_median.py reads these to place its counts on every boundary)
constexpr int kSelDigitBits = 8;            // digit of the radix select: 8 passes over the 64 bits of a key
constexpr int kSelThreads = 256;            // threads of a workgroup, one per histogram bin
constexpr int kSelKeysPerThread = 8;        // keys of one thread in one tile, as four 16-byte loads
constexpr int kSelMaxBlocks = 128;          // workgroups of a pass: a launch covers kSelMaxBlocks tiles, then strides
constexpr int kSelSmallMax = 8192;          // up to this many keys one workgroup runs all passes in one launch

constexpr int kSelPasses = 64 / kSelDigitBits;
constexpr int kSelBins = 1 << kSelDigitBits;
constexpr int kSelTile = kSelThreads * kSelKeysPerThread;       // keys of a workgroup per tile
constexpr int kRobustMaxBlocks = 256;       // workgroups of the raw-weight pass = partial maxima the scaling pass reduces

// Scratch of one select: hist [kSelPasses][kSelBins] (zeroed by the launcher), state [kSelPasses + 1][2] = (prefix, rank)
struct SchurSelectView {
    const unsigned long long* keys;     // [count] bit patterns of non-negative doubles (16-byte aligned)
    int64_t count;
    unsigned long long* hist;
    unsigned long long* state;
    double* out;                        // [1] the key of rank (count - 1) / 2
};

inline size_t schur_select_scratch_bytes() { return ((size_t)kSelPasses * kSelBins + 2 * (kSelPasses + 1)) * 8; }
// the select on stream s; *launches (if given) gets the number of kernel launches
void schur_select_launch(const SchurSelectView& W, hipStream_t s, int* launches);

struct SchurRobustView {
    int n, L;
    int64_t m;
    // the handle's rows (sorted by landmark), measurement, intrinsics and the resident state
    const int *row_pose, *row_lm;
    const double *row_u, *row_v, *intr, *states, *X;
    double* row_w;                      // [m] the handle's weights, rewritten in place
    double* saved;                      // [m] the snoop's saved weights, or NULL on a handle that never snooped
    const unsigned char* row_mask;      // [m] the snoop's row mask, or NULL
    // feature state (lives from the first re-weighting of a handle to its next upload)
    double* base;                       // [m] the weights as uploaded
    double* keys;                       // [2 m] |r|, row by row, u before v
    double* q;                          // [m] raw weights
    double* part;                       // [kRobustMaxBlocks] partial maxima of q
    double* res;                        // [2] c_obs, q_max
    SchurSelectView sel;
};

// base[k] = the weight row k was uploaded with (the saved one for a row the snoop rejected)
void schur_robust_capture_launch(const SchurRobustView& V, hipStream_t s);
// keys, select, raw weights, scaling, on stream s; returns the number of kernel launches
int schur_robust_launch(const SchurRobustView& V, double alpha, hipStream_t s);

}  // namespace vba
