// Host build of the combine rule of vinsat_amd/csrc/vba_snoop_pick.h (vba_snoop) for the CPU test-suite.
// Test infrastructure only: nothing in the product loads this.
#include "../../vinsat_amd/csrc/vba_snoop_pick.h"
#include <cstdint>
using namespace vba;

extern "C" {

// the fold of a sequence in order, as a lane folds its rows: the winner's position, or kSnoopNoPos
int hc_snoop_fold(int64_t count, const double* val) {
    double best = __builtin_nan("");
    int pos = kSnoopNoPos;
    for (int64_t k = 0; k < count; ++k) pick(best, pos, val[k], (int)k);
    return pos;
}

// the fold in the shape of the device: 16 lanes, lane l folds elements l, l + 16, ..., then a butterfly over masks 1, 2, 4, 8
// in which every lane combines with its partner; *agree receives 1 if all 16 lanes end with the same winner
int hc_snoop_butterfly(int64_t count, const double* val, int* agree) {
    double best[16];
    int pos[16];
    for (int l = 0; l < 16; ++l) {
        best[l] = __builtin_nan("");
        pos[l] = kSnoopNoPos;
        for (int64_t k = l; k < count; k += 16) pick(best[l], pos[l], val[k], (int)k);
    }
    for (int mask = 1; mask < 16; mask <<= 1) {
        double nb[16];
        int np[16];
        for (int l = 0; l < 16; ++l) {
            nb[l] = best[l];
            np[l] = pos[l];
            pick(nb[l], np[l], best[l ^ mask], pos[l ^ mask]);
        }
        for (int l = 0; l < 16; ++l) { best[l] = nb[l]; pos[l] = np[l]; }
    }
    *agree = 1;
    for (int l = 1; l < 16; ++l) if (pos[l] != pos[0]) *agree = 0;
    return pos[0];
}

int hc_snoop_no_pos(void) { return kSnoopNoPos; }

}  // extern "C"
