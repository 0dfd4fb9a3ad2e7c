// Host build of the closed forms of vinsat_amd/csrc/vba_schur_rel_math.h (vba_schur_reliability) for the CPU test-suite.
// Test infrastructure only: nothing in the product loads this.
#include "../../vinsat_amd/csrc/vba_schur_rel_math.h"
#include <cstdint>
using namespace vba;

extern "C" {

// per case: P = [p00, p01; p01, p11], r = (ru, rv), w -> sqrt(w r^T (I - P)^-1 r) or NaN
void hc_rel_wtest2(int64_t count, const double* P, const double* r, const double* w, double* out) {
    for (int64_t k = 0; k < count; ++k) out[k] = rel_wtest2(P[3 * k], P[3 * k + 1], P[3 * k + 2], r[2 * k], r[2 * k + 1], w[k]);
}

// per case: M = (00, 01, 02, 11, 12, 22), e[3], scale -> sqrt(scale e^T M^-1 e) or NaN
void hc_rel_wtest3(int64_t count, const double* M, const double* e, const double* scale, double* out) {
    for (int64_t k = 0; k < count; ++k) out[k] = rel_wtest3(M + 6 * k, e + 3 * k, scale[k]);
}

}  // extern "C"
