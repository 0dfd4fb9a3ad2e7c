// Host build of the closed forms of vinsat_amd/csrc/vba_power_math.h (vba_outlier_power) for the CPU test-suite.
// Test infrastructure only: nothing in the product loads this.
#include "../../vinsat_amd/csrc/vba_power_math.h"
#include <cstdint>
using namespace vba;

extern "C" {

// per case: R = [a, b; b, d] -> mu_min
void hc_sym2_mu_min(int64_t count, const double* abd, double* out) {
    for (int64_t k = 0; k < count; ++k) out[k] = sym2_mu_min(abd[3 * k], abd[3 * k + 1], abd[3 * k + 2]);
}

// per case: M = [m00, m01; m01, m11], R = [a, b; b, d] -> the larger root of det(M - mu R) = 0
void hc_pair_mu_max(int64_t count, const double* M, const double* abd, double* out) {
    for (int64_t k = 0; k < count; ++k)
        out[k] = pair_mu_max(M[3 * k], M[3 * k + 1], M[3 * k + 2], abd[3 * k], abd[3 * k + 1], abd[3 * k + 2]);
}

// per case: z = R^-1 r
void hc_sym2_solve(int64_t count, const double* abd, const double* r, double* z) {
    for (int64_t k = 0; k < count; ++k) sym2_solve(abd[3 * k], abd[3 * k + 1], abd[3 * k + 2], r[2 * k], r[2 * k + 1], z[2 * k], z[2 * k + 1]);
}

}  // extern "C"
