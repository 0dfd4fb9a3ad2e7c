// Host build of the closed forms of vinsat_amd/csrc/vba_schur_power_math.h (vba_schur_outlier_power) for the CPU test-suite.
// Test infrastructure only: nothing in the product loads this.
#include "../../vinsat_amd/csrc/vba_schur_power_math.h"
#include <cstdint>
using namespace vba;

extern "C" {

// per case: symmetric 3x3 (00, 01, 02, 11, 12, 22) -> its largest eigenvalue
void hc_sym3_mu_max(int64_t count, const double* M, double* out) {
    for (int64_t k = 0; k < count; ++k) out[k] = sym3_mu_max(M + 6 * k);
}

// per row: w, P = (p00, p01, p11), r = (ru, rv), T = Sigma_k J_k^T [9][2] row major -> the six figures
void hc_pow_row(int64_t count, const double* w, const double* P, const double* r, const double* T, double ncp, double* out) {
    for (int64_t k = 0; k < count; ++k) {
        double tu[9], tv[9];
        for (int a = 0; a < 9; ++a) { tu[a] = T[18 * k + 2 * a]; tv[a] = T[18 * k + 2 * a + 1]; }
        schur_pow_row(w[k], P[3 * k], P[3 * k + 1], P[3 * k + 2], r[2 * k], r[2 * k + 1], tu, tv, ncp, out + 6 * k);
    }
}

// per landmark: P_l (six numbers), sigma -> lm_mdb, lm_ext
void hc_pow_prior(int64_t count, const double* P, double sigma, double ncp, double* out) {
    for (int64_t l = 0; l < count; ++l) schur_pow_prior(P + 6 * l, sigma, ncp, out[2 * l], out[2 * l + 1]);
}

// per row: the first three rows of Sigma_il (3x3 row major), P_l of its landmark, e_l -> the pull; and det(I - P_l)
void hc_pow_pull(int64_t count, const double* G3, const double* P, const double* e, double inv_sigma2, double* out, double* det) {
    for (int64_t k = 0; k < count; ++k) {
        out[k] = schur_pow_pull(G3 + 9 * k, P + 6 * k, e + 3 * k, inv_sigma2);
        det[k] = schur_pow_prior_det(P + 6 * k);
    }
}

}  // extern "C"
