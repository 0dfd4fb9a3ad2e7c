// Stand-alone driver of the closed forms of vinsat_amd/csrc/vba_schur_power_math.h for an AddressSanitizer / UBSan build on the CPU
// (tests/test_schur_power_host.py).  Ordinary and degenerate inputs -- weight 0, singular and indefinite R, q = 0, NaN; here the
// sanitizers speak, and each result must be of the kind the header promises (finite, or NaN / inf where it says so).
#include "../../vinsat_amd/csrc/vba_schur_power_math.h"
#include <cmath>
#include <cstdio>
#include <vector>
using namespace vba;

static int all_nan(const double* x, int n) {
    for (int i = 0; i < n; ++i) if (!std::isnan(x[i])) return 0;
    return 1;
}
static int all_finite(const double* x, int n) {
    for (int i = 0; i < n; ++i) if (!std::isfinite(x[i])) return 0;
    return 1;
}

int main() {
    int bad = 0;
    const double nan = std::nan("");
    // ---- sym3_mu_max
    struct E3 { double m[6]; double want; };
    const std::vector<E3> eig = {
        {{2.0, 0.0, 0.0, 3.0, 0.0, 1.0}, 3.0},                    // diagonal
        {{0.25, 0.0, 0.0, 0.25, 0.0, 0.25}, 0.25},                // a multiple of I
        {{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, 0.0},                    // zero
        {{2.0, 1.0, 0.0, 2.0, 0.0, 3.0}, 3.0},                    // two equal eigenvalues (1, 3, 3)
        {{1.0 - 1e-12, 0.0, 0.0, 1.0, 0.0, 1.0 - 2e-12}, 1.0},    // within 1e-12 of I
        {{1.0, 1.0, 1.0, 1.0, 1.0, 1.0}, 3.0},                    // rank 1
    };
    for (const E3& c : eig) {
        const double mu = sym3_mu_max(c.m);
        if (!(std::fabs(mu - c.want) <= 8e-16 * (1.0 + std::fabs(c.want)))) ++bad;
    }
    const double mnan[6] = {1.0, nan, 0.0, 1.0, 0.0, 1.0}, minf[6] = {INFINITY, 0.0, 0.0, 1.0, 0.0, 1.0};
    if (!std::isnan(sym3_mu_max(mnan))) ++bad;
    (void)sym3_mu_max(minf);                                      // (inf - inf inside: NaN or inf, no trap)
    // ---- rows
    double tu[9], tv[9], out[6];
    for (int a = 0; a < 9; ++a) { tu[a] = 0.01 * (a + 1); tv[a] = -0.02 * (a - 4); }
    schur_pow_row(0.9, 0.3, 0.05, 0.4, 1.5, -2.0, tu, tv, 17.075, out);       // ordinary
    if (!all_finite(out, 6) || !(out[0] > 0.0)) ++bad;
    schur_pow_row(0.9, 1.0, 0.0, 0.5, 1.5, -2.0, tu, tv, 17.075, out);        // singular R
    if (!all_nan(out, 6)) ++bad;
    schur_pow_row(0.9, 1.5, 0.0, 0.5, 1.5, -2.0, tu, tv, 17.075, out);        // indefinite R
    if (!all_nan(out, 6)) ++bad;
    schur_pow_row(0.9, 1.5, 0.0, 1.5, 1.5, -2.0, tu, tv, 17.075, out);        // det > 0, mu_min < 0
    if (!all_nan(out, 6)) ++bad;
    schur_pow_row(0.9, nan, 0.0, 0.5, 1.5, -2.0, tu, tv, 17.075, out);        // NaN in P
    if (!all_nan(out, 6)) ++bad;
    schur_pow_row(0.0, 0.0, 0.0, 0.0, 1.5, -2.0, tu, tv, 17.075, out);        // w = 0 (the kernel never calls it so): inf / NaN, no trap
    schur_pow_row(0.9, 0.0, 0.0, 0.0, 0.0, 0.0, tu, tv, 17.075, out);         // P = 0, r = 0
    if (!all_finite(out, 6) || out[4] != 0.0 || out[5] != 0.0) ++bad;
    // ---- priors
    double a, x;
    const double Pord[6] = {0.2, 0.01, 0.0, 0.3, -0.02, 0.1}, Pone[6] = {1.0, 0.0, 0.0, 0.5, 0.0, 0.5}, Pbig[6] = {1.5, 0.0, 0.0, 0.5, 0.0, 0.5};
    schur_pow_prior(Pord, 0.05, 17.075, a, x);
    if (!std::isfinite(a) || !std::isfinite(x) || !(a > 0.05) || !(x > 0.0)) ++bad;
    schur_pow_prior(Pone, 0.05, 17.075, a, x);                                // q = 0
    if (!std::isnan(a) || !std::isnan(x)) ++bad;
    schur_pow_prior(Pbig, 0.05, 17.075, a, x);                                // q < 0
    if (!std::isnan(a) || !std::isnan(x)) ++bad;
    schur_pow_prior(mnan, 0.05, 17.075, a, x);
    if (!std::isnan(a) || !std::isnan(x)) ++bad;
    const double G3[9] = {1e-4, 0.0, 2e-4, 0.0, -1e-4, 0.0, 3e-4, 0.0, 1e-4}, e[3] = {0.01, -0.02, 0.005};
    if (!std::isfinite(schur_pow_pull(G3, Pord, e, 400.0))) ++bad;
    if (!std::isnan(schur_pow_pull(G3, Pone, e, 400.0))) ++bad;               // det(I - P_l) = 0
    if (!std::isnan(schur_pow_pull(G3, Pbig, e, 400.0))) ++bad;               // det < 0
    if (!std::isnan(schur_pow_pull(G3, mnan, e, 400.0))) ++bad;
    if (!(schur_pow_prior_det(Pord) > 0.0) || schur_pow_prior_det(Pone) != 0.0) ++bad;
    if (bad) { std::printf("sanitize_schur_power_main: %d failures\n", bad); return 1; }
    std::printf("sanitize_schur_power_main ok\n");
    return 0;
}
