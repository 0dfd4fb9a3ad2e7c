// Stand-alone driver of the closed forms of vinsat_amd/csrc/vba_power_math.h for an AddressSanitizer / UBSan build on the CPU
// (tests/test_outlier_power_host.py).  Ordinary, coincident, rank-deficient, zero and near-singular inputs; the values are
// checked against the test's tolerances elsewhere -- here only the sanitizers speak, and the results must be what the header
// promises for each kind (finite, or NaN / inf for an R that is not positive definite).
#include "../../vinsat_amd/csrc/vba_power_math.h"
#include <cmath>
#include <cstdio>
#include <vector>
using namespace vba;

int main() {
    struct Case { double m00, m01, m11, a, b, d; bool finite; };
    const std::vector<Case> cases = {
        {2.0, 0.5, 1.0, 0.9, -0.05, 0.8, true},        // ordinary
        {1.0, 0.0, 1.0, 0.7, 0.0, 0.7, true},          // coincident eigenvalues of R and of the pair
        {4.0, 2.0, 1.0, 0.9, 0.1, 0.6, true},          // M of rank 1
        {0.0, 0.0, 0.0, 0.9, 0.1, 0.6, true},          // M = 0
        {1.0, 0.2, 3.0, 1.0, 1.0 - 1e-12, 1.0, true},  // R within 1e-12 of singular
        {1.0, 0.2, 3.0, 1.0, 2.0, 1.0, false},         // R indefinite: NaN
    };
    int bad = 0;
    for (const Case& c : cases) {
        const double lo = sym2_mu_min(c.a, c.b, c.d), hi = sym2_mu_max(c.a, c.b, c.d);
        const double mu = pair_mu_max(c.m00, c.m01, c.m11, c.a, c.b, c.d);
        double z0, z1;
        sym2_solve(c.a, c.b, c.d, 1.0, -2.0, z0, z1);
        if (!(lo <= hi)) ++bad;
        if (std::isfinite(mu) != c.finite) ++bad;
        if (c.finite && !(mu >= 0.0)) ++bad;
        if (!std::isfinite(z0) || !std::isfinite(z1)) ++bad;
        // R z = r
        if (std::fabs(c.a * z0 + c.b * z1 - 1.0) > 1e-3 || std::fabs(c.b * z0 + c.d * z1 + 2.0) > 1e-3) ++bad;
    }
    if (bad) { std::printf("sanitize_power_main: %d failures\n", bad); return 1; }
    std::printf("sanitize_power_main ok\n");
    return 0;
}
