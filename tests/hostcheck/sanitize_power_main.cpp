// Stand-alone driver of the closed forms of vinsat_amd/csrc/vba_power_math.h for an AddressSanitizer / UBSan build on the CPU
// (tests/test_outlier_power_host.py).  Ordinary, coincident, rank-deficient, zero and near-singular inputs; the values are
// checked against the test's tolerances elsewhere -- here only the sanitizers speak, and the results must be what the header
// promises for each kind (finite, or NaN / inf for an R that is not positive definite).  And the scratch layouts of the two row-pass
// queries (vba_query_layout.h) at the smallest shape and at one that is no multiple of anything.
#include "../../vinsat_amd/csrc/vba_power_math.h"
#include "../../vinsat_amd/csrc/vba_query_layout.h"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace vba;

// The scratch layouts of the row-pass queries (vba_query_layout.h), counted and then placed over a block of the counted size:
// every buffer starts on a multiple of 256 bytes behind the one in front of it and the last one ends inside the block.  Each
// buffer is written over its whole length, so an overrun is the sanitizer's to report.
struct Span { void* p; size_t bytes; };
static int check_spans(char* base, size_t total, const std::vector<Span>& spans) {
    int bad = 0;
    const char* end_prev = base;
    for (const Span& sp : spans) {
        const char* p = static_cast<const char*>(sp.p);
        if (p < end_prev || (reinterpret_cast<uintptr_t>(p) & 255u) != 0 || p + sp.bytes > base + total) ++bad;
        else std::memset(sp.p, 0x5a, sp.bytes);
        end_prev = p + sp.bytes;
    }
    return bad;
}
static int check_layouts(size_t W, size_t N, size_t M) {
    int bad = 0;
    {
        Carver count;
        rel_layout(count, W, N, M);
        char* base = static_cast<char*>(std::aligned_alloc(256, count.total()));
        Carver place{base};
        const RelBufs b = rel_layout(place, W, N, M);
        if (place.total() != count.total()) ++bad;
        bad += check_spans(base, count.total(), {{b.lev, W * M * 8}, {b.wt, W * M * 8}, {b.perm, W * M * 4}, {b.pstat, W * N * 3 * 8}});
        std::free(base);
    }
    {
        Carver count;
        pow_layout(count, W, N, M);
        char* base = static_cast<char*>(std::aligned_alloc(256, count.total()));
        Carver place{base};
        const PowBufs b = pow_layout(place, W, N, M);
        if (place.total() != count.total()) ++bad;
        bad += check_spans(base, count.total(), {{b.row[0], W * M * 8}, {b.row[1], W * M * 8}, {b.row[2], W * M * 8}, {b.row[3], W * M * 8},
                                                 {b.pfit, W * N * 4 * 8}, {b.paux, W * N * 2 * 8}, {b.fit, W * 8 * 8}});
        std::free(base);
    }
    return bad;
}

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
    bad += check_layouts(1, 2, 3) + check_layouts(3, 17, 67);
    if (bad) { std::printf("sanitize_power_main: %d failures\n", bad); return 1; }
    std::printf("sanitize_power_main ok\n");
    return 0;
}
