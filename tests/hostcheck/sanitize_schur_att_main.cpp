// Stand-alone program for the sanitizers (tests/test_schur_att_host.py builds it with -fsanitize=address,undefined and runs it):
// the host build of vinsat_amd/csrc/vba_schur_att_math.h -- the per-edge body of the Gauss-Newton attitude factor of the
// free-landmark mode and the scatter's work items -- on a small case the Python test writes, against the numbers the Python oracle
// passes in.  Every array is a heap block of its exact size, so an index of the scatter outside the reduced system is an error here
// and not a neighbour's entry.  Test infrastructure only: nothing in the product loads this.
//
// Input file (argv[1]), all float64: n, sigma, tol, states [n][10], cumrot [n - 1][4], then the expected a [n - 1][3],
// J [n - 1][2][3][3], cost (sigma sum |a|^2), S [9n][9n] (lower triangle, the rest zero) and g [9n] of the factor alone on a zero system.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../vinsat_amd/csrc/vba_schur_att_math.h"

using namespace vba;

static double rel_diff(const std::vector<double>& a, const double* b, size_t count) {
    double d = 0.0, m = 0.0;
    for (size_t k = 0; k < count; ++k) {
        d = std::fmax(d, std::fabs(a[k] - b[k]));
        m = std::fmax(m, std::fabs(b[k]));
    }
    return m > 0.0 ? d / m : d;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s case.bin\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<double> in;
    double buf[512];
    size_t got;
    while ((got = std::fread(buf, 8, 512, f)) > 0) in.insert(in.end(), buf, buf + got);
    std::fclose(f);
    if (in.size() < 3) { std::fprintf(stderr, "short file\n"); return 2; }
    const int n = (int)in[0];
    const double sigma = in[1], tol = in[2];
    const int N = 9 * n, ne = n - 1;
    const size_t want = 3 + (size_t)n * 10 + (size_t)ne * 4 + (size_t)ne * 3 + (size_t)ne * kSchurAttJ + 1 + (size_t)N * N + N;
    if (n < 2 || in.size() != want) { std::fprintf(stderr, "file of %zu doubles, expected %zu\n", in.size(), want); return 2; }
    const double* p = in.data() + 3;
    const std::vector<double> states(p, p + (size_t)n * 10); p += (size_t)n * 10;
    const std::vector<double> cumrot(p, p + (size_t)ne * 4); p += (size_t)ne * 4;
    const double* a_ref = p; p += (size_t)ne * 3;
    const double* J_ref = p; p += (size_t)ne * kSchurAttJ;
    const double cost_ref = *p++;
    const double* S_ref = p; p += (size_t)N * N;
    const double* g_ref = p;

    // the per-edge body as the edge kernel runs it; the residual-only body of the cost kernel must give the same bits
    std::vector<double> a((size_t)ne * 3), J((size_t)ne * kSchurAttJ);
    double cost = 0.0;
    int fails = 0, negative = 0;
    for (int e = 0; e < ne; ++e) {
        const double *qi = &states[(size_t)e * 10 + 3], *qn = &states[(size_t)(e + 1) * 10 + 3], *c = &cumrot[(size_t)e * 4];
        const double n2 = schur_att_edge(qi, c, qn, &a[(size_t)e * 3], &J[(size_t)e * kSchurAttJ]);
        double w[4], a2[3];
        const double n2c = schur_att_residual(qi, c, qn, w, a2);
        if (n2c != n2 || a2[0] != a[(size_t)e * 3] || a2[1] != a[(size_t)e * 3 + 1] || a2[2] != a[(size_t)e * 3 + 2]) {
            std::fprintf(stderr, "edge %d: the residual-only body gives other bits\n", e);
            ++fails;
        }
        if (w[3] < 0.0) ++negative;
        cost += sigma * n2;
    }
    // the scatter: every work item of every pose, once, on a zero system
    std::vector<double> S((size_t)N * N, 0.0), g((size_t)N, 0.0);
    std::vector<int> hits((size_t)N * N, 0);
    for (int i = 0; i < n; ++i)
        for (int t = 0; t < kSchurAttItems; ++t) {
            const std::vector<double> before(S);
            schur_att_scatter_item(n, N, i, t, sigma, J.data(), a.data(), S.data(), g.data());
            for (size_t k = 0; k < S.size(); ++k) if (S[k] != before[k]) ++hits[k];
        }
    for (int R = 0; R < N; ++R)
        for (int C = 0; C < N; ++C) {
            const int h = hits[(size_t)R * N + C];
            if (h > 1 || (C > R && h != 0)) { std::fprintf(stderr, "entry (%d, %d) written %d times\n", R, C, h); ++fails; }
        }
    const double e_a = rel_diff(a, a_ref, a.size()), e_J = rel_diff(J, J_ref, J.size()), e_S = rel_diff(S, S_ref, S.size()),
                 e_g = rel_diff(g, g_ref, g.size()), e_c = std::fabs(cost - cost_ref) / std::fabs(cost_ref);
    std::printf("n %d (%d edges with d < 0): a %.2e J %.2e S %.2e g %.2e cost %.2e (tol %.1e)\n", n, negative, e_a, e_J, e_S, e_g, e_c, tol);
    if (!(e_a <= tol && e_J <= tol && e_S <= tol && e_g <= tol && e_c <= tol)) ++fails;
    if (fails) { std::fprintf(stderr, "%d failures\n", fails); return 1; }
    std::printf("sanitize_schur_att_main ok\n");
    return 0;
}
