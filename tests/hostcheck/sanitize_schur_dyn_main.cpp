// Stand-alone program for the sanitizers (tests/test_schur_dyn_host.py builds it with -fsanitize=address,undefined and runs it):
// the host build of vinsat_amd/csrc/vba_schur_dyn_math.h -- the per-edge body of the dynamics factor of the free-landmark mode and
// the scatter's work items -- on a small case the Python test writes, against the numbers the Python oracle passes in.  Every array
// is a heap block of its exact size, so an index of the scatter outside the reduced system is an error here and not a neighbour's
// entry.  Test infrastructure only: nothing in the product loads this.
//
// Input file (argv[1]), all float64: n, sigma, lamda, tol, states [n][10], steps [n - 1], then the expected r [n - 1][6],
// A = D Phi [n - 1][36], cost (sigma sum |r|^2), S [9n][9n] (lower triangle, the rest zero) and g [9n] of the factor alone on a
// zero system with lamda on the velocity diagonal.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../vinsat_amd/csrc/vba_schur_dyn_math.h"

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
    if (in.size() < 4) { std::fprintf(stderr, "short file\n"); return 2; }
    const int n = (int)in[0];
    const double sigma = in[1], lamda = in[2], tol = in[3];
    const int N = 9 * n, ne = n - 1;
    const size_t want = 4 + (size_t)n * 10 + ne + (size_t)ne * 6 + (size_t)ne * 36 + 1 + (size_t)N * N + N;
    if (n < 2 || in.size() != want) { std::fprintf(stderr, "file of %zu doubles, expected %zu\n", in.size(), want); return 2; }
    const double* p = in.data() + 4;
    const std::vector<double> states(p, p + (size_t)n * 10); p += (size_t)n * 10;
    std::vector<int> steps(ne);
    for (int e = 0; e < ne; ++e) steps[e] = (int)p[e];
    p += ne;
    const double* r_ref = p; p += (size_t)ne * 6;
    const double* A_ref = p; p += (size_t)ne * 36;
    const double cost_ref = *p++;
    const double* S_ref = p; p += (size_t)N * N;
    const double* g_ref = p;

    // the per-edge body, column by column as the kernel's lanes run it; the prediction must not depend on the column
    std::vector<double> r((size_t)ne * 6), A((size_t)ne * 36);
    double cost = 0.0;
    int fails = 0;
    for (int e = 0; e < ne; ++e) {
        if (steps[e] < 1 || steps[e] > kSchurDynMaxGap) { std::fprintf(stderr, "edge %d: %d steps\n", e, steps[e]); return 2; }
        double xhat0[6];
        for (int c = 0; c < 6; ++c) {
            double xhat[6], col[6];
            schur_dyn_edge_column(&states[(size_t)e * 10], steps[e], c, xhat, col);
            for (int k = 0; k < 6; ++k) {
                A[(size_t)e * 36 + 6 * k + c] = col[k];
                if (c == 0) xhat0[k] = xhat[k];
                else if (xhat[k] != xhat0[k]) { std::fprintf(stderr, "edge %d: the prediction depends on the tangent column\n", e); ++fails; }
            }
        }
        double xp[6], r2[6];
        schur_dyn_predict(&states[(size_t)e * 10], steps[e], xp);
        for (int k = 0; k < 6; ++k)
            if (xp[k] != xhat0[k]) { std::fprintf(stderr, "edge %d: the residual-only propagation gives other bits\n", e); ++fails; }
        cost += sigma * schur_dyn_residual(xhat0, &states[(size_t)(e + 1) * 10], &r[(size_t)e * 6]);
        (void)schur_dyn_residual(xp, &states[(size_t)(e + 1) * 10], r2);
    }
    // the scatter: every work item of every pose, once, on a zero system
    std::vector<double> S((size_t)N * N, 0.0), g((size_t)N, 0.0);
    std::vector<int> hits((size_t)N * N, 0);
    for (int i = 0; i < n; ++i)
        for (int t = 0; t < kSchurDynItems; ++t) {
            const std::vector<double> before(S);
            schur_dyn_scatter_item(n, N, i, t, sigma, lamda, A.data(), r.data(), S.data(), g.data());
            for (size_t k = 0; k < S.size(); ++k) if (S[k] != before[k]) ++hits[k];
        }
    for (int R = 0; R < N; ++R)
        for (int C = 0; C < N; ++C) {
            const int h = hits[(size_t)R * N + C];
            if (h > 1 || (C > R && h != 0)) { std::fprintf(stderr, "entry (%d, %d) written %d times\n", R, C, h); ++fails; }
        }
    const double e_r = rel_diff(r, r_ref, r.size()), e_A = rel_diff(A, A_ref, A.size()), e_S = rel_diff(S, S_ref, S.size()),
                 e_g = rel_diff(g, g_ref, g.size()), e_c = std::fabs(cost - cost_ref) / std::fabs(cost_ref);
    std::printf("n %d: r %.2e A %.2e S %.2e g %.2e cost %.2e (tol %.1e)\n", n, e_r, e_A, e_S, e_g, e_c, tol);
    if (!(e_r <= tol && e_A <= tol && e_S <= tol && e_g <= tol && e_c <= tol)) ++fails;
    if (fails) { std::fprintf(stderr, "%d failures\n", fails); return 1; }
    std::printf("sanitize_schur_dyn_main ok\n");
    return 0;
}
