// Stand-alone program for the sanitizers (tests/test_schur_prior_host.py builds it with -fsanitize=address,undefined and runs it):
// the host build of vinsat_amd/csrc/vba_schur_prior_math.h -- the per-prior body of the state prior factor of the free-landmark mode,
// the scatter's work items, and the 9x9 congruence and Cholesky inverse of the window hand-off -- on a small case the Python test
// writes, against the numbers the Python oracle passes in.  Every array is a heap block of its exact size, so an index of the scatter
// outside the reduced system is an error here and not a neighbour's entry.  Test infrastructure only: nothing in the product loads this.
//
// Input file (argv[1]), all float64: n, count, tol, steps, states [n][10], idx [count], anchors [count][10], infos [count][81], then the
// expected e [count][9], J [count][9], cost (sum e^T Lambda e), S [9n][9n] (lower triangle, the rest zero) and g [9n] of the factor alone
// on a zero system; then the hand-off: c [4], noise [3], Phi [36], Sigma [81], and the expected info [81].
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../vinsat_amd/csrc/vba_schur_prior_math.h"

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
    const int n = (int)in[0], count = (int)in[1], steps = (int)in[3];
    const double tol = in[2];
    const int N = 9 * n;
    const size_t nc = (size_t)count;
    const size_t want = 4 + (size_t)n * 10 + nc + nc * 10 + nc * 81 + nc * 9 + nc * 9 + 1 + (size_t)N * N + N + 4 + 3 + 36 + 81 + 81;
    if (n < 1 || count < 1 || count > n || in.size() != want) { std::fprintf(stderr, "file of %zu doubles, expected %zu\n", in.size(), want); return 2; }
    const double* p = in.data() + 4;
    const std::vector<double> states(p, p + (size_t)n * 10); p += (size_t)n * 10;
    std::vector<int> idx(nc);
    for (size_t k = 0; k < nc; ++k) idx[k] = (int)*p++;
    const std::vector<double> anchors(p, p + nc * 10); p += nc * 10;
    const std::vector<double> infos(p, p + nc * 81); p += nc * 81;
    const double* e_ref = p; p += nc * 9;
    const double* J_ref = p; p += nc * 9;
    const double cost_ref = *p++;
    const double* S_ref = p; p += (size_t)N * N;
    const double* g_ref = p; p += N;
    const std::vector<double> c(p, p + 4); p += 4;
    const std::vector<double> noise(p, p + 3); p += 3;
    const std::vector<double> Phi(p, p + 36); p += 36;
    const std::vector<double> Sigma(p, p + 81); p += 81;
    const double* info_ref = p;

    // the per-prior body as the terms kernel runs it; the residual-only body of the cost kernel must give the same bits
    std::vector<double> e(nc * 9), J(nc * 9), LF(nc * 81), Le(nc * 9);
    double cost = 0.0;
    int fails = 0, negative = 0;
    for (int k = 0; k < count; ++k) {
        const double *st = &states[(size_t)idx[k] * 10], *an = &anchors[(size_t)k * 10], *L = &infos[(size_t)k * 81];
        const double share = schur_prior_terms(st, an, L, &e[(size_t)k * 9], &J[(size_t)k * 9], &LF[(size_t)k * 81], &Le[(size_t)k * 9]);
        std::vector<double> w(4), e2(9), Le2(9);
        schur_prior_residual(st, an, w.data(), e2.data());
        const double share2 = schur_prior_cost(L, e2.data(), Le2.data());
        if (share2 != share) { std::fprintf(stderr, "prior %d: the residual-only body gives other bits\n", k); ++fails; }
        if (w[3] < 0.0) ++negative;
        cost += share;
    }
    // the scatter: every work item of every prior, once, on a zero system
    std::vector<double> S((size_t)N * N, 0.0), g((size_t)N, 0.0);
    std::vector<int> hits((size_t)N * N, 0);
    for (int k = 0; k < count; ++k)
        for (int t = 0; t < kSchurPriorItems; ++t) {
            const std::vector<double> before(S);
            schur_prior_scatter_item(n, N, idx[k], t, &J[(size_t)k * 9], &LF[(size_t)k * 81], &Le[(size_t)k * 9], S.data(), g.data());
            for (size_t q = 0; q < S.size(); ++q) if (S[q] != before[q]) ++hits[q];
        }
    for (int R = 0; R < N; ++R)
        for (int C = 0; C < N; ++C) {
            const int h = hits[(size_t)R * N + C];
            if (h > 1 || (C > R && h != 0)) { std::fprintf(stderr, "entry (%d, %d) written %d times\n", R, C, h); ++fails; }
        }
    // the hand-off's algebra, every work array a heap block of its own
    std::vector<double> R(9), G(81), T(81), Sp(81), Lw(81), Ww(81), info(81);
    schur_handoff_rotation(c.data(), R.data());
    schur_handoff_transition(Phi.data(), R.data(), G.data());
    schur_handoff_congruence(G.data(), Sigma.data(), steps, noise.data(), T.data(), Sp.data());
    const bool ok = schur_handoff_cholinv(Sp.data(), Lw.data(), Ww.data(), info.data());
    if (!ok) { std::fprintf(stderr, "the propagated covariance is not positive definite\n"); ++fails; }
    for (int a = 0; a < 9; ++a)
        for (int b = 0; b < a; ++b)
            if (info[9 * a + b] != info[9 * b + a] || Sp[9 * a + b] != Sp[9 * b + a]) { std::fprintf(stderr, "(%d, %d) is not mirrored\n", a, b); ++fails; }
    double e_i = 0.0;       // in sigmas of the information matrix
    for (int a = 0; a < 9; ++a)
        for (int b = 0; b < 9; ++b)
            e_i = std::fmax(e_i, std::fabs(info[9 * a + b] - info_ref[9 * a + b]) / std::sqrt(info_ref[9 * a + a] * info_ref[9 * b + b]));
    // a matrix that is not positive definite is refused and leaves the output alone
    std::vector<double> bad(Sp), keep(info);
    bad[9 * 4 + 4] = -1.0;
    if (schur_handoff_cholinv(bad.data(), Lw.data(), Ww.data(), info.data()) || info != keep) { std::fprintf(stderr, "an indefinite matrix was inverted\n"); ++fails; }
    const double e_e = rel_diff(e, e_ref, e.size()), e_J = rel_diff(J, J_ref, J.size()), e_S = rel_diff(S, S_ref, S.size()),
                 e_g = rel_diff(g, g_ref, g.size()), e_c = std::fabs(cost - cost_ref) / std::fabs(cost_ref);
    std::printf("n %d, %d priors (%d with d < 0): e %.2e J %.2e S %.2e g %.2e cost %.2e handoff info %.2e (tol %.1e)\n", n, count, negative, e_e, e_J, e_S,
                e_g, e_c, e_i, tol);
    if (!(e_e <= tol && e_J <= tol && e_S <= tol && e_g <= tol && e_c <= tol && e_i <= 1e-10)) ++fails;
    if (fails) { std::fprintf(stderr, "%d failures\n", fails); return 1; }
    std::printf("sanitize_schur_prior_main ok\n");
    return 0;
}
