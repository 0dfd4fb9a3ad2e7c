// Stand-alone program for the sanitizers (tests/test_schur_dyn_long_host.py builds it with -fsanitize=address,undefined and runs it):
// the host side of the long gaps of the dynamics factor of the free-landmark mode -- the plan the host makes when the factor is
// enabled (vinsat_amd/csrc/vba_schur_dyn_long.h: which edges are long, their slots, the partial count, the pool) and the scatter of
// vba_schur_dyn_math.h fed with the A = D Phi and r of a window WITH long gaps, as the Python oracle passes them in.  Every array is a
// heap block of its exact size.  Test infrastructure only: nothing in the product loads this.
//
// Input file (argv[1]), all float64: n, sigma, lamda, tol, steps [n - 1], r [n - 1][6], A [n - 1][36], then the expected S [9n][9n]
// (lower triangle, the rest zero) and g [9n] of the factor alone on a zero system with lamda on the velocity diagonal.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../vinsat_amd/csrc/vba_schur_dyn_long.h"
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
    const size_t want = 4 + ne + (size_t)ne * 6 + (size_t)ne * 36 + (size_t)N * N + N;
    if (n < 2 || in.size() != want) { std::fprintf(stderr, "file of %zu doubles, expected %zu\n", in.size(), want); return 2; }
    const double* p = in.data() + 4;
    std::vector<int> steps(ne);
    for (int e = 0; e < ne; ++e) steps[e] = (int)p[e];
    p += ne;
    const std::vector<double> r(p, p + (size_t)ne * 6); p += (size_t)ne * 6;
    const std::vector<double> A(p, p + (size_t)ne * 36); p += (size_t)ne * 36;
    const double* S_ref = p; p += (size_t)N * N;
    const double* g_ref = p;
    int fails = 0;

    // the plan: marked edges are exactly those of more than kSchurDynLongGap steps, slots follow each other without overlap, every
    // sub-chunk state and partial product of an edge lies inside its slot, and the pool is the sum of the slots for two parities
    std::vector<int> marked(steps), idx(ne), off(ne);
    const SchurDynLongPlan lp = schur_dyn_long_plan(n, marked.data(), true, idx.data(), off.data());
    int k = 0, used = 0;
    for (int e = 0; e < ne; ++e) {
        const bool is_long = steps[e] > kSchurDynLongGap;
        if (marked[e] != (is_long ? -steps[e] : steps[e])) { std::fprintf(stderr, "edge %d: %d steps marked %d\n", e, steps[e], marked[e]); ++fails; }
        if (!is_long) continue;
        if (k >= lp.nlong || idx[k] != e || off[k] != used) { std::fprintf(stderr, "edge %d: slot %d at %d, expected at %d\n", e, k, k < ne ? off[k] : -1, used); ++fails; break; }
        const LongPlan pl = long_plan(steps[e]);
        const int last = steps[e] - (pl.P - 1) * pl.L;
        if (pl.P < 1 || pl.P > 64 || pl.G > 128 || last < 1 || last > pl.L || pl.nsubL * pl.sub < pl.L || (pl.G + 15) / 16 > 8) {
            std::fprintf(stderr, "edge %d: plan L %d P %d sub %d nsubL %d G %d\n", e, pl.L, pl.P, pl.sub, pl.nsubL, pl.G); ++fails;
        }
        // what long_states writes: lane j < P records at sub-chunk (j nsubL + q), q < ceil(len_j / sub); the last index must be G - 1
        int top = -1;
        for (int j = 0; j < pl.P; ++j) {
            const int len = j < pl.P - 1 ? pl.L : last;
            top = j * pl.nsubL + (len + pl.sub - 1) / pl.sub - 1;
        }
        if (top != pl.G - 1) { std::fprintf(stderr, "edge %d: last recorded sub-chunk %d, G %d\n", e, top, pl.G); ++fails; }
        used += long_pool_states(pl);
        if (long_pool_states(pl) != 3 + pl.G + 8 * 6) ++fails;
        ++k;
    }
    if (k != lp.nlong || used != lp.pool_states || lp.npart != (ne + 255) / 256 + lp.nlong || lp.pool_bytes != (size_t)2 * used * 48) {
        std::fprintf(stderr, "plan: %d long, %d states, %d partials, %zu bytes\n", lp.nlong, lp.pool_states, lp.npart, lp.pool_bytes); ++fails;
    }
    // the serial fallback marks nothing and plans no pool
    std::vector<int> plain(steps);
    const SchurDynLongPlan sp = schur_dyn_long_plan(n, plain.data(), false, idx.data(), off.data());
    if (plain != steps || sp.nlong != 0 || sp.pool_states != 0 || sp.pool_bytes != 0 || sp.npart != (ne + 255) / 256) { std::fprintf(stderr, "serial plan marks edges\n"); ++fails; }

    // the scatter: every work item of every pose, once, on a zero system, with the long edges' A and r at their own indices
    std::vector<double> S((size_t)N * N, 0.0), g((size_t)N, 0.0);
    std::vector<int> hits((size_t)N * N, 0);
    for (int i = 0; i < n; ++i)
        for (int t = 0; t < kSchurDynItems; ++t) {
            const std::vector<double> before(S);
            schur_dyn_scatter_item(n, N, i, t, sigma, lamda, A.data(), r.data(), S.data(), g.data());
            for (size_t q = 0; q < S.size(); ++q) if (S[q] != before[q]) ++hits[q];
        }
    for (int R = 0; R < N; ++R)
        for (int C = 0; C < N; ++C) {
            const int h = hits[(size_t)R * N + C];
            if (h > 1 || (C > R && h != 0)) { std::fprintf(stderr, "entry (%d, %d) written %d times\n", R, C, h); ++fails; }
        }
    const double e_S = rel_diff(S, S_ref, S.size()), e_g = rel_diff(g, g_ref, g.size());
    std::printf("n %d: %d long edges, %d pool states, S %.2e g %.2e (tol %.1e)\n", n, lp.nlong, lp.pool_states, e_S, e_g, tol);
    if (!(e_S <= tol && e_g <= tol)) ++fails;
    if (fails) { std::fprintf(stderr, "%d failures\n", fails); return 1; }
    std::printf("sanitize_schur_dyn_long_main ok\n");
    return 0;
}
