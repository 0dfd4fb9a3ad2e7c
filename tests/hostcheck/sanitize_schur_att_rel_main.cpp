// Stand-alone program for the sanitizers (tests/test_schur_att_rel_host.py builds it with -fsanitize=address,undefined and runs it):
// the host build of vinsat_amd/csrc/vba_schur_att_rel.h -- the closed forms of one attitude edge of vba_schur_reliability_att -- edge
// by edge as k_rel_att_edges runs it, on the cases the Python test writes (n = 2, 12, 29).  It prints leverage and w-test of every
// edge with 17 digits; the Python test compares them with the oracle.  Here the trace is also held against the dense 3x6 by 6x6 by
// 6x3 product written out in full.  Every array is a heap block of its exact size, so a read outside a 9x9 block of the last pose
// or the last edge is an error here and not a neighbour's entry.  Test infrastructure only: nothing in the product loads this.
//
// Input file (argv[1]), all float64, one record per case until the end of the file: n, sigma, J [n - 1][18], a [n - 1][3],
// state_cov [n][81], edge_cov [n - 1][81].
// Output: per case a line "case <n>", then per edge "edge <e> <leverage> <wtest>"; the last line says ok and the number of cases.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../vinsat_amd/csrc/vba_schur_att_rel.h"

using namespace vba;

// tr(sigma J Sigma6 J^T) with J and Sigma6 written out in full; *mag = the same sum over the absolute values of its terms
static double dense_leverage(double sigma, const double* J, const double* st_i, const double* ed_i, const double* st_n, double* mag) {
    double J6[3][6], Sg[6][6];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) { J6[r][c] = J[3 * r + c]; J6[r][3 + c] = J[9 + 3 * r + c]; }
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            Sg[a][b] = st_i[9 * (3 + a) + 3 + b];
            Sg[a][3 + b] = ed_i[9 * (3 + a) + 3 + b];
            Sg[3 + b][a] = ed_i[9 * (3 + a) + 3 + b];
            Sg[3 + a][3 + b] = st_n[9 * (3 + a) + 3 + b];
        }
    double tr = 0.0, ab = 0.0;
    for (int r = 0; r < 3; ++r)
        for (int a = 0; a < 6; ++a)
            for (int b = 0; b < 6; ++b) { tr += J6[r][a] * Sg[a][b] * J6[r][b]; ab += std::fabs(J6[r][a] * Sg[a][b] * J6[r][b]); }
    *mag = sigma * ab;
    return sigma * tr;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<double> in;
    double buf[512];
    size_t got;
    while ((got = std::fread(buf, 8, 512, f)) > 0) in.insert(in.end(), buf, buf + got);
    std::fclose(f);
    int fails = 0, cases = 0;
    size_t at = 0;
    while (at < in.size()) {
        if (in.size() - at < 2) { std::fprintf(stderr, "short record\n"); return 2; }
        const int n = (int)in[at];
        const double sigma = in[at + 1];
        at += 2;
        if (n < 2) { std::fprintf(stderr, "n = %d\n", n); return 2; }
        const size_t ne = (size_t)n - 1, want = ne * 18 + ne * 3 + (size_t)n * 81 + ne * 81;
        if (in.size() - at < want) { std::fprintf(stderr, "record of n = %d is short\n", n); return 2; }
        const double* p = in.data() + at;
        const std::vector<double> J(p, p + ne * 18); p += ne * 18;
        const std::vector<double> a(p, p + ne * 3); p += ne * 3;
        const std::vector<double> state(p, p + (size_t)n * 81); p += (size_t)n * 81;
        const std::vector<double> edge(p, p + ne * 81);
        at += want;
        std::printf("case %d\n", n);
        for (size_t e = 0; e < ne; ++e) {
            const double *st_i = &state[e * 81], *ed_i = &edge[e * 81], *st_n = &state[(e + 1) * 81];
            double P[9];
            schur_att_rel_P(&J[e * 18], st_i, ed_i, st_n, sigma, P);
            const double lev = schur_att_rel_leverage(P), wt = schur_att_rel_wtest(P, &a[e * 3], sigma);
            // the cross block is read once: (a, b) and (b, a) across the two poses are the same entry of edge_cov
            for (int r = 0; r < 3; ++r)
                for (int c = 3; c < 6; ++c)
                    if (schur_att_rel_sigma(st_i, ed_i, st_n, r, c) != schur_att_rel_sigma(st_i, ed_i, st_n, c, r)) {
                        std::fprintf(stderr, "edge %zu: Sigma6 (%d, %d) and (%d, %d) differ\n", e, r, c, c, r);
                        ++fails;
                    }
            double mag;
            const double dense = dense_leverage(sigma, &J[e * 18], st_i, ed_i, st_n, &mag);
            if (!(std::fabs(lev - dense) <= 1e-14 * mag)) {           // (108 terms, each rounded a few times)
                std::fprintf(stderr, "edge %zu: trace %.17g against the dense product %.17g\n", e, lev, dense);
                ++fails;
            }
            std::printf("edge %zu %.17g %.17g\n", e, lev, wt);
        }
        ++cases;
    }
    if (cases == 0) { std::fprintf(stderr, "no case in the file\n"); return 2; }
    if (fails) { std::fprintf(stderr, "%d failures\n", fails); return 1; }
    std::printf("sanitize_schur_att_rel_main ok (%d cases)\n", cases);
    return 0;
}
