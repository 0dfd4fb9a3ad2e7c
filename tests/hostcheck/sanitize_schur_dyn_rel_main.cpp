// Stand-alone program for the sanitizers (tests/test_schur_dyn_rel_host.py builds it with -fsanitize=address,undefined and runs it):
// the host build of vinsat_amd/csrc/vba_schur_dyn_rel.h -- the closed form of the edge leverage of vba_schur_reliability_dyn -- lane
// by lane as k_rel_edges runs it, on the cases the Python test writes (n = 2, 12, 29), against the leverages the Python oracle passes
// in and against the dense 6x12 by 12x12 by 12x6 product formed here.  Every array is a heap block of its exact size, so a read
// outside a 9x9 block of the last pose or the last edge is an error here and not a neighbour's entry.  Test infrastructure only:
// nothing in the product loads this.
//
// Input file (argv[1]), all float64, one record per case until the end of the file: n, sigma, tol, A = D Phi [n - 1][36],
// state_cov [n][81], edge_cov [n - 1][81], the expected edge_leverage [n - 1].
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../vinsat_amd/csrc/vba_schur_dyn_rel.h"

using namespace vba;

// tr(sigma J Sigma12 J^T) with J and Sigma12 written out in full
static double dense_leverage(double sigma, const double* A, const double* st_i, const double* ed_i, const double* st_n) {
    static const int comp[6] = {0, 1, 2, 6, 7, 8};
    double J[6][12] = {}, Sg[12][12];
    for (int r = 0; r < 6; ++r) {
        for (int c = 0; c < 6; ++c) J[r][c] = A[6 * r + c];
        J[r][6 + r] = -(r < 3 ? 1.0 : kVelCoeff);
    }
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) {
            Sg[a][b] = st_i[9 * comp[a] + comp[b]];
            Sg[a][6 + b] = ed_i[9 * comp[a] + comp[b]];
            Sg[6 + b][a] = ed_i[9 * comp[a] + comp[b]];
            Sg[6 + a][6 + b] = st_n[9 * comp[a] + comp[b]];
        }
    double tr = 0.0;
    for (int r = 0; r < 6; ++r)
        for (int a = 0; a < 12; ++a)
            for (int b = 0; b < 12; ++b) tr += J[r][a] * Sg[a][b] * J[r][b];
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
        if (in.size() - at < 3) { std::fprintf(stderr, "short record\n"); return 2; }
        const int n = (int)in[at];
        const double sigma = in[at + 1], tol = in[at + 2];
        at += 3;
        if (n < 2) { std::fprintf(stderr, "n = %d\n", n); return 2; }
        const size_t ne = (size_t)n - 1, want = ne * 36 + (size_t)n * 81 + ne * 81 + ne;
        if (in.size() - at < want) { std::fprintf(stderr, "record of n = %d is short\n", n); return 2; }
        const double* p = in.data() + at;
        const std::vector<double> A(p, p + ne * 36); p += ne * 36;
        const std::vector<double> state(p, p + (size_t)n * 81); p += (size_t)n * 81;
        const std::vector<double> edge(p, p + ne * 81); p += ne * 81;
        const std::vector<double> ref(p, p + ne);
        at += want;
        double e_ref = 0.0, e_dense = 0.0, lo = 1e300, hi = -1e300;
        for (size_t e = 0; e < ne; ++e) {
            double diag[6];
            for (int c = 0; c < 6; ++c)     // lane c of the edge's group
                diag[c] = schur_dyn_rel_edge_diag(&A[e * 36], &state[e * 81], &edge[e * 81], &state[(e + 1) * 81], c);
            const double lev = schur_dyn_rel_edge_leverage(sigma, diag);
            const double dense = dense_leverage(sigma, &A[e * 36], &state[e * 81], &edge[e * 81], &state[(e + 1) * 81]);
            // the cross block is read once: (a, b) and (b, a) across the two poses are the same entry of edge_cov
            for (int a = 0; a < 6; ++a)
                for (int b = 6; b < 12; ++b)
                    if (schur_dyn_rel_sigma(&state[e * 81], &edge[e * 81], &state[(e + 1) * 81], a, b) !=
                        schur_dyn_rel_sigma(&state[e * 81], &edge[e * 81], &state[(e + 1) * 81], b, a)) {
                        std::fprintf(stderr, "edge %zu: Sigma12 (%d, %d) and (%d, %d) differ\n", e, a, b, b, a);
                        ++fails;
                    }
            e_ref = std::fmax(e_ref, std::fabs(lev - ref[e]));
            e_dense = std::fmax(e_dense, std::fabs(lev - dense));
            lo = std::fmin(lo, lev); hi = std::fmax(hi, lev);
        }
        // relative to the largest entry of the family, as the Python side measures
        double top = 0.0;
        for (size_t e = 0; e < ne; ++e) top = std::fmax(top, std::fabs(ref[e]));
        std::printf("n %d: against the oracle %.2e, against the dense product %.2e (tol %.1e), leverages %.6f .. %.6f\n", n, e_ref / top,
                    e_dense / top, tol, lo, hi);
        if (!(e_ref / top <= tol && e_dense / top <= tol)) ++fails;
        ++cases;
    }
    if (cases == 0) { std::fprintf(stderr, "no case in the file\n"); return 2; }
    if (fails) { std::fprintf(stderr, "%d failures\n", fails); return 1; }
    std::printf("sanitize_schur_dyn_rel_main ok (%d cases)\n", cases);
    return 0;
}
