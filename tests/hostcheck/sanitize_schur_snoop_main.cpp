// Stand-alone driver of the decision rule of vba_schur_snoop (vinsat_amd/csrc/vba_schur_snoop_pick.h through
// hostcheck_schur_snoop.cpp) for an AddressSanitizer / UBSan build on the CPU (tests/test_schur_snoop_host.py): a few hundred
// seeded small problems -- poses and landmarks without rows, tracks of one row, zero weights, NaN and tied tests, every min_rows
// around a pose's count -- in arrays of exactly their size on the heap, so an index outside a segment is the sanitizer's to
// report.  Checked here: all 16 lanes of every pose agree, a row is never rejected twice, a rejected landmark has no weighted row
// left, a non-finite critical value and info != 0 reject nothing.
#include "hostcheck_schur_snoop.cpp"

#include <algorithm>
#include <cstdio>

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static unsigned rnd(unsigned mod) {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(g_state >> 33) % mod;
}

static int one_problem(int n, int L, int info, double crit, int scaled, double s0sq) {
    std::vector<int> rp, rl;
    for (int l = 0; l < L; ++l) {
        const int t = (int)rnd(7);                          // track length 0 .. 6, distinct poses in ascending order
        std::vector<int> poses;
        for (int i = 0; i < n && (int)poses.size() < t; ++i)
            if (rnd(2)) poses.push_back(i);
        for (int i : poses) { rp.push_back(i); rl.push_back(l); }
    }
    const int m = (int)rp.size();
    if (m == 0) return 0;
    std::vector<int> lm_ptr(L + 1, 0), pose_ptr(n + 1, 0), pose_rows(m);
    for (int k = 0; k < m; ++k) { ++lm_ptr[rl[k] + 1]; ++pose_ptr[rp[k] + 1]; }
    for (int l = 0; l < L; ++l) lm_ptr[l + 1] += lm_ptr[l];
    for (int i = 0; i < n; ++i) pose_ptr[i + 1] += pose_ptr[i];
    std::vector<int> fill(pose_ptr.begin(), pose_ptr.end() - 1);
    for (int k = 0; k < m; ++k) pose_rows[fill[rp[k]]++] = k;
    std::vector<double> w(m), wt(m), lmwt(L);
    for (int k = 0; k < m; ++k) {
        w[k] = rnd(8) == 0 ? 0.0 : 0.95;
        wt[k] = rnd(10) == 0 ? __builtin_nan("") : (double)rnd(6);         // few distinct values: ties everywhere
    }
    for (int l = 0; l < L; ++l) lmwt[l] = rnd(10) == 0 ? __builtin_nan("") : (double)rnd(6);
    std::vector<unsigned char> own(m), rej(L), via(m);
    int bad = 0;
    for (int min_rows = 0; min_rows <= 8; ++min_rows) {
        double used = 0.0;
        const int agree = hc_schur_snoop(n, L, m, lm_ptr.data(), rp.data(), rl.data(), pose_ptr.data(), pose_rows.data(), w.data(), wt.data(),
                                         lmwt.data(), s0sq, info, crit, scaled, min_rows, (int)rnd(4), own.data(), rej.data(), via.data(), &used);
        if (!agree) ++bad;
        int any = 0;
        for (int k = 0; k < m; ++k) {
            if (own[k] && via[k]) ++bad;
            if ((own[k] || via[k]) && !(w[k] > 0.0)) ++bad;
            if (w[k] > 0.0 && rej[rl[k]] && !via[k]) ++bad;
            any += own[k] + via[k];
        }
        for (int i = 0; i < n; ++i) {
            int lost = 0;
            for (int r = pose_ptr[i]; r < pose_ptr[i + 1]; ++r) lost += own[pose_rows[r]];
            if (lost > 1) ++bad;
        }
        if ((info != 0 || !(used - used == 0.0)) && any != 0) ++bad;
    }
    return bad;
}

int main() {
    int bad = 0;
    for (int rep = 0; rep < 300; ++rep) {
        const int n = 1 + (int)rnd(20), L = 1 + (int)rnd(40);
        const int kind = rep % 6;
        const double nan = __builtin_nan(""), inf = __builtin_inf();
        if (kind == 0) bad += one_problem(n, L, 0, 2.0, 0, 1.0);
        if (kind == 1) bad += one_problem(n, L, 0, 1.0, 1, 4.0);
        if (kind == 2) bad += one_problem(n, L, 0, 1.0, 1, nan);
        if (kind == 3) bad += one_problem(n, L, 595, 1.0, 1, 4.0);
        if (kind == 4) bad += one_problem(n, L, 0, inf, 0, 1.0);
        if (kind == 5) bad += one_problem(n, L, 0, 0.0, 0, 1.0);
    }
    if (bad) { std::printf("sanitize_schur_snoop_main: %d failures\n", bad); return 1; }
    std::printf("sanitize_schur_snoop_main ok\n");
    return 0;
}
