// Stand-alone program for the sanitizers (tests/test_schur_dyn_cov_host.py builds it with -fsanitize=address,undefined and runs it):
// the host build of vinsat_amd/csrc/vba_schur_dyn_cov.h -- the index map of k_state_gather, the entries k_cov_gather reads, and the
// builder of the tile list of the selected W^T W product -- for n = 2, 12, 29, 86 and a block list whose blocks straddle tile edges.
// Every array is a heap block of its exact size, so an entry outside the N x N system or a tile outside the list's range is an
// error here.  Test infrastructure only: nothing in the product loads this.
//
// It asserts: every entry the gathers read lies in a listed tile; every listed tile is read by some entry; every read is at or below
// the diagonal (the only triangle the product forms); the map agrees with u(i, c) written out here a second time.
#include <cstdio>
#include <vector>

#include "../../vinsat_amd/csrc/vba_schur_dyn_cov.h"

using namespace vba;

static const int kTile = 64;

static int check(int n) {
    const int N = 9 * n, nbu = (N + kTile - 1) / kTile;
    // block list: every diagonal block, the neighbours at distance 1 and 2, and every seventh pose against pose 0 and the pose
    // ten before it (blocks far from the diagonal; with 6 rows per pose and tiles of 64 most of them straddle a tile edge)
    std::vector<int> bi, bj;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j)
            if (i - j <= 2 || (i % 7 == 0 && (j == 0 || j == i - 10))) { bi.push_back(i); bj.push_back(j); }
    const int nblk = (int)bi.size();
    std::vector<int> tiles;
    schur_dyn_cov_tiles(n, nblk, bi.data(), bj.data(), kTile, tiles);
    int fails = 0;
    if (tiles.size() % 2 != 0 || tiles.size() / 2 > (size_t)nbu * (nbu + 1) / 2) { std::fprintf(stderr, "n %d: %zu ints in the tile list\n", n, tiles.size()); return 1; }
    std::vector<char> listed((size_t)nbu * nbu, 0), used((size_t)nbu * nbu, 0);
    int prev = -1;
    for (size_t k = 0; k < tiles.size(); k += 2) {
        const int I = tiles[k], J = tiles[k + 1];
        if (I < 0 || I >= nbu || J < 0 || J > I) { std::fprintf(stderr, "n %d: tile (%d, %d) outside the lower triangle of %d\n", n, I, J, nbu); return 1; }
        const int q = I * (I + 1) / 2 + J;
        if (q <= prev) { std::fprintf(stderr, "n %d: tile (%d, %d) out of order or listed twice\n", n, I, J); ++fails; }
        prev = q;
        listed[(size_t)I * nbu + J] = 1;
    }
    std::vector<char> seen((size_t)N * N, 0);      // (exact size: an entry outside the system is the sanitizer's to report)
    auto read = [&](SchurEntry s, const char* what, int b) {
        if (s.r < 0 || s.r >= N || s.c < 0 || s.c > s.r) { std::fprintf(stderr, "n %d: %s %d reads (%d, %d)\n", n, what, b, s.r, s.c); ++fails; return; }
        seen[(size_t)s.r * N + s.c] = 1;
        const size_t tl = (size_t)(s.r / kTile) * nbu + s.c / kTile;
        if (!listed[tl]) { std::fprintf(stderr, "n %d: %s %d reads (%d, %d) in an unlisted tile\n", n, what, b, s.r, s.c); ++fails; }
        used[tl] = 1;
    };
    // k_state_gather, entry by entry as its threads run, against the map written out again
    for (int e = 0; e < 81 * (2 * n - 1); ++e) {
        const SchurEntry s = schur_state_gather_entry(n, e);
        read(s, "state entry", e);
        const int b = e / 81, a = (e % 81) / 9, c = e % 9, i = b < n ? b : b - n, j = b < n ? b : b - n + 1;
        const int p = a < 6 ? 6 * i + a : 6 * n + 3 * i + (a - 6), q = c < 6 ? 6 * j + c : 6 * n + 3 * j + (c - 6);
        if (s.r != (p > q ? p : q) || s.c != (p > q ? q : p)) { std::fprintf(stderr, "n %d: entry %d maps to (%d, %d), expected (%d, %d)\n", n, e, s.r, s.c, p, q); ++fails; }
    }
    // the pose part of a state block reads what k_cov_gather reads for the diagonal block
    for (int i = 0; i < n; ++i)
        for (int a = 0; a < 6; ++a)
            for (int c = 0; c < 6; ++c) {
                const SchurEntry s = schur_state_entry(n, i, a, i, c), p = schur_pair_entry(i, a, i, c);
                if (s.r != p.r || s.c != p.c) { std::fprintf(stderr, "n %d: pose %d (%d, %d): state and pair gathers read different entries\n", n, i, a, c); ++fails; }
            }
    for (int b = 0; b < nblk; ++b)
        for (int a = 0; a < 6; ++a)
            for (int c = 0; c < 6; ++c) read(schur_pair_entry(bi[b], a, bj[b], c), "block", b);
    int nlisted = 0;
    for (size_t k = 0; k < listed.size(); ++k) {
        nlisted += listed[k];
        if (listed[k] && !used[k]) { std::fprintf(stderr, "n %d: tile (%zu, %zu) is listed and never read\n", n, k / nbu, k % nbu); ++fails; }
    }
    // a state block and its two neighbours: the mirror entries of a state block read one stored entry
    for (int i = 0; i < n; ++i)
        for (int a = 0; a < 9; ++a)
            for (int c = 0; c < a; ++c) {
                const SchurEntry s = schur_state_entry(n, i, a, i, c), t = schur_state_entry(n, i, c, i, a);
                if (s.r != t.r || s.c != t.c) { std::fprintf(stderr, "n %d: pose %d (%d, %d) and its mirror read different entries\n", n, i, a, c); ++fails; }
            }
    std::printf("n %d: N %d, %d tiles per side, %d of %d listed, %d blocks\n", n, N, nbu, nlisted, nbu * (nbu + 1) / 2, nblk);
    return fails;
}

int main() {
    int fails = 0;
    const int ns[] = {2, 12, 29, 86};
    for (int n : ns) fails += check(n);
    if (fails) { std::fprintf(stderr, "%d failures\n", fails); return 1; }
    std::printf("sanitize_schur_dyn_cov_main ok\n");
    return 0;
}
