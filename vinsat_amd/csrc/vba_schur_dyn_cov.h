// vba_schur_dyn_cov.h -- the index arithmetic of vba_schur_covariance_dyn (vba_schur_cov.hip): which entry of the stored lower
// triangle of S9^-1 every output entry reads, as host/device functions, and the host-side list of the tiles those entries lie in.
// k_state_gather reads through the map and the tile list is built from it, so the selected product (k_syrk_wtw_sel) computes every
// tile a gather reads and the CPU test-suite can compile and check both (tests/hostcheck/sanitize_schur_dyn_cov_main.cpp).  Internal.
//
// Unknowns of the reduced system of a handle with the dynamics factor: [6 n pose | 3 n velocity] (vba_schur_dyn_math.h).  Component
// c of the 9-vector [dp, dtheta, dv] of pose i -- the coordinates of vba_covariance -- is unknown 6 i + c for c < 6 and
// 6 n + 3 i + (c - 6) for the velocity.
#pragma once

#include <vector>

#include "vba_math.h"

namespace vba {

struct SchurEntry { int r, c; };        // an entry of the stored triangle: r >= c

VBA_HD int schur_state_unknown(int n, int i, int c) { return c < 6 ? 6 * i + c : 6 * n + 3 * i + (c - 6); }

// Sigma(x_i, x_j)[a][c], a, c in 0 .. 8, where it is stored: S9^-1 is symmetric and only its lower triangle is computed, so the
// entry (u(i, a), u(j, c)) is read at (max, min).  For a state block (i == j) that reads the lower triangle and mirrors it; for
// an edge block (j = i + 1) it decides per entry which of the two is stored (pose-pose and velocity-velocity entries of pose i + 1
// lie below those of pose i, but the velocity of pose i lies below the pose unknowns of pose i + 1).
VBA_HD SchurEntry schur_state_entry(int n, int i, int a, int j, int c) {
    const int p = schur_state_unknown(n, i, a), q = schur_state_unknown(n, j, c);
    return p >= q ? SchurEntry{p, q} : SchurEntry{q, p};
}

// entry (a, c), a, c in 0 .. 5, of the listed block (i >= j) of the pose part as k_cov_gather reads it
VBA_HD SchurEntry schur_pair_entry(int i, int a, int j, int c) {
    if (i == j) return SchurEntry{6 * i + (a > c ? a : c), 6 * i + (a < c ? a : c)};
    return SchurEntry{6 * i + a, 6 * j + c};
}

// Entry e (0 .. 81 (2 n - 1) - 1) of the outputs of k_state_gather: the n state blocks, then the n - 1 edge blocks, row major.
VBA_HD SchurEntry schur_state_gather_entry(int n, int e) {
    const int b = e / 81, a = (e % 81) / 9, c = e % 9;
    return b < n ? schur_state_entry(n, b, a, b, c) : schur_state_entry(n, b - n, a, b - n + 1, c);
}

// The tiles (I, J), I >= J, of kT x kT entries that hold an entry some output of vba_schur_covariance_dyn reads: those of the state and
// edge blocks and of the listed pose blocks, marked entry by entry (blocks straddle tile edges, and so does the pose / velocity
// boundary 6 n).  tiles gets I, J per tile, in the order of the full product's enumeration (I upwards, J upwards inside).
inline void schur_dyn_cov_tiles(int n, int nblk, const int* blk_i, const int* blk_j, int kT, std::vector<int>& tiles) {
    const int nbu = (9 * n + kT - 1) / kT;
    std::vector<char> mark((size_t)nbu * nbu, 0);
    auto hit = [&](SchurEntry s) { mark[(size_t)(s.r / kT) * nbu + s.c / kT] = 1; };
    for (int e = 0; e < 81 * (2 * n - 1); ++e) hit(schur_state_gather_entry(n, e));
    for (int b = 0; b < nblk; ++b)
        for (int a = 0; a < 6; ++a)
            for (int c = 0; c < 6; ++c) hit(schur_pair_entry(blk_i[b], a, blk_j[b], c));
    tiles.clear();
    for (int I = 0; I < nbu; ++I)
        for (int J = 0; J <= I; ++J)
            if (mark[(size_t)I * nbu + J]) { tiles.push_back(I); tiles.push_back(J); }
}

}  // namespace vba
