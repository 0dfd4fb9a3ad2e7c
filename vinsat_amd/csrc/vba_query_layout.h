// vba_query_layout.h -- how the scratch of a query (vba_covariance, vba_reliability, vba_outlier_power, vba_snoop,
// vba_snoop_scaled) is cut into buffers.  Plain host C++ without HIP, so that tests/hostcheck/sanitize_power_main.cpp and
// sanitize_snoop_fit_main.cpp run it under the sanitizers.
//
// A layout is written once, as a function that takes its buffers from a Carver in order; it runs twice: over a Carver without a
// base it only counts (total() is the size to allocate), over the allocation it places the buffers.  Every buffer starts on a
// multiple of 256 bytes.
#pragma once
#include <cstddef>

struct Carver {
    char* base = nullptr;       // nullptr: counting
    size_t off = 0;
    template <class T>
    T* take(size_t count) {
        T* q = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += (count * sizeof(T) + 255) & ~size_t(255);
        return q;
    }
    size_t total() const { return off; }
};

// vba_reliability: lev, wt [W][m_max] doubles, perm [W][m_max] ints, pstat [W][n_max][3] doubles -- 20 bytes per row and window
// (W = 4096 windows of 50 000 rows: 1.6 GB per row array, 4.1 GB in all)
struct RelBufs { double *lev, *wt; int* perm; double* pstat; };
inline RelBufs rel_layout(Carver& c, size_t W, size_t N, size_t M) {
    RelBufs b;
    b.lev = c.take<double>(W * M);
    b.wt = c.take<double>(W * M);
    b.perm = c.take<int>(W * M);
    b.pstat = c.take<double>(W * N * 3);
    return b;
}

// vba_outlier_power, beyond the reliability scratch (whose device copy of the permutation it reads): four row arrays [W][m_max],
// pose_fit [W][n_max][4], the two pose numbers behind the window totals, fit [W][8]
struct PowBufs { double *row[4], *pfit, *paux, *fit; };
inline PowBufs pow_layout(Carver& c, size_t W, size_t N, size_t M) {
    PowBufs b;
    for (double*& r : b.row) r = c.take<double>(W * M);
    b.pfit = c.take<double>(W * N * 4);
    b.paux = c.take<double>(W * N * 2);
    b.fit = c.take<double>(W * 8);
    return b;
}

// vba_snoop, beyond the reliability scratch (whose wtest array and device copy of the permutation it uses).  Unlike a query's, this
// scratch is state: orig [W][m_max] the confidence a rejected row had, mask [W][m_max] the cumulative rejections, both in the input
// order of the rows and valid until the window's rows are uploaded again; prej [W][n_max] rows each pose lost in the last call.
struct SnoopBufs { double* orig; unsigned char* mask; int* prej; };
inline SnoopBufs snoop_layout(Carver& c, size_t W, size_t N, size_t M) {
    SnoopBufs b;
    b.orig = c.take<double>(W * M);
    b.mask = c.take<unsigned char>(W * M);
    b.prej = c.take<int>(W * N);
    return b;
}

// vba_snoop_scaled, beside the snoop state above and a query's scratch like the first three: pose [W][n_max][3] per pose the sum
// of w |r|^2, the sum of the leverages and the rows of non-zero weight; win [W][2] per window s0sq and the critical value used.
struct SnoopFitBufs { double *pose, *win; };
inline SnoopFitBufs snoop_fit_layout(Carver& c, size_t W, size_t N) {
    SnoopFitBufs b;
    b.pose = c.take<double>(W * N * 3);
    b.win = c.take<double>(W * 2);
    return b;
}
