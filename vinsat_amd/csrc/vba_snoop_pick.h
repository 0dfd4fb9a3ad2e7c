// vba_snoop_pick.h -- the combine rule of data snooping (vba_snoop, vba_snoop.hip): which of two candidates (w-test value, sorted
// position of the row) is rejected first.  Plain C++ that the device row pass and a host program both compile
// (tests/hostcheck/hostcheck_snoop.cpp, tests/test_snoop_host.py).
//
// The rule is a strict total order on candidates of distinct positions, so a fold gives one winner in whatever order and shape
// the partial results meet (a lane's rows in sequence, then the butterfly of the 16 lanes of a pose):
//   a NaN value never wins (an empty partial result is (NaN, kSnoopNoPos));
//   the larger value wins;
//   equal values: the smaller position wins.  Inside a pose the upload's stable sort keeps the input order, so the smaller sorted
//   position is the smaller input row index.
#pragma once

#if defined(__HIPCC__)
#define VBA_PICK_HD __host__ __device__ __forceinline__
#else
#define VBA_PICK_HD inline
#endif

namespace vba {

constexpr int kSnoopNoPos = 0x7fffffff;     // the position of "no candidate"

// true: candidate a is rejected before candidate b
VBA_PICK_HD bool better(double a_val, int a_pos, double b_val, int b_pos) {
    if (a_val != a_val) return false;
    if (b_val != b_val) return true;
    return a_val > b_val || (a_val == b_val && a_pos < b_pos);
}

// (val, pos) <- the better of (val, pos) and (o_val, o_pos)
VBA_PICK_HD void pick(double& val, int& pos, double o_val, int o_pos) {
    const bool take = better(o_val, o_pos, val, pos);
    val = take ? o_val : val;
    pos = take ? o_pos : pos;
}

}  // namespace vba
