// vba_solve_cr.hip -- the reduced system over the separators by block cyclic reduction: the first two levels on their own CUs
// (k_cr_level01), the rest in one workgroup (k_solve_reduced_cr).  Device bodies and the method: vba_solve_cr_body.h.
#include "vba_solve_cr_body.h"

namespace vba {

#ifdef VBA_RESIDENT_STAMPS
VBA_KSTAMP_FETCH(fetch_kstamps_cr)
#endif

template <bool PIVOT>
__global__ __launch_bounds__(256) void k_cr_level01(DevView V, int s) {
    __shared__ __attribute__((aligned(16))) double blk[7 * 252];
    cr_level01_body<PIVOT>(V, s, blockIdx.y, blockIdx.x, blk);
}

template <bool PIVOT>
static void launch_cr_level01_t(const DevView& V, int n0_max, hipStream_t s) {
    hipLaunchKernelGGL(k_cr_level01<PIVOT>, dim3((n0_max + 3) / 4, V.W), dim3(256), 0, s, V, V.chunk);
}
template <bool PIVOT, int PRE>
static void launch_reduced_cr_t(const DevView& V, size_t lds, hipStream_t s) {
    hipLaunchKernelGGL((k_solve_reduced_cr<PIVOT, PRE>), dim3(V.W), dim3(kCrThreads), lds, s, V, V.chunk);
}

// separators of the longest and of the shortest window of the handle
static int n0_max_of(const DevView& V) { return (V.n_max + V.chunk - 1) / V.chunk - 1; }
static int n0_min_of(const DevView& V) { return (V.n_min + V.chunk - 1) / V.chunk - 1; }

void launch_cr_tail2(const DevView& V, bool pivot, hipStream_t s) {
    const size_t lds = cr_tail2_lds_bytes(n0_max_of(V));
    if (pivot) launch_reduced_cr_t<true, 2>(V, lds, s);
    else launch_reduced_cr_t<false, 2>(V, lds, s);
}

void launch_cr_front2(const DevView& V, bool pivot, hipStream_t s) {
    const int n0_max = n0_max_of(V);
    if (n0_max < kCrSplitMin) return;
    if (pivot) launch_cr_level01_t<true>(V, n0_max, s);
    else launch_cr_level01_t<false>(V, n0_max, s);
    launch_cr_tail2(V, pivot, s);
}

void launch_cr_short(const DevView& V, bool pivot, hipStream_t s) {
    const int n0_max = n0_max_of(V);
    if (n0_min_of(V) >= kCrSplitMin || n0_max <= 0) return;
    const int nb = n0_max < kCrSplitMin ? n0_max : kCrSplitMin - 1;
    const size_t lds = (size_t)nb * 252 * sizeof(double);
    if (pivot) launch_reduced_cr_t<true, 0>(V, lds, s);
    else launch_reduced_cr_t<false, 0>(V, lds, s);
}

void launch_solve_cr(const DevView& V, bool pivot, hipStream_t s) {
    launch_cr_front2(V, pivot, s);      // first levels on their own CUs, the rest in one workgroup
    launch_cr_short(V, pivot, s);
}

hipError_t configure_cr_device() {
    const LdsLimit set[] = {
        {reinterpret_cast<const void*>(k_solve_reduced_cr<false, 0>), kCrLdsCap}, {reinterpret_cast<const void*>(k_solve_reduced_cr<true, 0>), kCrLdsCap},
        {reinterpret_cast<const void*>(k_solve_reduced_cr<false, 2>), kCrTail2LdsCap}, {reinterpret_cast<const void*>(k_solve_reduced_cr<true, 2>), kCrTail2LdsCap}};
    return set_lds_limits(set);
}

}  // namespace vba
