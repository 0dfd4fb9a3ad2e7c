// vba_solve_units.h -- solver-internal: the limits the solver units agree on and the host launchers they offer each other.
// vba_solve.hip's dispatch (launch_solve, configure_solver_device) calls them; the rest of the library sees vba_launch.h only.
// Every launcher takes `pivot` (the kernels with row pivoting inside a 9x9 block, or the unpivoted ones: see solver_mine,
// vba_solve_step.h) and is asynchronous on `s`.  hipFuncSetAttribute needs a kernel's address, so every unit sets the
// dynamic-LDS limits of its own kernels (configure_*_device, per device, from configure_solver_device).
#pragma once
#include <hip/hip_runtime.h>

#include "vba_device.h"

namespace vba {

constexpr int kCrMax = 64;
constexpr int kFusedChunkMax = 28;  // largest chunk whose blocks, staged inputs and elimination scratch fit 160 KiB of LDS
constexpr int kCrThreads = 1024;
constexpr int kCrSplitMin = 24;     // from this many separators on, the first level runs as its own multi-CU kernel (re-measured with
                                    // the two-wave chunks: 56.2 us per call against 59.1 with all levels in the one workgroup)


#pragma GCC visibility push(hidden)     // (internal to the library, like everything in vba_context.h)
// vba_solve.hip
bool walk_forms_blocks(const DevView& V);   // the sequential walk of the batched mode forms its blocks itself

// vba_solve_seq.hip
void launch_solve_blockdiag(const DevView& V, bool pivot, hipStream_t s);           // landmark-only phase: independent poses
void launch_solve_walk(const DevView& V, bool pivot, bool forms, hipStream_t s);    // k_solve_quad (V.pack == 2) or k_solve

// vba_solve_chunks.hip
// level-1 chunk elimination (forms: from the per-pose inputs), the second level if V.chunk2 > 0 and, unless V.chunk2 < 0 (cyclic
// reduction: launch_solve_cr), the sequential walk of the last reduced system
void launch_solve_chunks(const DevView& V, bool pivot, bool forms, hipStream_t s);
void launch_solve_recover2(const DevView& V, hipStream_t s);                        // level 2 -> level 1 separators
void launch_solve_recover(const DevView& V, int chunk, hipStream_t s);              // interiors (chunk == 0: none) + retraction
hipError_t configure_chunks_device();

// vba_solve_cr.hip: the reduced system of a one-level partition by block cyclic reduction (every window picks its kernel by its
// own number of separators; the launches cover the range of the handle)
void launch_solve_cr(const DevView& V, bool pivot, hipStream_t s);          // = launch_cr_front2 + launch_cr_short
void launch_cr_front2(const DevView& V, bool pivot, hipStream_t s);         // kCrSplitMin separators or more: k_cr_level01 + launch_cr_tail2
void launch_cr_tail2(const DevView& V, bool pivot, hipStream_t s);          // k_solve_reduced_cr<., 2>: what two levels in front left
void launch_cr_short(const DevView& V, bool pivot, hipStream_t s);          // k_solve_reduced_cr<., 0>: windows below kCrSplitMin, if any
hipError_t configure_cr_device();

// vba_solve_variants.hip (comparison builds, make VARIANTS=1): true if the handle asks for one of the comparison solvers, which
// has then been launched in place of the production path
bool launch_solve_comparison(const DevView& V, bool pivot, hipStream_t s);
hipError_t configure_variants_device();

// sets the dynamic-LDS limit of each kernel of a unit's list
struct LdsLimit { const void* fn; int bytes; };
template <int N>
inline hipError_t set_lds_limits(const LdsLimit (&set)[N]) {
    for (const LdsLimit& e : set) {
        const hipError_t rc = hipFuncSetAttribute(e.fn, hipFuncAttributeMaxDynamicSharedMemorySize, e.bytes);
        if (rc != hipSuccess) return rc;
    }
    return hipSuccess;
}
#pragma GCC visibility pop

}  // namespace vba
