// vba_options.hip -- what a caller can set on a handle: vba_set_option and the setters behind it, solver, integrator, stream, prior,
// host watch; and the counters that tell what the choices did.
#include "vba_context.h"

// How every setter opens: a call speculated under the old value is dropped (settle), and the generation moves on (touch) so that
// nothing keyed to the old value is replayed -- before the new value is looked at: a rejected value moves the generation too.
static int begin_setting(vba_handle h) {
    if (!h) return fail(VBA_EINVAL, "null handle");
    if (int rc = settle(h)) return rc;
    h->touch();
    return VBA_OK;
}

int vba_set_solver2(vba_handle h, int chunk, int chunk2) {
    if (int rc = begin_setting(h)) return rc;
    if (chunk < 2 || chunk > 60 || (chunk2 != 0 && chunk2 != -1 && (chunk2 < 2 || chunk2 > 60)))
        return fail(VBA_EINVAL, "chunk sizes must be in [2, 60] (chunk2 = 0: single level, -1: cyclic reduction)");
    if (chunk2 == -1 && (h->n_max + chunk - 1) / chunk - 1 > 128)
        return fail(VBA_EINVAL, "chunk2 = -1 needs at most 128 separators: chunk >= ceil(n_max / 129)");
    h->V.chunk = chunk;
    h->V.chunk2 = chunk2;
    h->no_pack = 0;
    return VBA_OK;
}

int vba_set_solver(vba_handle h, int chunk) {
    if (int rc = begin_setting(h)) return rc;
    h->V.chunk2 = 0;
    if (chunk == -1) {      // default: many windows supply their own parallelism (one wave walks each chain);
        h->no_pack = 0;     // otherwise the chain is cut into chunks and the reduced system over the (at most 64)
                            // separators is solved by cyclic reduction in one workgroup; very long chains: two levels
        if (h->W > kPartitionedWindowsMax || h->n_max < 8) { h->V.chunk = 0; return VBA_OK; }
        // <= 64 separators while that keeps the chunks at <= 8 poses, else up to 128 (their first reduction level runs
        // on its own CUs either way, see k_cr_level0)
        const int c64 = (h->n_max + 64) / 65, c128 = (h->n_max + 128) / 129;
        int c1 = std::max(std::min(c64, std::max(8, c128)), 2);
        // bandwidth mode: the chunks are there for throughput, not for the shortest chain -- fewer separators (less redundant
        // work in the reduced system) win: chunks of 12 measured +7 .. +9 % at 100 poses (256 .. 1000 windows) over the latency
        // rule's chunks of 2, +2 % at 500 poses over chunks of 8 (4 / 8 / 16 / 14 all slower; tools/attic/chunk_bw.sh)
        if (!h->V.lat) c1 = std::max(c1, std::min(12, std::max(2, h->n_max / 3)));
        // latency mode, several windows: the chunk elimination holds 256 registers, i.e. 1024 two-wave blocks are one round of
        // the chip and block 1025 waits for a second one (18 C3 windows of 63 chunks: 26.1 us against 17.7 at 15 windows) --
        // chunks of up to 12 poses where that keeps the elimination in one round (172.8 -> 180.4 k it/s at 18 windows,
        // 194.9 -> 202.3 at 22; no difference where it does not fit either way)
        // latency mode (re-measured in round 4 with the kernels as they are now): chunks of 8 also where 64 separators would allow
        // shorter ones -- one window of 100 poses (C2) 24.8 k it/s against 23.4 k with chunks of 2, 16 such windows 367 k against 319 k,
        // 64 windows 903 k against 749 k; 200 poses: on par with the old rule's 4 for one window, +5 % from 16 windows on
        if (h->V.lat) c1 = std::max(c1, std::min(8, std::max(2, h->n_max / 3)));
        if (h->V.lat && h->W > 1) {
            int c = c1;
            while (c < 12 && (int64_t)h->W * ((h->n_max + c - 1) / c) > 1024) ++c;
            if ((int64_t)h->W * ((h->n_max + c - 1) / c) <= 1024) c1 = c;
        }
        if (c1 <= 60) {
            h->V.chunk = c1;
            h->V.chunk2 = -1;
        } else {
            const int c3 = std::min(std::max((int)std::ceil(std::cbrt((double)h->n_max)), 2), 60);
            h->V.chunk = c3;
            h->V.chunk2 = c3;
        }
        return VBA_OK;
    }
    if (chunk == -2) {      // sequential, one window per wavefront (no packing): diagnostic / comparison
        h->V.chunk = 0;
        h->no_pack = 1;
        return VBA_OK;
    }
#ifndef VBA_VARIANTS
    if (chunk == -3) return fail(VBA_EINVAL, "three windows per wavefront (k_solve_packed) is a comparison variant that this build does not carry (make VARIANTS=1)");
#endif
    if (chunk == -3) {      // sequential, three windows per wavefront whenever the pose counts allow it
        h->V.chunk = 0;
        h->no_pack = 0;
        h->pack_min = 3;
        return VBA_OK;
    }
    if (chunk < 0 || chunk == 1 || chunk > 60) return fail(VBA_EINVAL, "chunk must be -3, -2, -1, 0 or in [2, 60]");
    h->V.chunk = chunk;
    h->no_pack = 0;
    return VBA_OK;
}

int vba_set_integrator(vba_handle h, int hop100) {
    if (int rc = begin_setting(h)) return rc;
    h->V.hop = hop100 ? 1 : 0;
    h->V.nblk_long = h->V.hop ? 0 : *std::max_element(h->n_long.begin(), h->n_long.end());
    return VBA_OK;
}

int vba_set_accumulate_lanes(vba_handle h, int lanes) {
    if (int rc = begin_setting(h)) return rc;
    if (lanes == 0) {
        const double avg = (double)h->m_max / (double)h->n_max;
        int G = 4;
        while (G < 64 && avg / G > 16.0) G *= 2;     // measured on C3 x 1024: G = 8 (12.5 rows per lane) is the fastest
        // few windows: spend idle lanes on shorter per-lane loops (latency) instead of fewer shuffles (throughput)
        // (limit re-measured in round 4 with the handle's other defaults as they are now: 3 windows of 500 poses 57.4 k it/s with 32
        // lanes against 52.8 k with 16, 6 windows 93.0 against 91.2 with 16 instead of 8; 2, 4, 8, 12 windows unchanged)
        while (G < 64 && (int64_t)h->W * h->n_max * G * 2 <= 49152) G *= 2;
        lanes = G;
    }
    if (lanes != 4 && lanes != 8 && lanes != 16 && lanes != 32 && lanes != 64) return fail(VBA_EINVAL, "lanes must be 0, 4, 8, 16, 32 or 64");
    h->V.acc_lanes = lanes;
    return VBA_OK;
}

// Tiles of 256 rows per observation block of the latency-mode trial kernel (plain geometry: fusion bit 0 off).  Measured on the
// chained 20-call schedule (k it/s, tiles 1 / 2 / 4 / 8): one C4 window (782 tiles) 15.3 / 16.4 / 17.4 / 16.2, one C5 window
// (1954 tiles) 9.8 / 11.5 / 12.2 / 12.1, 8 C3 windows (1568) 113.9 / 120.6 / 121.9, 22 C3 windows (4312) 185 / 197 / 195; one C3
// window (196, with that fusion mask) 19.7 / 20.6 / 19.8.  Results do not depend on it (see k_trial).
int vba_set_trial_tiles(vba_handle h, int tiles) {
    if (int rc = begin_setting(h)) return rc;
    if (tiles == 0) {
        const int64_t blocks = (int64_t)h->W * h->V.nblk_obs;
        tiles = blocks >= 600 ? 4 : (blocks >= 150 ? 2 : 1);
    }
    if (tiles != 1 && tiles != 2 && tiles != 4 && tiles != 8) return fail(VBA_EINVAL, "tiles must be 0 (automatic), 1, 2, 4 or 8");
    h->V.trial_tiles = tiles;
    return VBA_OK;
}

static int vba_set_key_carry(vba_handle h, int on) {
    if (int rc = begin_setting(h)) return rc;
    h->carry_enabled = on != 0;
    h->carry_ok = false;
    return VBA_OK;
}

static int vba_set_fusion(vba_handle h, int mask) {
    if (int rc = begin_setting(h)) return rc;
    if (mask < 0 || mask > 127) return fail(VBA_EINVAL, "mask must be in [0, 127]");
#ifndef VBA_VARIANTS
    if (mask & (16 | 32 | 64)) return fail(VBA_EINVAL, "mask bits 4 .. 6 select comparison variants that this build does not carry (make VARIANTS=1)");
#endif
    h->fusion = mask;
    h->fusion_auto = false;
    return VBA_OK;
}

static int vba_set_chunk_waves(vba_handle h, int waves) {
    if (int rc = begin_setting(h)) return rc;
    if (waves != 1 && waves != 2) return fail(VBA_EINVAL, "waves must be 1 or 2");
    h->chunk_waves = waves;
    return VBA_OK;
}

static int vba_set_warm_select(vba_handle h, int on) {
    if (int rc = begin_setting(h)) return rc;
    h->warm_enabled = on == 2 ? 2 : (on != 0);
    h->inline_select = on != 3;     // 3: warm select as its own kernel (k_select_warm), the round-2 mid-point; comparison / tests
    return VBA_OK;
}

static int vba_set_warm_shift(vba_handle h, int shift) {
    if (int rc = begin_setting(h)) return rc;
    if (shift < 42 || shift > 51) return fail(VBA_EINVAL, "shift must be in [42, 51]");
    h->V.warm_shift = shift;
    h->carry_ok = 0;            // a histogram binned with another width cannot be resolved
    return VBA_OK;
}

static int vba_set_bucket_cap(vba_handle h, int cap) {
    if (int rc = begin_setting(h)) return rc;
    if (!h->bucket_cap_alloc) return fail(VBA_ESTATE, "this handle has no bin buckets (it runs the bandwidth-mode kernels)");
    if (cap != 0 && (cap < 8 || cap > h->bucket_cap_alloc)) return fail(VBA_EINVAL, "cap must be 0 (default) or in [8, allocated capacity]");
    h->V.bucket_cap = cap ? cap : h->bucket_cap_alloc;
    h->carry_ok = 0;            // buckets filled with another stride are not addressable any more
    return VBA_OK;
}

int vba_set_host_watch(vba_handle h, int slot, const void* live, const void* copy, int64_t bytes) {
    if (!h || slot < 0 || slot >= 8) return fail(VBA_EINVAL, "bad argument (8 watch slots)");
    if (live && (!copy || bytes < 1)) return fail(VBA_EINVAL, "a watched buffer needs its reference copy and a size");
    watch_quiesce(h);
    h->watch[slot].live = live;
    h->watch[slot].copy = live ? copy : nullptr;
    h->watch[slot].bytes = live ? (size_t)bytes : 0;
    return VBA_OK;
}

static int vba_set_pipeline(vba_handle h, int on) {
    if (int rc = begin_setting(h)) return rc;
    h->pipeline = on != 0;
    return VBA_OK;
}

int vba_pipeline_stats(vba_handle h, int* hits, int* discards) {
    if (!h) return fail(VBA_EINVAL, "null handle");
    if (hits) *hits = h->spec_hits;
    if (discards) *discards = h->spec_discards;
    return VBA_OK;
}

int vba_warm_select_misses(vba_handle h, int* count) {
    if (!h || !count) return fail(VBA_EINVAL, "null argument");
    *count = h->warm_misses;
    return VBA_OK;
}

// fp32 reprojection Jacobian (include/vinsat_ba.h: what is fp32).  A flag of the view: the schedule graphs of the two modes are
// told apart by their view bytes, and the settle drops a call speculated in the other mode.
static int vba_set_jacobian_f32(vba_handle h, int on) {
    if (int rc = begin_setting(h)) return rc;
    if (on != 0 && on != 1) return fail(VBA_EINVAL, "jacobian_f32 must be 0 (fp64, default) or 1 (fp32)");
    h->V.jac_f32 = on;
    return VBA_OK;
}

static int vba_set_pivoting(vba_handle h, int always) {
    if (int rc = begin_setting(h)) return rc;
    h->pivot_mode = always ? 1 : 0;
    return VBA_OK;
}

int vba_solver_fallbacks(vba_handle h, int* count) {
    if (!h || !count) return fail(VBA_EINVAL, "null argument");
    *count = h->fallbacks;
    return VBA_OK;
}

int vba_set_stream(vba_handle h, void* hip_stream, int external) {
    if (int rc = begin_setting(h)) return rc;
    hipStreamSynchronize(h->stream);        // (behind the settle: what it enqueued on the old stream has run as well)
    h->stream = external ? (hipStream_t)hip_stream : h->own_stream;
    return VBA_OK;
}

// No settle: a speculated call carries the `reg` it was enqueued with (spec.reg), and vba_iterate_resident takes it only if
// that is still the handle's; otherwise it settles there.
int vba_set_prior(vba_handle h, int on) {
    if (!h) return fail(VBA_EINVAL, "null handle");
    h->reg = on != 0;
    h->touch();
    return VBA_OK;
}

// the settings a caller of BA() never needs, behind one entry point (include/vinsat_ba.h: VBA_OPT_*)
int vba_set_option(vba_handle h, int option, int value) {
    switch (option) {
        case VBA_OPT_ACCUMULATE_LANES: return vba_set_accumulate_lanes(h, value);
        case VBA_OPT_TRIAL_TILES: return vba_set_trial_tiles(h, value);
        case VBA_OPT_KEY_CARRY: return vba_set_key_carry(h, value);
        case VBA_OPT_WARM_SELECT: return vba_set_warm_select(h, value);
        case VBA_OPT_WARM_SHIFT: return vba_set_warm_shift(h, value);
        case VBA_OPT_BUCKET_CAP: return vba_set_bucket_cap(h, value);
        case VBA_OPT_FUSION: return vba_set_fusion(h, value);
        case VBA_OPT_CHUNK_WAVES: return vba_set_chunk_waves(h, value);
        case VBA_OPT_PIVOTING: return vba_set_pivoting(h, value);
        case VBA_OPT_PIPELINE: return vba_set_pipeline(h, value);
        case VBA_OPT_SCHEDULE_GRAPH: return vba_set_schedule_graph(h, value);
        case VBA_OPT_CHAIN_PROFILE: return vba_set_chain_profile(h, value);
        case VBA_OPT_JACOBIAN_F32: return vba_set_jacobian_f32(h, value);
        default: return fail(VBA_EINVAL, "unknown option (VBA_OPT_*)");
    }
}
