// vrc_plan.h -- the launch planner of the frame kernels: which build of the table in vrc_kernels.hip runs (lane map, waves
// per SIMD), how the frame is cut into work units (sample chunk, tail chunk, tail tiles) and how large the grid is.
// A function of values: no HIP call, no renderer, no globals, so it runs -- and is tested, tests/test_frame_plan.py --
// on a machine without a device.  vrc_renderer.cpp's render_impl is its only caller in the library.
#pragma once
#include <cstdio>
#include <cstdlib>

#include "vrc_internal.h"

namespace vrc {

// Scheduling knobs of the frame kernels.  Every renderer carries its own copy (two renderers may use different
// kernels, from different threads); the process-wide defaults (vrc_renderer.cpp) only seed new renderers and are read
// and written under their mutex.
struct Tuning {
    uint32_t blocks_per_cu = 0;         // 0 = the library's choice of build (waves per SIMD), see plan_units
    bool blocks_per_cu_set = false;
    uint32_t sample_chunk = 0;   // 0 = automatic
    uint32_t tail_units_per_wave = 4;   // automatic chunking: units of half the chunk for the last tiles (0 = off); tools/chunk_time.py
    bool reuse_invariant = false;       // pinhole camera: walk a unit's sample-invariant rays once (never a process default)
    bool walk_from_root = false;        // measurement switch: no ray starts below the root
    uint32_t lane_samples = 0;          // lane <-> (pixel, sample) map of the stage-synchronous kernel: 0 = automatic, 1, 4
    bool quad_walks = true;             // pinhole kernels: the sample-invariant walks quadrant by quadrant where a launch allows it
};

struct PlanInput {
    vrc_camera cam;
    vrc_frame_params p;         // the caller's, range-checked (render_impl)
    uint32_t width, height;     // of the frame
    uint32_t depth;             // of the scene
    int cu_count;
    bool fused;                 // resolve + pack + reset in the frame kernel (vrc_render_frame_resolved)
    bool capture;               // a primary-hit capture is set (vrc_renderer_set_primary_capture)
    Tuning tuning;
};

struct FramePlan {
    const FrameKernel* kernel;  // the table row to launch; nullptr = nothing to launch (this shard owns no rows)
    uint32_t grid, lds;
    vrc_frame_params p;         // normalised: spp 0 -> 1, the shard fields reset when unsharded
    uint32_t n_items, sample_chunk, sample_chunk_tail, tail_tiles, checker_wide;   // as in FrameArgs
};

// The build, the work units and the grid for the kind and the lane map that `v` names (its waves are chosen here), into
// `u`, whose p and n_items plan_frame has filled in.  `fit`: the workgroups whose LDS fits a CU.
inline int plan_units(const PlanInput& in, FrameVariant v, uint32_t fit, FramePlan& u)
{
    const Tuning& tuning = in.tuning;
    const vrc_frame_params& p = u.p;
    const bool s4 = v.map == LaneMap::samples4;
    const uint64_t items = u.n_items;
    uint64_t want = (items + VRC_RENDER_BLOCK - 1) / VRC_RENDER_BLOCK;
    u.sample_chunk = u.sample_chunk_tail = u.tail_tiles = 0;
    // waves per SIMD: the kind's standard build, or for the lens one-bounce kernel on the 8 x 8 map 7 -- by the caller's
    // blocks_per_cu >= 7, by default for whole-spp units (tools/sweep_waves.sh, profiles/r03/sweep_waves_below.txt: 7 by
    // 1-1.5 % with frames in flight, 6 alone on the chip).  Deep trees: the stacks of that many workgroups do not fit a CU's
    // LDS.  A kind without a build at these waves (the from-root builds) runs its standard build on this grid.
    v.waves = 0u;                                // (no build has 0: the kind's standard build)
    v.waves = frame_kernel(v)->v.waves;
    const bool whole_spp = p.use_samples && p.spp > 1 && tuning.sample_chunk >= p.spp;
    if (!v.pinhole && v.one_bounce && v.map == LaneMap::tile8x8 && (tuning.blocks_per_cu ? tuning.blocks_per_cu >= 7u : whole_spp))
        v.waves = 7u;
    if (v.waves > fit) v.waves = fit;
    u.kernel = vrc::frame_kernel(v);
    // workgroups per CU on the grid: the build's waves, or fewer if the caller asks for fewer
    const uint32_t bpc = tuning.blocks_per_cu && tuning.blocks_per_cu < v.waves ? tuning.blocks_per_cu : v.waves;
    const uint64_t cap = (uint64_t)in.cu_count * bpc;
    if (p.use_samples && p.spp > 1) {
        // Units should be short against the launch (its end waits for the last unit of every wave, and the oldest
        // wave of a SIMD runs ~3.6x faster than the youngest) yet not so small that the accumulator atomics and
        // queue traffic show: the largest chunk that still gives ~48 units per wave of a full grid, else 2 samples
        // per unit, else (small multi-GPU shards) 1.  Measured: C3 1.91 -> 1.83 ms, C5 26.3 -> 26.0 ms
        // (tools/chunk_time.py).
        const uint64_t tiles = items / 64, waves = cap * (VRC_RENDER_BLOCK / 64);
        uint32_t c = tuning.sample_chunk ? tuning.sample_chunk : p.spp;
        if (c > p.spp) c = p.spp;
        if (!tuning.sample_chunk && s4) {
            // four samples abreast: a unit's samples come in fours (a tile has 16 pixels, so there are four times the units)
            while (c % 8u == 0u && tiles * (p.spp / c) < 48 * waves) c /= 2;
        } else if (!tuning.sample_chunk) {
            while (c > 2 && tiles * ((p.spp + c - 1) / c) < 48 * waves) c = (c + 1) / 2;
            if (c == 2 && tiles * ((p.spp + 1) / 2) < 8 * waves) c = 1;
        }
        u.sample_chunk = c < p.spp ? c : 0;
        // shorter units for the tiles handed out last (about four per wave): halves the spread of the waves' end times
        uint64_t units = tiles * ((p.spp + c - 1) / c);
        if (!tuning.sample_chunk && c >= 2 && tuning.tail_units_per_wave && (!s4 || c % 8u == 0u)) {
            const uint32_t ct = c / 2, cpt_tail = (p.spp + ct - 1) / ct;
            uint64_t tt = (uint64_t)tuning.tail_units_per_wave * waves / cpt_tail;
            if (tt > tiles) tt = tiles;
            u.sample_chunk_tail = ct;
            u.tail_tiles = (uint32_t)tt;
            units = (tiles - tt) * ((p.spp + c - 1) / c) + tt * cpt_tail;
        }
#ifdef VRC_EXP_UNITS   // experiment builds only (tools/build_variant.py): "head chunk,tail chunk,tail units per wave" from the environment
        if (const char* ev = getenv("VRC_EXP_UNITS")) {
            unsigned ec = 0, ect = 0, etpw = 0;
            if (sscanf(ev, "%u,%u,%u", &ec, &ect, &etpw) == 3 && ec >= 1 && ect >= 1 && !s4) {
                c = ec > p.spp ? p.spp : ec;
                u.sample_chunk = c < p.spp ? c : 0;
                const uint32_t cpt_tail = (p.spp + ect - 1) / ect;
                uint64_t tt = (uint64_t)etpw * waves / cpt_tail;
                if (tt > tiles) tt = tiles;
                u.sample_chunk_tail = ect; u.tail_tiles = (uint32_t)tt;
                units = (tiles - tt) * ((p.spp + c - 1) / c) + tt * cpt_tail;
            }
        }
#endif
        // the kernel numbers work units in 32 bits
        if (units > 0xfffffff0ull) return fail(VRC_ERR_INVALID, "vrc_render_frame: %llu work units (tiles x sample chunks) do not fit 32 bits; "
                                               "use fewer samples per call or a larger sample chunk", (unsigned long long)units);
        // one wave per unit until the chip is full: a shard of few tiles still spreads over all CUs
        want = (units + VRC_RENDER_BLOCK / 64 - 1) / (VRC_RENDER_BLOCK / 64);
    }
    u.grid = (uint32_t)(want < cap ? want : cap);
    return VRC_OK;
}

inline int plan_frame(const PlanInput& in, FramePlan& out)
{
    const Tuning& tuning = in.tuning;
    out = FramePlan{};
    vrc_frame_params& p = out.p;
    p = in.p;
    if (p.spp == 0) p.spp = 1;
    // rows this shard owns, in compact row space
    uint32_t rows = in.height;
    if (p.row_block && p.shard_count > 1) {
        const uint32_t nblocks = (in.height + p.row_block - 1) / p.row_block;
        const uint32_t mine = nblocks > p.shard_index ? (nblocks - p.shard_index + p.shard_count - 1) / p.shard_count : 0;
        rows = mine * p.row_block;
    } else {
        p.row_block = 0; p.shard_index = 0; p.shard_count = 1;
    }
    // checkerboard frames on the stage-synchronous kernel: 16 x 8 pixel tiles, 64 selected pixels each
    out.checker_wide = p.checker_parity >= 0 ? 1u : 0u;
    // the lane <-> (pixel, sample) map (vrc_renderer_set_lane_samples): four samples abreast where the kernel has a build for it
    // and the frame's samples divide by four -- the accumulators make the order of a pixel's samples immaterial, the 0.4 / 0.6
    // blend of the non-sample mode (raycaster.hpp:79-85) does not
    const bool can_s4 = p.use_samples && p.spp % 4u == 0u && p.checker_parity < 0 &&
                        p.gi_bounces <= 1u && !tuning.walk_from_root && !tuning.reuse_invariant &&
                        (tuning.sample_chunk == 0u || tuning.sample_chunk % 4u == 0u);
    // The library's choice (lane_samples 0), measured on C3 / C4 and their 1/2 .. 1/8 shards (profiles/r04/ab_lane_map.txt,
    // shard_inflight_lane_map.txt): four abreast for a launch that has the chip to itself -- 3-6 % off a frame's latency: four
    // times the units, a quarter as long, no accumulator atomics -- and the pixel tiles for whole-spp units, which a caller asks
    // for when frames overlap (there the 8 x 8 map wins by 5 %: both maps issue the same number of VALU instructions,
    // profiles/r04/pmcq_ns{1,4}.txt, and four abreast has four times the queue pops and unit prologues for a wave to sit out,
    // which a chip kept full by overlapping launches cannot hide -- DESIGN.md section 9).
    const bool caller_whole_spp = tuning.sample_chunk != 0u && tuning.sample_chunk >= p.spp;
    // the build to launch (vrc_internal.h, FrameVariant): its lane map is final here, but for the quadrant walks (below)
    FrameVariant v{camera_is_pinhole(in.cam), p.gi_bounces <= 1u, in.fused, tuning.walk_from_root, LaneMap::tile8x8, 0u};
    if (can_s4 && (tuning.lane_samples == 4u || (tuning.lane_samples == 0u && !caller_whole_spp))) v.map = LaneMap::samples4;
    const bool s4 = v.map == LaneMap::samples4;
    const uint32_t tw = s4 ? 4u : 8u;
    const uint32_t tiles_per_row = out.checker_wide ? (in.width + 15u) / 16u : (in.width + tw - 1u) / tw;
    const uint64_t items = (uint64_t)tiles_per_row * ((rows + tw - 1u) / tw) * 64ull;
    if (items > 0xfffffff0ull) return fail(VRC_ERR_INVALID, "vrc_render_frame: frame too large");
    out.n_items = (uint32_t)items;
    if (out.n_items == 0) return VRC_OK;
    // Quadrant walks (render_sync_body's QUAD; vrc_renderer_set_quad_walks, on by default): the pinhole kernels on the 8 x 8 map
    // when every work unit has a multiple of four samples (the walks of a pixel's sample-invariant rays are laid out four
    // abreast), without invariant-ray reuse (one walk per unit: nothing to lay out) and without the primary-hit capture (which
    // records per-lane complexities); the tree must have 8 levels or more (a walk's final state waits in stack rows 3..7); and
    // this build of the library must have them.
    // Decided BEFORE the occupancy and the unit policy, which follow the build that is launched (its builds sit at their own
    // occupancy); the one condition that needs the policy's result -- every unit a multiple of four samples -- is checked after
    // it, and a launch that fails it is planned again for the plain build.
    const bool quad_candidate = vrc::quad_available() && tuning.quad_walks && !s4 && p.use_samples && p.spp % 4u == 0u &&
                                !tuning.reuse_invariant && !in.capture && !v.from_root && !out.checker_wide && v.pinhole && in.depth >= 8u;
    out.lds = frame_lds_bytes(in.depth);
    const uint32_t fit = 163840u / out.lds;          // workgroups whose LDS fits a CU
    if (quad_candidate) v.map = LaneMap::quad;
    if (int rc = plan_units(in, v, fit, out)) return rc;
    if (quad_candidate) {
        const uint32_t c_head = out.sample_chunk ? out.sample_chunk : p.spp, c_tail = out.sample_chunk_tail ? out.sample_chunk_tail : c_head;
        v.map = LaneMap::tile8x8;
        if (c_head % 4u != 0u || c_tail % 4u != 0u) return plan_units(in, v, fit, out);
    }
    return VRC_OK;
}

}  // namespace vrc
