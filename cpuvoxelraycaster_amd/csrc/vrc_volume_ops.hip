// vrc_volume_ops.hip -- the entry points on volumes alone that have their kernels in files of their own (include/vrc.h): the
// automaton step and the seeded fill (vrc_cells_*; vrc_cells.hip), the calls along an axis (vrc_columns_*; vrc_columns.hip),
// the calls between two depths (vrc_levels_*; vrc_levels.hip) and the dilation and erosion by a list of offsets
// (vrc_morph_apply; vrc_morph.hip).  Host code only: checks, then one staged_call (vrc_volume_state.h; ordering: DESIGN.md).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vrc.h"
#include "vrc_box_words.h"
#include "vrc_cells.h"
#include "vrc_columns.h"
#include "vrc_levels.h"
#include "vrc_morph.h"
#include "vrc_volume_state.h"

// ---- cells: a neighbour-count step between two volumes and the seeded fill (the rules: include/vrc.h; the kernels: vrc_cells.hip) ----

extern "C" int vrc_cells_step(vrc_volume* dst, vrc_volume* src, int neighbours, uint32_t birth_mask, uint32_t survive_mask, int outside,
                              uint64_t* changed, int mem, void* stream)
{
    const char* what = "vrc_cells_step";
    if (!dst || !src) return vrc::fail(VRC_ERR_INVALID, "%s: null argument", what);
    if (const int rc = check_pair(what, dst, src, true)) return rc;
    if (neighbours != VRC_CELLS_FACES && neighbours != VRC_CELLS_ALL) return vrc::fail(VRC_ERR_INVALID, "%s: neighbours %d is neither 6 nor 26", what, neighbours);
    const uint32_t counts = (2u << neighbours) - 1u;                    // bits 0 .. neighbours
    if (birth_mask & ~counts) return vrc::fail(VRC_ERR_INVALID, "%s: birth_mask 0x%x has a bit above bit %d", what, birth_mask, neighbours);
    if (survive_mask & ~counts) return vrc::fail(VRC_ERR_INVALID, "%s: survive_mask 0x%x has a bit above bit %d", what, survive_mask, neighbours);
    if (outside != 0 && outside != 1) return vrc::fail(VRC_ERR_INVALID, "%s: outside %d is neither 0 nor 1", what, outside);
    if (changed)
        if (const int rc = check_mem(what, mem)) return rc;
    // the counter is the call's one list: in host form it is staged in 8 bytes of the call's own and the call is synchronous
    const Call call = pair_call(dst, src, changed ? mem : VRC_MEM_DEVICE, stream);
    const StagePart parts[] = {{changed, 8u, STAGE_OUT}};
    return staged_call(what, call, parts, [&](void* const* d) {
        const hipError_t zeroed = d[0] ? hipMemsetAsync(d[0], 0, 8u, call.st) : hipSuccess;
        if (zeroed == hipSuccess)
            vrc::cells_step_run(dst->d_bricks, src->d_bricks, dst->depth, neighbours, birth_mask, survive_mask, outside, (unsigned long long*)d[0], call.st);
        return zeroed;
    });
}

extern "C" int vrc_cells_fill_random(vrc_volume* v, uint32_t seed, uint64_t threshold, const uint32_t* lo_hi, int op, void* stream)
{
    const char* what = "vrc_cells_fill_random";
    if (!v) return vrc::fail(VRC_ERR_INVALID, "%s: null volume", what);
    if (threshold > (1ull << 32)) return vrc::fail(VRC_ERR_INVALID, "%s: threshold %llu above 2^32", what, (unsigned long long)threshold);
    if (const int rc = check_op(what, op)) return rc;
    const uint32_t S = 1u << v->depth, whole[6] = {0u, 0u, 0u, S, S, S};
    uint32_t lo[3], hi[3];
    if (!clip_box(lo_hi ? lo_hi : whole, S, lo, hi)) return VRC_OK;      // empty, inverted or wholly outside: nothing to write
    const Call call = volume_call(v->device, VRC_MEM_DEVICE, stream, v, true);
    return staged_call(what, call, [&]() {
        vrc::cells_fill_random_run(v->d_bricks, v->depth, seed, threshold, lo, hi, op, call.st);
        return hipSuccess;
    });
}

// ---- columns: the profile of every column, spans from height maps, selection by the solid voxels met (the rules: include/vrc.h; the kernels: vrc_columns.hip) ----

// rect (NULL: the whole face) into out[4]: non-empty and inside [0, S]^2, not clipped
static int check_rect(const char* what, const uint32_t* rect, uint32_t S, uint32_t out[4])
{
    const uint32_t whole[4] = {0u, 0u, S, S};
    for (int i = 0; i < 4; ++i) out[i] = (rect ? rect : whole)[i];
    if (out[0] < out[2] && out[1] < out[3] && out[2] <= S && out[3] <= S) return VRC_OK;
    return vrc::fail(VRC_ERR_INVALID, "%s: rect (%u, %u, %u, %u) is empty or outside the %u x %u face", what, out[0], out[1], out[2], out[3], S, S);
}

extern "C" int vrc_columns_profile(vrc_volume* v, int direction, const uint32_t* rect, vrc_column* out, int mem, void* stream)
{
    const char* what = "vrc_columns_profile";
    if (!v) return vrc::fail(VRC_ERR_INVALID, "%s: null volume", what);
    if (!out) return vrc::fail(VRC_ERR_INVALID, "%s: null out", what);
    if (direction < 0 || direction > 5) return vrc::fail(VRC_ERR_INVALID, "%s: bad direction %d", what, direction);
    uint32_t r[4];
    if (const int rc = check_rect(what, rect, 1u << v->depth, r)) return rc;
    if (const int rc = check_mem(what, mem)) return rc;
    const Call call = volume_call(v->device, mem, stream, v, false);
    const StagePart parts[] = {{out, (size_t)(r[2] - r[0]) * (r[3] - r[1]) * sizeof(vrc_column), STAGE_OUT}};
    return staged_call(what, call, parts, [&](void* const* d) {
        vrc::columns_profile_run(v->d_bricks, v->depth, direction, r, (vrc_column*)d[0], call.st);
        return hipSuccess;
    });
}

extern "C" int vrc_columns_fill(vrc_volume* v, int axis, const uint32_t* rect, const int32_t* lo_map, int32_t lo_const, const int32_t* hi_map,
                                int32_t hi_const, int op, int mem, void* stream)
{
    const char* what = "vrc_columns_fill";
    if (!v) return vrc::fail(VRC_ERR_INVALID, "%s: null volume", what);
    if (axis < 0 || axis > 2) return vrc::fail(VRC_ERR_INVALID, "%s: bad axis %d", what, axis);
    uint32_t r[4];
    if (const int rc = check_rect(what, rect, 1u << v->depth, r)) return rc;
    if (const int rc = check_op(what, op)) return rc;
    if (const int rc = check_mem(what, mem)) return rc;
    const Call call = volume_call(v->device, mem, stream, v, true);
    const size_t map_bytes = (size_t)(r[2] - r[0]) * (r[3] - r[1]) * 4u;
    const StagePart parts[] = {{lo_map, map_bytes, STAGE_IN}, {hi_map, map_bytes, STAGE_IN}};
    return staged_call(what, call, parts, [&](void* const* d) {
        vrc::columns_fill_run(v->d_bricks, v->depth, axis, r, (const int32_t*)d[0], lo_const, (const int32_t*)d[1], hi_const, op, call.st);
        return hipSuccess;
    });
}

extern "C" int vrc_columns_select(vrc_volume* dst, vrc_volume* src, int direction, uint32_t lo, uint32_t hi, int of, int op, void* stream)
{
    const char* what = "vrc_columns_select";
    if (!dst || !src) return vrc::fail(VRC_ERR_INVALID, "%s: null argument", what);
    if (const int rc = check_pair(what, dst, src, true)) return rc;
    if (direction < 0 || direction > 5) return vrc::fail(VRC_ERR_INVALID, "%s: bad direction %d", what, direction);
    if (lo > hi) return vrc::fail(VRC_ERR_INVALID, "%s: lo %u above hi %u", what, lo, hi);
    if (of < VRC_COLUMNS_SOLID || of > (VRC_COLUMNS_SOLID | VRC_COLUMNS_EMPTY)) return vrc::fail(VRC_ERR_INVALID, "%s: bad of %d", what, of);
    if (const int rc = check_op(what, op)) return rc;
    // no count reaches S: a bound above S + 1 selects what S + 1 selects
    const uint32_t top = (1u << src->depth) + 1u, band_lo = lo < top ? lo : top, band_hi = hi < top ? hi : top;
    const Call call = pair_call(dst, src, VRC_MEM_DEVICE, stream);
    return staged_call(what, call, [&]() {
        vrc::columns_select_run(dst->d_bricks, src->d_bricks, dst->depth, direction, band_lo, band_hi, of, op, call.st);
        return hipSuccess;
    });
}

// ---- levels: the counts of the 2^k cubes, and volumes of two depths made from one another (the rules: include/vrc.h; the kernels: vrc_levels.hip) ----

extern "C" int vrc_levels_counts(vrc_volume* src, uint32_t k, uint32_t* counts, int mem, void* stream)
{
    const char* what = "vrc_levels_counts";
    if (!src) return vrc::fail(VRC_ERR_INVALID, "%s: null volume", what);
    if (!counts) return vrc::fail(VRC_ERR_INVALID, "%s: null counts", what);
    if (k == 0u || k > src->depth) return vrc::fail(VRC_ERR_INVALID, "%s: k %u not in [1, %u], the volume's depth", what, k, src->depth);
    if (const int rc = check_mem(what, mem)) return rc;
    const Call call = volume_call(src->device, mem, stream, src, false);
    const StagePart parts[] = {{counts, (size_t)4u << (3u * (src->depth - k)), STAGE_OUT}};
    return staged_call(what, call, parts, [&](void* const* d) { return vrc::levels_counts_run(src->d_bricks, src->depth, k, (uint32_t*)d[0], call.st); });
}

extern "C" int vrc_levels_reduce(vrc_volume* dst, vrc_volume* src, uint32_t lo, uint32_t hi, int op, void* stream)
{
    const char* what = "vrc_levels_reduce";
    if (!dst || !src) return vrc::fail(VRC_ERR_INVALID, "%s: null argument", what);
    if (const int rc = check_pair(what, dst, src, false)) return rc;
    if (dst->depth >= src->depth) return vrc::fail(VRC_ERR_INVALID, "%s: destination of depth %u is not below the source's %u", what, dst->depth, src->depth);
    if (const int rc = check_op(what, op)) return rc;
    // no count is above 8^k: a bound above 8^k + 1 selects what 8^k + 1 selects
    const uint32_t k = src->depth - dst->depth, top = (1u << (3u * k)) + 1u, band_lo = lo < top ? lo : top, band_hi = hi < top ? hi : top;
    const Call call = pair_call(dst, src, VRC_MEM_DEVICE, stream);
    return staged_call(what, call, [&]() {
        const hipError_t e = reserve(dst->d_levels, dst->levels_cap, vrc::levels_scratch_bytes(src->depth, k));
        return e != hipSuccess ? e : vrc::levels_reduce_run(dst->d_bricks, src->d_bricks, src->depth, k, band_lo, band_hi, op, dst->d_levels, call.st);
    });
}

extern "C" int vrc_levels_expand(vrc_volume* dst, vrc_volume* src, int op, void* stream)
{
    const char* what = "vrc_levels_expand";
    if (!dst || !src) return vrc::fail(VRC_ERR_INVALID, "%s: null argument", what);
    if (const int rc = check_pair(what, dst, src, false)) return rc;
    if (dst->depth <= src->depth) return vrc::fail(VRC_ERR_INVALID, "%s: destination of depth %u is not above the source's %u", what, dst->depth, src->depth);
    if (const int rc = check_op(what, op)) return rc;
    const Call call = pair_call(dst, src, VRC_MEM_DEVICE, stream);
    return staged_call(what, call, [&]() {
        vrc::levels_expand_run(dst->d_bricks, dst->depth, src->d_bricks, dst->depth - src->depth, op, call.st);
        return hipSuccess;
    });
}

// ---- morphology: dilation and erosion by a list of offsets (the rule: include/vrc.h; the kernels: vrc_morph.hip) ----

extern "C" int vrc_morph_apply(vrc_volume* dst, vrc_volume* src, int what_op, int of, uint64_t n, const int32_t* offsets, const int32_t* origin, int outside,
                               int op, int mem, void* stream)
{
    const char* what = "vrc_morph_apply";
    if (!dst || !src) return vrc::fail(VRC_ERR_INVALID, "%s: null argument", what);
    if (const int rc = check_pair(what, dst, src, true)) return rc;
    if (what_op != VRC_MORPH_DILATE && what_op != VRC_MORPH_ERODE) return vrc::fail(VRC_ERR_INVALID, "%s: bad what %d", what, what_op);
    if (of != VRC_MORPH_SOLID && of != VRC_MORPH_EMPTY) return vrc::fail(VRC_ERR_INVALID, "%s: bad of %d", what, of);
    if (outside != 0 && outside != 1) return vrc::fail(VRC_ERR_INVALID, "%s: outside %d is neither 0 nor 1", what, outside);
    if (const int rc = check_op(what, op)) return rc;
    if (const int rc = check_mem(what, mem)) return rc;
    if (n > VRC_MORPH_MAX_OFFSETS) return vrc::fail(VRC_ERR_INVALID, "%s: %llu offsets, more than %u", what, (unsigned long long)n, VRC_MORPH_MAX_OFFSETS);
    if (n && !offsets) return vrc::fail(VRC_ERR_INVALID, "%s: null offsets", what);
    const int32_t pivot[3] = {origin ? origin[0] : 0, origin ? origin[1] : 0, origin ? origin[2] : 0};
    if (mem == VRC_MEM_HOST)
        for (uint64_t i = 0; i < n; ++i) {
            const long long e[3] = {(long long)offsets[3u * i] - pivot[0], (long long)offsets[3u * i + 1u] - pivot[1], (long long)offsets[3u * i + 2u] - pivot[2]};
            for (int a = 0; a < 3; ++a)
                if (e[a] < -VRC_MORPH_REACH || e[a] > VRC_MORPH_REACH)
                    return vrc::fail(VRC_ERR_INVALID, "%s: offset %llu is (%lld, %lld, %lld) after the origin, beyond +-%d", what, (unsigned long long)i, e[0], e[1],
                                     e[2], VRC_MORPH_REACH);
        }
    // the list is the call's one part: in host form it is staged in a block of the call's own and the call is synchronous
    const Call call = pair_call(dst, src, mem, stream);
    const StagePart parts[] = {{offsets, (size_t)n * 12u, STAGE_IN}};
    return staged_call(what, call, parts, [&](void* const* d) {
        // the prepared element: a block of dst's own, fixed in size; the calls that write it are dst's edits, one behind the other
        const hipError_t e = dst->d_morph ? hipSuccess : hipMalloc(&dst->d_morph, vrc::MORPH_BLOCK_BYTES);
        return e != hipSuccess ? e : vrc::morph_run(dst->d_bricks, src->d_bricks, dst->depth, what_op == VRC_MORPH_ERODE, of == VRC_MORPH_EMPTY, outside, n,
                                                    (const int32_t*)d[0], pivot, op, dst->d_morph, call.st);
    });
}
