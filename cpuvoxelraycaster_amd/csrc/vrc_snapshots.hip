// vrc_snapshots.hip -- the snapshots taken from an editable volume (include/vrc.h) and their calls: the labels of its connected
// components (vrc_labels_*, vrc_fall_*, vrc_rigid_*, vrc_fracture_*), its distance and travel fields (vrc_distance_*, vrc_travel_*)
// with the straight-line walks over them (vrc_sight_*), and the difference of two volumes as a list of changed words
// (vrc_delta_*).  Kernels: vrc_components.hip, vrc_fall.hip, vrc_rigid.hip, vrc_fracture.hip, vrc_distance.hip, vrc_travel.hip,
// vrc_sight.hip, vrc_delta.hip.  A snapshot owns its memory, is never written after its creator returns, and keeps no event and
// no scratch: its host-memory calls stage in a block of their own, and what it selects or places goes into a volume as an edit
// of that volume (staged_call in vrc_volume_state.h; ordering: DESIGN.md).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <new>

#include "../../include/vrc.h"
#include "vrc_components.h"
#include "vrc_delta.h"
#include "vrc_distance.h"
#include "vrc_fall.h"
#include "vrc_fracture.h"
#include "vrc_rigid.h"
#include "vrc_sight.h"
#include "vrc_travel.h"
#include "vrc_volume_state.h"

struct vrc_labels {
    int device = 0;
    uint32_t depth = 0;
    uint64_t count = 0;
    uint32_t* d_ids = nullptr;            // 8^depth ids, indexed by key
    vrc_component* d_records = nullptr;   // count records, nullptr when count == 0
    bool fractured = false;               // made by vrc_fracture_label: the pieces carry a cell
    uint32_t* d_piece_cells = nullptr;    // fractured: count cells, nullptr when count == 0
};

struct vrc_distance {
    int device = 0;
    uint32_t depth = 0;
    int connectivity = 0;                 // 6 / 26: a travel field made with it; 0: a Euclidean field or a sight field
    bool euclidean = false;               // made by vrc_volume_distance_field: the squared distance to a set, so sqrt is 1-Lipschitz
    uint32_t* d_field = nullptr;          // 8^depth squared distances (travel field: steps), [(x*S + y)*S + z]
};

namespace {

// The frame of the creators: the NULL stream, behind the last asynchronous edit of the medium (and of `seeds`, where given),
// as commit / download are.  *d_array gets the snapshot's 8^depth words (its owner frees them, on failure too), a scratch
// block of `scratch_bytes` lives for the call; run(d_scratch) enqueues the work and reads back the few words the creator needs.
template <class Run>
int snapshot_run(const char* what, vrc_volume* medium, vrc_volume* seeds, uint32_t** d_array, size_t scratch_bytes, Run run)
{
    uint32_t* d_scratch = nullptr;
    const int rc = staged_call(what, null_stream_call(medium, seeds, false, true), [&]() {
        hipError_t e = hipMalloc((void**)d_array, (size_t)4u << (3u * medium->depth));
        if (e == hipSuccess) e = hipMalloc((void**)&d_scratch, scratch_bytes);
        return e == hipSuccess ? run(d_scratch) : e;
    });
    if (d_scratch) (void)hipFree(d_scratch);
    return rc;
}

// the packed maximum of a field's reduction, (value << 32) | ~dense index, 0 where nothing was counted: the value and
// the x y z of the index
void decode_argmax(unsigned long long packed, uint32_t depth, uint32_t* value, uint32_t argmax[3])
{
    *value = 0u; argmax[0] = argmax[1] = argmax[2] = 0u;
    if (!packed) return;
    const uint32_t index = ~(uint32_t)packed, mask = (1u << depth) - 1u;
    *value = (uint32_t)(packed >> 32);
    argmax[0] = index >> (2u * depth); argmax[1] = (index >> depth) & mask; argmax[2] = index & mask;
}

}  // namespace

// ---- connected components --------------------------------------------------

extern "C" int vrc_volume_label_components(vrc_volume* medium, int connectivity, int through, vrc_labels** out, uint64_t* n_components)
{
    const char* what = "vrc_volume_label_components";
    if (!medium || !out) return vrc::fail(VRC_ERR_INVALID, "%s: null argument", what);
    if (const int rc = check_connectivity(what, connectivity)) return rc;
    if (const int rc = check_through(what, through)) return rc;
    vrc_labels* l = new (std::nothrow) vrc_labels();
    if (!l) return vrc::fail(VRC_ERR_OOM, "out of host memory");
    l->device = medium->device; l->depth = medium->depth;
    uint32_t C = 0;
    const int rc = snapshot_run(what, medium, nullptr, &l->d_ids, vrc::components_scratch_bytes(l->depth), [&](uint32_t* d_scratch) {
        vrc::components_roots_run(medium->d_bricks, l->depth, connectivity, through, nullptr, l->d_ids, d_scratch, nullptr);
        hipError_t run = hipGetLastError();
        if (run == hipSuccess) run = hipMemcpy(&C, vrc::components_total_slot(d_scratch, l->depth), 4, hipMemcpyDeviceToHost);
        if (run == hipSuccess && C) run = hipMalloc((void**)&l->d_records, (size_t)C * sizeof(vrc_component));
        if (run == hipSuccess && C) {
            vrc::components_ids_run(l->depth, l->d_ids, d_scratch, l->d_records, nullptr);
            run = hipGetLastError();
        }
        return run;
    });
    if (rc) {
        (void)vrc_labels_destroy(l);
        return rc;
    }
    l->count = C;
    *out = l;
    if (n_components) *n_components = C;
    return VRC_OK;
}

extern "C" int vrc_labels_destroy(vrc_labels* l)
{
    if (!l) return VRC_OK;
    (void)hipSetDevice(l->device);
    (void)hipDeviceSynchronize();       // device-memory calls may still be reading it on a caller's stream
    if (l->d_ids) (void)hipFree(l->d_ids);
    if (l->d_records) (void)hipFree(l->d_records);
    if (l->d_piece_cells) (void)hipFree(l->d_piece_cells);
    delete l;
    return VRC_OK;
}

extern "C" uint64_t vrc_labels_count(const vrc_labels* l) { return l ? l->count : 0; }
extern "C" uint32_t vrc_labels_depth(const vrc_labels* l) { return l ? l->depth : 0; }
extern "C" uint64_t vrc_labels_bytes(const vrc_labels* l)
{
    return l ? ((uint64_t)4u << (3u * l->depth)) + l->count * (sizeof(vrc_component) + (l->fractured ? 4u : 0u)) : 0;
}

extern "C" int vrc_labels_components(const vrc_labels* l, uint64_t first, uint64_t capacity, vrc_component* out, int mem, void* stream)
{
    const char* what = "vrc_labels_components";
    if (!l) return vrc::fail(VRC_ERR_INVALID, "%s: null labels", what);
    if (const int rc = check_mem(what, mem)) return rc;
    if (!out && capacity) return vrc::fail(VRC_ERR_INVALID, "%s: null buffer with capacity %llu", what, (unsigned long long)capacity);
    const uint64_t want = window_of(first, capacity, l->count);
    if (!want) return VRC_OK;
    // no list to stage: the records are copied out of the snapshot as they lie there
    const Call call = snapshot_call(l->device, mem, stream);
    return staged_call(what, call, [&]() {
        return hipMemcpyAsync(out, l->d_records + first, (size_t)want * sizeof(vrc_component), mem == VRC_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                              call.st);
    });
}

extern "C" int vrc_labels_at(const vrc_labels* l, uint64_t n, const uint32_t* xyz, uint32_t* ids, int mem, void* stream)
{
    const char* what = "vrc_labels_at";
    if (!l) return vrc::fail(VRC_ERR_INVALID, "%s: null labels", what);
    if (const int rc = check_mem(what, mem)) return rc;
    if (n == 0) return VRC_OK;
    if (!xyz || !ids) return vrc::fail(VRC_ERR_INVALID, "%s: null buffer", what);
    if (const int rc = check_count(what, n, LANE_ITEMS, "voxels")) return rc;
    const Call call = snapshot_call(l->device, mem, stream);
    const StagePart parts[] = {{xyz, (size_t)n * 12u, STAGE_IN}, {ids, (size_t)n * 4u, STAGE_OUT}};
    return staged_call(what, call, parts, [&](void* const* d) {
        vrc::components_at_run(l->d_ids, l->depth, n, (const uint32_t*)d[0], (uint32_t*)d[1], call.st);
        return hipSuccess;
    });
}

extern "C" int vrc_labels_select(const vrc_labels* l, const uint8_t* keep, vrc_volume* dst, int op, int mem, void* stream)
{
    const char* what = "vrc_labels_select";
    if (!l || !dst) return vrc::fail(VRC_ERR_INVALID, "%s: null argument", what);
    if (const int rc = check_op(what, op)) return rc;
    if (const int rc = check_mem(what, mem)) return rc;
    if (const int rc = check_same(what, "labels", l->depth, l->device, dst)) return rc;
    if (!keep && l->count) return vrc::fail(VRC_ERR_INVALID, "%s: null keep with %llu components", what, (unsigned long long)l->count);
    const Call call = volume_call(l->device, mem, stream, dst, true);
    const StagePart parts[] = {{keep, (size_t)l->count, STAGE_IN}};
    return staged_call(what, call, parts, [&](void* const* d) {
        vrc::components_select_run(l->d_ids, l->depth, (const uint8_t*)d[0], dst->d_bricks, op, call.st);
        return hipSuccess;
    });
}

// how far every piece can fall (the rule: include/vrc.h; the passes: vrc_fall.hip).  Synchronous, on the NULL stream.
// Not a staged_call: the scratch block is needed in both memory kinds and holds the staged offsets behind it, the rounds
// read a flag back between launches, and the offsets come down only from a run that converged.
extern "C" int vrc_fall_drops(const vrc_labels* l, vrc_volume* fixed, int direction, uint32_t drop_limit, int32_t* offsets, int mem, vrc_fall_stats* stats)
{
    const char* what = "vrc_fall_drops";
    if (!l) return vrc::fail(VRC_ERR_INVALID, "%s: null labels", what);
    if (direction < VRC_FACE_XN || direction > VRC_FACE_ZP) return vrc::fail(VRC_ERR_INVALID, "%s: direction %d is not a face code 0..5", what, direction);
    if (const int rc = check_mem(what, mem)) return rc;
    if (fixed)
        if (const int rc = check_same(what, "labels", l->depth, l->device, fixed)) return rc;
    if (!offsets && l->count) return vrc::fail(VRC_ERR_INVALID, "%s: null offsets with %llu components", what, (unsigned long long)l->count);
    vrc_fall_stats none = {};
    if (!stats) stats = &none;
    *stats = none;
    if (!l->count) return VRC_OK;
    const size_t scratch_bytes = vrc::fall_scratch_bytes(l->count), offset_bytes = (size_t)l->count * 12u;
    uint8_t* d_scratch = nullptr;
    uint32_t converged = 0;
    hipError_t e = hipSetDevice(l->device);
    if (e == hipSuccess && fixed) e = order_behind_edits(fixed, nullptr);
    if (e == hipSuccess) e = hipMalloc((void**)&d_scratch, scratch_bytes + (mem == VRC_MEM_HOST ? offset_bytes : 0u));
    int32_t* d_offsets = mem == VRC_MEM_HOST ? (int32_t*)(d_scratch + scratch_bytes) : offsets;
    if (e == hipSuccess)
        e = vrc::fall_run(l->d_ids, l->d_records, l->count, l->depth, fixed ? fixed->d_bricks : nullptr, direction, drop_limit, d_offsets, (uint32_t*)d_scratch,
                          nullptr, stats, &converged);
    if (e == hipSuccess && converged && mem == VRC_MEM_HOST) e = hipMemcpy(offsets, d_offsets, offset_bytes, hipMemcpyDeviceToHost);
    if (d_scratch) (void)hipFree(d_scratch);
    if (e != hipSuccess) return vrc::fail_hip(e, what);
    if (!converged) return vrc::fail(VRC_ERR_HIP, "%s: internal error: no fixed point within the bound of %u rounds", what, stats->rounds);
    return VRC_OK;
}

// every piece, moved by its own offset, into dst
extern "C" int vrc_fall_place(const vrc_labels* l, const uint8_t* keep, const int32_t* offsets, vrc_volume* dst, int op, int mem, void* stream)
{
    const char* what = "vrc_fall_place";
    if (!l || !dst) return vrc::fail(VRC_ERR_INVALID, "%s: null argument", what);
    if (const int rc = check_op(what, op)) return rc;
    if (op == VRC_COPY_REPLACE) return vrc::fail(VRC_ERR_INVALID, "%s: VRC_COPY_REPLACE has no meaning for a scatter", what);
    if (const int rc = check_mem(what, mem)) return rc;
    if (const int rc = check_same(what, "labels", l->depth, l->device, dst)) return rc;
    if (!offsets && l->count) return vrc::fail(VRC_ERR_INVALID, "%s: null offsets with %llu components", what, (unsigned long long)l->count);
    if (!l->count) return VRC_OK;
    const Call call = volume_call(l->device, mem, stream, dst, true);
    const StagePart parts[] = {{offsets, (size_t)l->count * 12u, STAGE_IN}, {keep, (size_t)l->count, STAGE_IN}};
    return staged_call(what, call, parts, [&](void* const* d) {
        vrc::place_run(l->d_ids, l->depth, (const uint8_t*)d[1], (const int32_t*)d[0], dst->d_bricks, op, call.st);
        return hipSuccess;
    });
}

// ---- the pieces as rigid bodies with a pose (the rules: include/vrc.h; the kernels: vrc_rigid.hip) ---------------

// maps in host memory are held to the limits of vrc_volume_stamp_affine here, maps in device memory by the kernel
static int check_affines(const char* what, uint64_t count, const vrc_affine* maps, int mem)
{
    if (mem == VRC_MEM_HOST)
        for (uint64_t i = 0; i < count; ++i)
            if (const int rc = check_affine(what, maps + i, (long long)i)) return rc;
    return VRC_OK;
}

extern "C" int vrc_rigid_moments(const vrc_labels* l, uint64_t first, uint64_t capacity, vrc_piece_moments* out, int mem, void* stream)
{
    const char* what = "vrc_rigid_moments";
    if (!l) return vrc::fail(VRC_ERR_INVALID, "%s: null labels", what);
    if (const int rc = check_mem(what, mem)) return rc;
    if (!out && capacity) return vrc::fail(VRC_ERR_INVALID, "%s: null buffer with capacity %llu", what, (unsigned long long)capacity);
    const uint64_t want = window_of(first, capacity, l->count);
    if (!want) return VRC_OK;
    const Call call = snapshot_call(l->device, mem, stream);
    const StagePart parts[] = {{out, (size_t)want * sizeof(vrc_piece_moments), STAGE_OUT}};
    return staged_call(what, call, parts, [&](void* const* d) { return vrc::moments_run(l->d_ids, l->depth, first, want, (vrc_piece_moments*)d[0], call.st); });
}

extern "C" int vrc_rigid_place_affine(const vrc_labels* l, const uint8_t* keep, const vrc_affine* maps, const uint32_t* boxes, vrc_volume* dst, int op, int mem,
                                      void* stream)
{
    const char* what = "vrc_rigid_place_affine";
    if (!l || !dst) return vrc::fail(VRC_ERR_INVALID, "%s: null argument", what);
    if (const int rc = check_op(what, op)) return rc;
    if (op == VRC_COPY_REPLACE) return vrc::fail(VRC_ERR_INVALID, "%s: VRC_COPY_REPLACE has no meaning where pieces may overlap", what);
    if (const int rc = check_mem(what, mem)) return rc;
    if (const int rc = check_same(what, "labels", l->depth, l->device, dst, false)) return rc;      // dst may have another depth
    if (!maps && l->count) return vrc::fail(VRC_ERR_INVALID, "%s: null maps with %llu components", what, (unsigned long long)l->count);
    if (const int rc = check_affines(what, l->count, maps, mem)) return rc;
    if (!l->count) return VRC_OK;
    const size_t C = (size_t)l->count;
    const Call call = volume_call(l->device, mem, stream, dst, true);
    const StagePart parts[] = {{maps, C * sizeof(vrc_affine), STAGE_IN}, {boxes, C * 24u, STAGE_IN}, {keep, C, STAGE_IN}};
    return staged_call(what, call, parts, [&](void* const* d) {
        vrc::place_affine_run(l->d_ids, l->d_records, l->count, l->depth, (const uint8_t*)d[2], (const vrc_affine*)d[0], (const uint32_t*)d[1], dst->d_bricks,
                              dst->depth, op, call.st);
        return hipSuccess;
    });
}

extern "C" int vrc_rigid_contacts(const vrc_labels* l, const uint8_t* keep, const vrc_affine* maps, const uint32_t* boxes, vrc_volume* world,
                                  vrc_piece_contact* out, int mem, void* stream)
{
    const char* what = "vrc_rigid_contacts";
    if (!l || !world) return vrc::fail(VRC_ERR_INVALID, "%s: null argument", what);
    if (const int rc = check_mem(what, mem)) return rc;
    if (const int rc = check_same(what, "labels", l->depth, l->device, world, false)) return rc;    // the world may have another depth
    if (!maps && l->count) return vrc::fail(VRC_ERR_INVALID, "%s: null maps with %llu components", what, (unsigned long long)l->count);
    if (!out && l->count) return vrc::fail(VRC_ERR_INVALID, "%s: null records with %llu components", what, (unsigned long long)l->count);
    if (const int rc = check_affines(what, l->count, maps, mem)) return rc;
    if (!l->count) return VRC_OK;
    const size_t C = (size_t)l->count;
    // the call reads the world's occupancy, as vrc_volume_count_boxes does: behind its last edit, not an edit itself
    const Call call = volume_call(l->device, mem, stream, world, false);
    const StagePart parts[] = {{out, C * sizeof(vrc_piece_contact), STAGE_OUT}, {maps, C * sizeof(vrc_affine), STAGE_IN}, {boxes, C * 24u, STAGE_IN}, {keep, C, STAGE_IN}};
    return staged_call(what, call, parts, [&](void* const* d) {
        return vrc::contacts_run(l->d_ids, l->d_records, l->count, l->depth, (const uint8_t*)d[3], (const vrc_affine*)d[1], (const uint32_t*)d[2], world->d_bricks,
                                 world->depth, (vrc_piece_contact*)d[0], call.st);
    });
}

static int check_posed_depth(const char* what, uint32_t posed_depth)
{
    return posed_depth >= 2 && posed_depth <= 10 ? VRC_OK : vrc::fail(VRC_ERR_INVALID, "%s: posed depth %u not in [2,10]", what, posed_depth);
}

extern "C" int vrc_rigid_pair_contacts(const vrc_labels* l, const uint8_t* keep, const vrc_affine* maps, const uint32_t* boxes, uint32_t posed_depth,
                                       uint64_t n_pairs, const uint32_t* pairs, vrc_piece_contact* out, int mem, void* stream)
{
    const char* what = "vrc_rigid_pair_contacts";
    if (!l) return vrc::fail(VRC_ERR_INVALID, "%s: null labels", what);
    if (const int rc = check_mem(what, mem)) return rc;
    if (const int rc = check_posed_depth(what, posed_depth)) return rc;
    if (!maps && l->count) return vrc::fail(VRC_ERR_INVALID, "%s: null maps with %llu components", what, (unsigned long long)l->count);
    if ((!pairs || !out) && n_pairs) return vrc::fail(VRC_ERR_INVALID, "%s: null %s with %llu pairs", what, pairs ? "records" : "pairs", (unsigned long long)n_pairs);
    if (n_pairs >= (1ull << 32)) return vrc::fail(VRC_ERR_INVALID, "%s: %llu pairs are too many (a pair's index is below 2^32)", what, (unsigned long long)n_pairs);
    if (!n_pairs || !l->count) return VRC_OK;
    if (const int rc = check_affines(what, l->count, maps, mem)) return rc;
    // pairs in host memory are held to the pieces here, pairs in device memory by the kernel
    if (mem == VRC_MEM_HOST)
        for (uint64_t k = 0; k < n_pairs; ++k)
            for (int side = 0; side < 2; ++side)
                if (pairs[2u * k + side] >= l->count)
                    return vrc::fail(VRC_ERR_INVALID, "%s: pair %llu: piece %u of %llu components", what, (unsigned long long)k, pairs[2u * k + side],
                                     (unsigned long long)l->count);
    const size_t C = (size_t)l->count, P = (size_t)n_pairs;
    const Call call = snapshot_call(l->device, mem, stream);
    const StagePart parts[] = {{out, P * sizeof(vrc_piece_contact), STAGE_OUT}, {maps, C * sizeof(vrc_affine), STAGE_IN}, {boxes, C * 24u, STAGE_IN},
                               {pairs, P * 8u, STAGE_IN}, {keep, C, STAGE_IN}};
    return staged_call(what, call, parts, [&](void* const* d) {
        return vrc::pair_contacts_run(l->d_ids, l->d_records, l->count, l->depth, (const uint8_t*)d[4], (const vrc_affine*)d[1], (const uint32_t*)d[2], posed_depth,
                                      n_pairs, (const uint32_t*)d[3], (vrc_piece_contact*)d[0], call.st);
    });
}

// The frame of the two broad-phase calls.  Not a staged_call: the scratch block is needed in both memory kinds and holds the
// staged boxes and keep behind it, the host reads the total back between the count and the emission, and a host-memory
// window comes down in pieces of at most 2^20 pairs.  Synchronous either way: the block is freed before return.
static int box_pair_call(const char* what, const vrc_labels* l, const uint8_t* keep, const uint32_t* boxes, uint32_t posed_depth, uint64_t* count, uint64_t first,
                         uint64_t capacity, uint32_t* pairs, int mem, void* stream)
{
    if (!l) return vrc::fail(VRC_ERR_INVALID, "%s: null labels", what);
    if (const int rc = check_mem(what, mem)) return rc;
    if (const int rc = check_posed_depth(what, posed_depth)) return rc;
    if (!boxes && l->count) return vrc::fail(VRC_ERR_INVALID, "%s: null boxes with %llu components", what, (unsigned long long)l->count);
    if (l->count > vrc::BOX_PAIR_PIECES)
        return vrc::fail(VRC_ERR_INVALID, "%s: %llu components are too many for a pass of C^2 box tests (at most 2^20)", what, (unsigned long long)l->count);
    if (count) *count = 0;
    if (!l->count || (!count && !capacity)) return VRC_OK;
    const bool host = mem == VRC_MEM_HOST;
    const size_t C = (size_t)l->count, slot_bytes = (vrc::box_pair_scratch_bytes(C) + 15u) & ~(size_t)15u, box_bytes = (C * 24u + 15u) & ~(size_t)15u;
    const uint64_t chunk = 1ull << 20;
    hipStream_t st = (hipStream_t)stream;
    uint8_t* block = nullptr;
    uint32_t* d_window = nullptr;
    hipError_t e = hipSetDevice(l->device);
    if (e == hipSuccess) e = hipMalloc((void**)&block, slot_bytes + (host ? box_bytes + C : 0u));
    unsigned long long* slots = (unsigned long long*)block;
    const uint32_t* d_boxes = boxes;
    const uint8_t* d_keep = keep;
    if (host && e == hipSuccess) {
        d_boxes = (const uint32_t*)(block + slot_bytes);
        e = hipMemcpyAsync((void*)d_boxes, boxes, C * 24u, hipMemcpyHostToDevice, st);
        if (keep && e == hipSuccess) {
            d_keep = block + slot_bytes + box_bytes;
            e = hipMemcpyAsync((void*)d_keep, keep, C, hipMemcpyHostToDevice, st);
        }
    }
    unsigned long long total = 0;
    if (e == hipSuccess) {
        vrc::box_pair_count_run(d_keep, d_boxes, C, posed_depth, slots, st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&total, slots + C, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    const uint64_t want = e == hipSuccess ? window_of(first, capacity, total) : 0u;
    if (want && !host) {
        vrc::box_pairs_run(d_keep, d_boxes, C, posed_depth, slots, first, want, pairs, st);
        e = hipGetLastError();
    } else if (want) {
        e = hipMalloc((void**)&d_window, (size_t)(want < chunk ? want : chunk) * 8u);
        for (uint64_t at = 0; at < want && e == hipSuccess; at += chunk) {
            const uint64_t now = want - at < chunk ? want - at : chunk;
            vrc::box_pairs_run(d_keep, d_boxes, C, posed_depth, slots, first + at, now, d_window, st);
            if ((e = hipGetLastError()) == hipSuccess) e = hipMemcpyAsync(pairs + 2u * at, d_window, (size_t)now * 8u, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (d_window) (void)hipFree(d_window);
    if (block) (void)hipFree(block);
    if (e != hipSuccess) return vrc::fail_hip(e, what);
    if (count) *count = total;
    return VRC_OK;
}

extern "C" int vrc_rigid_box_pair_count(const vrc_labels* l, const uint8_t* keep, const uint32_t* boxes, uint32_t posed_depth, uint64_t* count, int mem, void* stream)
{
    const char* what = "vrc_rigid_box_pair_count";
    if (!count) return vrc::fail(VRC_ERR_INVALID, "%s: null count", what);
    return box_pair_call(what, l, keep, boxes, posed_depth, count, 0, 0, nullptr, mem, stream);
}

extern "C" int vrc_rigid_box_pairs(const vrc_labels* l, const uint8_t* keep, const uint32_t* boxes, uint32_t posed_depth, uint64_t first, uint64_t capacity,
                                   uint32_t* pairs, int mem, void* stream)
{
    const char* what = "vrc_rigid_box_pairs";
    if (!pairs && capacity) return vrc::fail(VRC_ERR_INVALID, "%s: null buffer with capacity %llu", what, (unsigned long long)capacity);
    return box_pair_call(what, l, keep, boxes, posed_depth, nullptr, first, capacity, pairs, mem, stream);
}

// ---- Voronoi fracture (the rule: include/vrc.h; the cells: vrc_fracture.hip; the labelling: vrc_components.hip) ------

// One scratch block for the call: the labelling's counts, the dense cell field, the site table and the stacks, and behind
// them the staged sites of a host-memory call.  Not a staged_call: the host reads C back between the two halves.
extern "C" int vrc_fracture_label(vrc_volume* medium, int connectivity, int through, uint64_t n_sites, const int32_t* sites_xyz, uint32_t max_d2, int mem,
                                  vrc_labels** out, uint64_t* n_components)
{
    const char* what = "vrc_fracture_label";
    if (!medium || !out) return vrc::fail(VRC_ERR_INVALID, "%s: null argument", what);
    if (const int rc = check_connectivity(what, connectivity)) return rc;
    if (const int rc = check_through(what, through)) return rc;
    if (const int rc = check_mem(what, mem)) return rc;
    if (n_sites == 0) return vrc::fail(VRC_ERR_INVALID, "%s: no sites", what);
    if (!sites_xyz) return vrc::fail(VRC_ERR_INVALID, "%s: null sites", what);
    if (n_sites >= 0xffffffffull) return vrc::fail(VRC_ERR_INVALID, "%s: %llu sites are too many (an index is below 2^32 - 1)", what, (unsigned long long)n_sites);
    if (medium->depth < 2 || medium->depth > 10) return vrc::fail(VRC_ERR_INVALID, "%s: depth %u not in [2,10]", what, medium->depth);
    vrc_labels* l = new (std::nothrow) vrc_labels();
    if (!l) return vrc::fail(VRC_ERR_OOM, "out of host memory");
    l->device = medium->device; l->depth = medium->depth; l->fractured = true;
    const size_t label_bytes = (vrc::components_scratch_bytes(l->depth) + 15u) & ~(size_t)15u, cell_bytes = (size_t)4u << (3u * l->depth);
    const size_t work_bytes = vrc::fracture_scratch_bytes(l->depth, medium->cu_count, n_sites), site_bytes = (size_t)n_sites * 12u;
    uint32_t C = 0;
    const int rc = snapshot_run(what, medium, nullptr, &l->d_ids, label_bytes + cell_bytes + work_bytes + (mem == VRC_MEM_HOST ? site_bytes : 0u), [&](uint32_t* d_scratch) {
        uint32_t* d_cells = d_scratch + label_bytes / 4u;
        uint32_t* d_work = d_cells + cell_bytes / 4u;
        const int32_t* d_sites = sites_xyz;
        hipError_t run = hipSuccess;
        if (mem == VRC_MEM_HOST) {
            d_sites = (const int32_t*)(d_work + work_bytes / 4u);
            run = hipMemcpyAsync((void*)d_sites, sites_xyz, site_bytes, hipMemcpyHostToDevice, nullptr);
        }
        if (run == hipSuccess) {
            vrc::fracture_cells_run(d_sites, n_sites, l->depth, max_d2, medium->cu_count, d_cells, d_work, nullptr);
            vrc::components_roots_run(medium->d_bricks, l->depth, connectivity, through, d_cells, l->d_ids, d_scratch, nullptr);
            run = hipGetLastError();
        }
        if (run == hipSuccess) run = hipMemcpy(&C, vrc::components_total_slot(d_scratch, l->depth), 4, hipMemcpyDeviceToHost);
        if (run == hipSuccess && C) run = hipMalloc((void**)&l->d_records, (size_t)C * sizeof(vrc_component));
        if (run == hipSuccess && C) run = hipMalloc((void**)&l->d_piece_cells, (size_t)C * 4u);
        if (run == hipSuccess && C) {
            vrc::components_ids_run(l->depth, l->d_ids, d_scratch, l->d_records, nullptr);
            vrc::fracture_piece_cells_run(l->d_records, C, d_cells, l->depth, l->d_piece_cells, nullptr);
            run = hipGetLastError();
        }
        return run;
    });
    if (rc) {
        (void)vrc_labels_destroy(l);
        return rc;
    }
    l->count = C;
    *out = l;
    if (n_components) *n_components = C;
    return VRC_OK;
}

extern "C" int vrc_fracture_piece_sites(const vrc_labels* l, uint64_t first, uint64_t capacity, uint32_t* sites, int mem, void* stream)
{
    const char* what = "vrc_fracture_piece_sites";
    if (!l) return vrc::fail(VRC_ERR_INVALID, "%s: null labels", what);
    if (!l->fractured) return vrc::fail(VRC_ERR_INVALID, "%s: not fracture labels (the pieces of vrc_volume_label_components have no cell)", what);
    if (const int rc = check_mem(what, mem)) return rc;
    if (!sites && capacity) return vrc::fail(VRC_ERR_INVALID, "%s: null buffer with capacity %llu", what, (unsigned long long)capacity);
    const uint64_t want = window_of(first, capacity, l->count);
    if (!want) return VRC_OK;
    const Call call = snapshot_call(l->device, mem, stream);
    const StagePart parts[] = {{sites, (size_t)want * 4u, STAGE_OUT}};
    return staged_call(what, call, parts, [&](void* const* d) {
        return hipMemcpyAsync(d[0], l->d_piece_cells + first, (size_t)want * 4u, hipMemcpyDeviceToDevice, call.st);
    });
}

// ---- distance field ----------------------------------------------------------

extern "C" int vrc_volume_distance_field(vrc_volume* medium, int to, int outside, vrc_distance** out, vrc_distance_stats* stats)
{
    const char* what = "vrc_volume_distance_field";
    if (!medium || !out) return vrc::fail(VRC_ERR_INVALID, "%s: null argument", what);
    if (to != VRC_FLOOD_SOLID && to != VRC_FLOOD_EMPTY) return vrc::fail(VRC_ERR_INVALID, "%s: bad to %d", what, to);
    if (medium->depth < 2 || medium->depth > 10) return vrc::fail(VRC_ERR_INVALID, "%s: depth %u not in [2,10]", what, medium->depth);
    vrc_distance* d = new (std::nothrow) vrc_distance();
    if (!d) return vrc::fail(VRC_ERR_OOM, "out of host memory");
    d->device = medium->device; d->depth = medium->depth; d->euclidean = true;
    unsigned long long host[2] = {0ull, 0ull};
    const int rc = snapshot_run(what, medium, nullptr, &d->d_field, vrc::distance_scratch_bytes(d->depth, medium->cu_count), [&](uint32_t* d_scratch) {
        vrc::distance_run(medium->d_bricks, d->depth, to, outside, medium->cu_count, d->d_field, d_scratch, nullptr);
        const hipError_t run = hipGetLastError();
        return run != hipSuccess ? run : hipMemcpy(host, vrc::distance_stats_slots(d_scratch), sizeof host, hipMemcpyDeviceToHost);
    });
    if (rc) {
        (void)vrc_distance_destroy(d);
        return rc;
    }
    if (stats) {
        stats->features = host[0]; stats->reserved = 0u;
        decode_argmax(host[1], d->depth, &stats->max_d2, stats->argmax);
    }
    *out = d;
    return VRC_OK;
}

extern "C" int vrc_distance_destroy(vrc_distance* d)
{
    if (!d) return VRC_OK;
    (void)hipSetDevice(d->device);
    (void)hipDeviceSynchronize();       // device-memory calls may still be reading it on a caller's stream
    if (d->d_field) (void)hipFree(d->d_field);
    delete d;
    return VRC_OK;
}

extern "C" uint32_t vrc_distance_depth(const vrc_distance* d) { return d ? d->depth : 0; }
extern "C" uint64_t vrc_distance_bytes(const vrc_distance* d) { return d ? (uint64_t)4u << (3u * d->depth) : 0; }
extern "C" const uint32_t* vrc_distance_data(const vrc_distance* d) { return d ? d->d_field : nullptr; }
extern "C" int vrc_travel_connectivity(const vrc_distance* d) { return d ? d->connectivity : 0; }

extern "C" int vrc_distance_at(const vrc_distance* d, uint64_t n, const uint32_t* xyz, uint32_t* d2, int mem, void* stream)
{
    const char* what = "vrc_distance_at";
    if (!d) return vrc::fail(VRC_ERR_INVALID, "%s: null distance field", what);
    if (const int rc = check_mem(what, mem)) return rc;
    if (n == 0) return VRC_OK;
    if (!xyz || !d2) return vrc::fail(VRC_ERR_INVALID, "%s: null buffer", what);
    if (const int rc = check_count(what, n, LANE_ITEMS, "voxels")) return rc;
    const Call call = snapshot_call(d->device, mem, stream);
    const StagePart parts[] = {{xyz, (size_t)n * 12u, STAGE_IN}, {d2, (size_t)n * 4u, STAGE_OUT}};
    return staged_call(what, call, parts, [&](void* const* p) {
        vrc::distance_at_run(d->d_field, d->depth, n, (const uint32_t*)p[0], (uint32_t*)p[1], call.st);
        return hipSuccess;
    });
}

extern "C" int vrc_distance_download(const vrc_distance* d, uint32_t* d2_host)
{
    const char* what = "vrc_distance_download";
    if (!d || !d2_host) return vrc::fail(VRC_ERR_INVALID, "%s: null argument", what);
    hipError_t e = hipSetDevice(d->device);
    if (e == hipSuccess) e = hipMemcpy(d2_host, d->d_field, (size_t)4u << (3u * d->depth), hipMemcpyDeviceToHost);
    return done(e, what);
}

extern "C" int vrc_distance_select(const vrc_distance* d, uint32_t lo, uint32_t hi, vrc_volume* dst, int op, void* stream)
{
    const char* what = "vrc_distance_select";
    if (!d || !dst) return vrc::fail(VRC_ERR_INVALID, "%s: null argument", what);
    if (const int rc = check_op(what, op)) return rc;
    if (lo > hi) return vrc::fail(VRC_ERR_INVALID, "%s: lo %u above hi %u", what, lo, hi);
    if (const int rc = check_same(what, "field", d->depth, d->device, dst)) return rc;
    const Call call = volume_call(d->device, VRC_MEM_DEVICE, stream, dst, true);
    return staged_call(what, call, [&]() {
        vrc::distance_select_run(d->d_field, d->depth, lo, hi, dst->d_bricks, op, call.st);
        return hipSuccess;
    });
}

// ---- travel-distance field -----------------------------------------------------

extern "C" int vrc_travel_field(vrc_volume* seeds, vrc_volume* medium, int connectivity, int through, uint32_t step_limit, vrc_distance** out,
                                       vrc_travel_stats* stats)
{
    const char* what = "vrc_travel_field";
    if (!seeds || !medium) return vrc::fail(VRC_ERR_INVALID, "%s: null volume", what);
    if (!out) return vrc::fail(VRC_ERR_INVALID, "%s: null argument", what);
    if (const int rc = check_connectivity(what, connectivity)) return rc;
    if (const int rc = check_through(what, through)) return rc;
    if (seeds != medium)                                                // one volume twice is allowed: seeds within their own medium
        if (const int rc = check_pair(what, seeds, medium, true)) return rc;
    if (medium->depth < 2 || medium->depth > 10) return vrc::fail(VRC_ERR_INVALID, "%s: depth %u not in [2,10]", what, medium->depth);
    vrc_distance* d = new (std::nothrow) vrc_distance();
    if (!d) return vrc::fail(VRC_ERR_OOM, "out of host memory");
    d->device = medium->device; d->depth = medium->depth; d->connectivity = connectivity;
    unsigned long long host[3] = {0ull, 0ull, 0ull};
    uint32_t sweeps = 0, converged = 0;
    const int rc = snapshot_run(what, medium, seeds, &d->d_field, vrc::travel_scratch_bytes(d->depth), [&](uint32_t* d_scratch) {
        const hipError_t run = vrc::travel_run(seeds->d_bricks, medium->d_bricks, d->depth, connectivity, through, step_limit, d->d_field, d_scratch, nullptr,
                                               &sweeps, &converged);
        return run != hipSuccess ? run : hipMemcpy(host, vrc::travel_stats_slots(d_scratch), sizeof host, hipMemcpyDeviceToHost);
    });
    if (rc) {
        (void)vrc_distance_destroy(d);
        return rc;
    }
    if (!converged) {
        (void)vrc_distance_destroy(d);
        return vrc::fail(VRC_ERR_HIP, "%s: internal error: no fixed point within the bound of %u sweeps", what, sweeps);
    }
    if (stats) {
        stats->seeds = host[0]; stats->reached = host[1]; stats->sweeps = sweeps; stats->reserved = 0u;
        decode_argmax(host[2], d->depth, &stats->max_steps, stats->argmax);
    }
    *out = d;
    return VRC_OK;
}

extern "C" int vrc_travel_trace_paths(const vrc_distance* d, uint64_t n, const uint32_t* start_xyz, uint32_t capacity, uint32_t* paths_xyz,
                                        uint32_t* lengths, int mem, void* stream)
{
    const char* what = "vrc_travel_trace_paths";
    if (!d) return vrc::fail(VRC_ERR_INVALID, "%s: null distance field", what);
    if (d->connectivity != VRC_CONNECT_FACES && d->connectivity != VRC_CONNECT_ALL)
        return vrc::fail(VRC_ERR_INVALID, "%s: not a travel field (a Euclidean field has no routes)", what);
    if (const int rc = check_mem(what, mem)) return rc;
    if (n == 0) return VRC_OK;
    if (!start_xyz || !lengths) return vrc::fail(VRC_ERR_INVALID, "%s: null buffer", what);
    if (!paths_xyz && capacity) return vrc::fail(VRC_ERR_INVALID, "%s: null paths with capacity %u", what, capacity);
    if (const int rc = check_count(what, n, LANE_ITEMS, "starts")) return rc;
    if (capacity && n > (1ull << 58) / capacity) return vrc::fail(VRC_ERR_INVALID, "%s: %llu routes of capacity %u are too many", what, (unsigned long long)n, capacity);
    const Call call = snapshot_call(d->device, mem, stream);
    // the caller's paths go up first, so that what the kernel leaves alone comes back as it was
    const StagePart parts[] = {{start_xyz, (size_t)n * 12u, STAGE_IN}, {lengths, (size_t)n * 4u, STAGE_OUT}, {paths_xyz, (size_t)n * capacity * 12u, STAGE_INOUT}};
    return staged_call(what, call, parts, [&](void* const* p) {
        vrc::travel_trace_run(d->d_field, d->depth, d->connectivity, n, (const uint32_t*)p[0], capacity, (uint32_t*)p[2], (uint32_t*)p[1], call.st);
        return hipSuccess;
    });
}

// ---- straight-line walks over a field (the rule: include/vrc.h; the kernels: vrc_sight.hip) ---------------------------

// what both sight calls refuse alike
static int check_sight(const char* what, uint32_t lo, uint32_t hi, int flags)
{
    if (lo > hi) return vrc::fail(VRC_ERR_INVALID, "%s: lo %u above hi %u", what, lo, hi);
    if (flags & ~(VRC_SIGHT_TOUCH | VRC_SIGHT_PLAIN)) return vrc::fail(VRC_ERR_INVALID, "%s: unknown flag bits in %d", what, flags);
    return VRC_OK;
}

// The stride needs the free radius that only a distance to a set holds, and a band without an upper end.  A sight field has
// connectivity 0 as well, but its values are no such distance (NONE in every shadow, small next to the eye): it walks plainly.
static bool sight_strides(const vrc_distance* d, uint32_t hi, int flags) { return d->euclidean && hi == 0xffffffffu && !(flags & VRC_SIGHT_PLAIN); }

extern "C" int vrc_sight_segments(const vrc_distance* d, uint64_t n, const int32_t* segments, uint32_t lo, uint32_t hi, int flags, vrc_sight* out, int mem,
                                  void* stream)
{
    const char* what = "vrc_sight_segments";
    if (!d) return vrc::fail(VRC_ERR_INVALID, "%s: null distance field", what);
    if (const int rc = check_mem(what, mem)) return rc;
    if (const int rc = check_sight(what, lo, hi, flags)) return rc;
    if (n == 0) return VRC_OK;
    if (!segments || !out) return vrc::fail(VRC_ERR_INVALID, "%s: null buffer", what);
    if (const int rc = check_count(what, n, LANE_ITEMS, "segments")) return rc;
    const Call call = snapshot_call(d->device, mem, stream);
    const StagePart parts[] = {{out, (size_t)n * sizeof(vrc_sight), STAGE_OUT}, {segments, (size_t)n * 24u, STAGE_IN}};
    return staged_call(what, call, parts, [&](void* const* p) {
        vrc::sight_segments_run(d->d_field, d->depth, n, (const int32_t*)p[1], lo, hi, (flags & VRC_SIGHT_TOUCH) != 0, sight_strides(d, hi, flags),
                                (vrc_sight*)p[0], call.st);
        return hipSuccess;
    });
}

// A creator without a volume: the NULL stream, nothing to order behind.  The field and the 16 bytes of stats are allocated
// inside the frame; the blocking read-back of the stats has synchronised when it returns.
extern "C" int vrc_sight_field(const vrc_distance* d, const uint32_t eye[3], uint32_t radius, uint32_t lo, uint32_t hi, int flags, vrc_distance** out,
                               vrc_sight_stats* stats)
{
    const char* what = "vrc_sight_field";
    if (!d || !out || !eye) return vrc::fail(VRC_ERR_INVALID, "%s: null argument", what);
    if (const int rc = check_sight(what, lo, hi, flags)) return rc;
    const uint32_t S = 1u << d->depth;
    if (eye[0] >= S || eye[1] >= S || eye[2] >= S) return vrc::fail(VRC_ERR_INVALID, "%s: eye %u %u %u outside the volume of %u^3", what, eye[0], eye[1], eye[2], S);
    vrc_distance* f = new (std::nothrow) vrc_distance();
    if (!f) return vrc::fail(VRC_ERR_OOM, "out of host memory");
    f->device = d->device; f->depth = d->depth;
    unsigned long long* d_stats = nullptr;
    unsigned long long host[2] = {0ull, 0ull};
    const int rc = staged_call(what, snapshot_call(d->device, VRC_MEM_DEVICE, nullptr), [&]() {
        hipError_t e = hipMalloc((void**)&f->d_field, (size_t)4u << (3u * f->depth));
        if (e == hipSuccess) e = hipMalloc((void**)&d_stats, sizeof host);
        if (e == hipSuccess) e = hipMemsetAsync(d_stats, 0, sizeof host, nullptr);
        if (e != hipSuccess) return e;
        vrc::sight_field_run(d->d_field, d->depth, eye, radius, lo, hi, (flags & VRC_SIGHT_TOUCH) != 0, sight_strides(d, hi, flags), f->d_field, d_stats, nullptr);
        e = hipGetLastError();
        return e != hipSuccess ? e : hipMemcpy(host, d_stats, sizeof host, hipMemcpyDeviceToHost);
    });
    if (d_stats) (void)hipFree(d_stats);
    if (rc) {
        (void)vrc_distance_destroy(f);
        return rc;
    }
    if (stats) {
        stats->visible = host[0]; stats->reserved = 0u;
        decode_argmax(host[1], f->depth, &stats->max_d2, stats->argmax);
    }
    *out = f;
    return VRC_OK;
}

// ---- a field read at the voxels of every posed piece (the rule: include/vrc.h; the kernels: vrc_rigid.hip) ---------

extern "C" int vrc_rigid_clearance(const vrc_labels* l, const uint8_t* keep, const vrc_affine* maps, const uint32_t* boxes, const vrc_distance* field,
                                   vrc_piece_clearance* out, int mem, void* stream)
{
    const char* what = "vrc_rigid_clearance";
    if (!l || !field) return vrc::fail(VRC_ERR_INVALID, "%s: null argument", what);
    if (const int rc = check_mem(what, mem)) return rc;
    if (field->device != l->device) return vrc::fail(VRC_ERR_INVALID, "%s: labels on device %d, field on device %d", what, l->device, field->device);
    if (!maps && l->count) return vrc::fail(VRC_ERR_INVALID, "%s: null maps with %llu components", what, (unsigned long long)l->count);
    if (!out && l->count) return vrc::fail(VRC_ERR_INVALID, "%s: null records with %llu components", what, (unsigned long long)l->count);
    if (const int rc = check_affines(what, l->count, maps, mem)) return rc;
    if (!l->count) return VRC_OK;
    const size_t C = (size_t)l->count;
    // both are snapshots, never written after creation: there is no edit to wait for
    const Call call = snapshot_call(l->device, mem, stream);
    const StagePart parts[] = {{out, C * sizeof(vrc_piece_clearance), STAGE_OUT}, {maps, C * sizeof(vrc_affine), STAGE_IN}, {boxes, C * 24u, STAGE_IN}, {keep, C, STAGE_IN}};
    return staged_call(what, call, parts, [&](void* const* d) {
        return vrc::clearance_run(l->d_ids, l->d_records, l->count, l->depth, (const uint8_t*)d[3], (const vrc_affine*)d[1], (const uint32_t*)d[2], field->d_field,
                                  field->depth, (vrc_piece_clearance*)d[0], call.st);
    });
}

// ---- deltas: the changed words of two volumes (the rule: include/vrc.h; the kernels: vrc_delta.hip) -----------------

struct vrc_delta {
    int device = 0;
    uint32_t depth = 0;
    uint64_t count = 0;
    uint2* d_records = nullptr;           // count records {word, bits}, nullptr when count == 0
    vrc_delta_stats stats = {};
};

// what the passes reduced, as the stats of a list of `words` records
static vrc_delta_stats delta_stats_of(const vrc::DeltaTotals& t, uint64_t words)
{
    vrc_delta_stats s = {};
    s.words = words;
    s.voxels = t.voxels;
    for (int a = 0; a < 3 && words; ++a) { s.lo[a] = t.lo[a]; s.hi[a] = t.hi[a]; }
    return s;
}

// Not a snapshot_run: the array is sized by what the host reads back between scan and emit.
extern "C" int vrc_delta_diff(vrc_volume* before, vrc_volume* after, vrc_delta** out, vrc_delta_stats* stats)
{
    const char* what = "vrc_delta_diff";
    if (!before || !after || !out) return vrc::fail(VRC_ERR_INVALID, "%s: null argument", what);
    if (before == after) return vrc::fail(VRC_ERR_INVALID, "%s: before and after are the same volume", what);
    if (const int rc = check_pair(what, before, after, true)) return rc;
    vrc_delta* d = new (std::nothrow) vrc_delta();
    if (!d) return vrc::fail(VRC_ERR_OOM, "out of host memory");
    d->device = before->device; d->depth = before->depth;
    void* d_scratch = nullptr;
    vrc::DeltaTotals totals = {};
    const int rc = staged_call(what, null_stream_call(after, before, false, true), [&]() {
        hipError_t e = hipMalloc(&d_scratch, vrc::delta_scratch_bytes(d->depth));
        if (e == hipSuccess) {
            vrc::delta_offsets_run(before->d_bricks, after->d_bricks, d->depth, d_scratch, nullptr);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpy(&totals, d_scratch, sizeof totals, hipMemcpyDeviceToHost);
        if (e == hipSuccess && totals.words) e = hipMalloc((void**)&d->d_records, (size_t)totals.words * 8u);
        if (e == hipSuccess && totals.words) vrc::delta_emit_run(before->d_bricks, after->d_bricks, d->depth, d_scratch, d->d_records, nullptr);
        return e;
    });
    if (d_scratch) (void)hipFree(d_scratch);
    if (rc) {
        (void)vrc_delta_destroy(d);
        return rc;
    }
    d->count = totals.words;
    d->stats = delta_stats_of(totals, d->count);
    if (stats) *stats = d->stats;
    *out = d;
    return VRC_OK;
}

extern "C" int vrc_delta_create(uint32_t depth, int device, uint64_t n, const uint32_t* records, int mem, vrc_delta** out, vrc_delta_stats* stats)
{
    const char* what = "vrc_delta_create";
    if (!out) return vrc::fail(VRC_ERR_INVALID, "%s: null argument", what);
    if (depth < 2 || depth > 10) return vrc::fail(VRC_ERR_INVALID, "%s: depth %u not in [2,10]", what, depth);
    if (const int rc = check_mem(what, mem)) return rc;
    if (!records && n) return vrc::fail(VRC_ERR_INVALID, "%s: null records with n = %llu", what, (unsigned long long)n);
    if (const int rc = vrc::require_device(device, nullptr)) return rc;
    vrc_delta* d = new (std::nothrow) vrc_delta();
    if (!d) return vrc::fail(VRC_ERR_OOM, "out of host memory");
    d->device = device; d->depth = depth;
    // a list longer than the field has words breaks the rule within its first n_words + 1 records: those are looked at
    const uint32_t n_words = vrc::delta_words(depth), n_check = (uint32_t)(n <= n_words ? n : n_words + 1u);
    vrc::DeltaTotals* d_totals = nullptr;
    vrc::DeltaTotals totals = {};
    uint2 bad[2] = {};
    hipError_t e = hipMalloc((void**)&d_totals, sizeof totals);
    if (e == hipSuccess && n_check) e = hipMalloc((void**)&d->d_records, (size_t)n_check * 8u);
    if (e == hipSuccess && n_check)
        e = hipMemcpyAsync(d->d_records, records, (size_t)n_check * 8u, mem == VRC_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, nullptr);
    if (e == hipSuccess) {
        vrc::delta_check_run(d->d_records, n_check, depth, d_totals, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(&totals, d_totals, sizeof totals, hipMemcpyDeviceToHost);
    const bool refused = e == hipSuccess && (totals.first_bad != 0xffffffffu || n > n_words);
    if (refused && totals.first_bad < n_check) {
        const uint32_t from = totals.first_bad ? totals.first_bad - 1u : 0u;
        e = hipMemcpy(bad, d->d_records + from, totals.first_bad ? 16u : 8u, hipMemcpyDeviceToHost);
        if (!totals.first_bad) bad[1] = bad[0];
    }
    if (d_totals) (void)hipFree(d_totals);
    if (e != hipSuccess || refused) (void)vrc_delta_destroy(d);
    if (e != hipSuccess) return vrc::fail_hip(e, what);
    if (refused) {
        const unsigned long long i = totals.first_bad;
        if (totals.first_bad >= n_check) return vrc::fail(VRC_ERR_INVALID, "%s: %llu records for the %u words of depth %u", what, (unsigned long long)n, n_words, depth);
        if (bad[1].y == 0u) return vrc::fail(VRC_ERR_INVALID, "%s: record %llu (word %u): bits are 0", what, i, bad[1].x);
        if (bad[1].x >= n_words) return vrc::fail(VRC_ERR_INVALID, "%s: record %llu: word %u beyond the %u words of depth %u", what, i, bad[1].x, n_words, depth);
        return vrc::fail(VRC_ERR_INVALID, "%s: record %llu: word %u is not above word %u of the record before it", what, i, bad[1].x, bad[0].x);
    }
    d->count = n;
    d->stats = delta_stats_of(totals, n);
    if (stats) *stats = d->stats;
    *out = d;
    return VRC_OK;
}

extern "C" int vrc_delta_destroy(vrc_delta* d)
{
    if (!d) return VRC_OK;
    (void)hipSetDevice(d->device);
    (void)hipDeviceSynchronize();       // an apply or a device-memory window may still be reading it on a caller's stream
    if (d->d_records) (void)hipFree(d->d_records);
    delete d;
    return VRC_OK;
}

extern "C" uint64_t vrc_delta_count(const vrc_delta* d) { return d ? d->count : 0; }
extern "C" uint32_t vrc_delta_depth(const vrc_delta* d) { return d ? d->depth : 0; }
extern "C" uint64_t vrc_delta_bytes(const vrc_delta* d) { return d ? d->count * 8u : 0; }

extern "C" int vrc_delta_get_stats(const vrc_delta* d, vrc_delta_stats* out)
{
    if (!d || !out) return vrc::fail(VRC_ERR_INVALID, "vrc_delta_get_stats: null argument");
    *out = d->stats;
    return VRC_OK;
}

extern "C" int vrc_delta_records(const vrc_delta* d, uint64_t first, uint64_t capacity, uint32_t* out, int mem, void* stream)
{
    const char* what = "vrc_delta_records";
    if (!d) return vrc::fail(VRC_ERR_INVALID, "%s: null delta", what);
    if (const int rc = check_mem(what, mem)) return rc;
    if (!out && capacity) return vrc::fail(VRC_ERR_INVALID, "%s: null buffer with capacity %llu", what, (unsigned long long)capacity);
    const uint64_t want = window_of(first, capacity, d->count);
    if (!want) return VRC_OK;
    const Call call = snapshot_call(d->device, mem, stream);
    const StagePart parts[] = {{out, (size_t)want * 8u, STAGE_OUT}};
    return staged_call(what, call, parts, [&](void* const* p) {
        return hipMemcpyAsync(p[0], d->d_records + first, (size_t)want * 8u, hipMemcpyDeviceToDevice, call.st);
    });
}

extern "C" int vrc_delta_apply(const vrc_delta* d, vrc_volume* dst, void* stream)
{
    const char* what = "vrc_delta_apply";
    if (!d || !dst) return vrc::fail(VRC_ERR_INVALID, "%s: null argument", what);
    if (const int rc = check_same(what, "delta", d->depth, d->device, dst)) return rc;
    if (!d->count) return VRC_OK;
    const Call call = volume_call(d->device, VRC_MEM_DEVICE, stream, dst, true);
    return staged_call(what, call, [&]() {
        vrc::delta_apply_run(d->d_records, (uint32_t)d->count, dst->d_bricks, call.st);
        return hipSuccess;
    });
}
