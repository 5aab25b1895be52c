// vrc_snapshots.hip -- the snapshots taken from an editable volume (include/vrc.h): the labels of its connected components
// (vrc_volume_label_components, vrc_labels_*; kernels in vrc_components.hip; the pieces' moments, posed placement and
// contacts, vrc_rigid_*, kernels in vrc_rigid.hip) and its exact squared Euclidean distance field
// with the selection by distance that grow / shrink / hollow are made of (vrc_volume_distance_field, vrc_distance_*;
// kernels in vrc_distance.hip), and the travel-distance field from a set of seeds, kept in the same snapshot object, with the
// routes read off it (vrc_travel_field, vrc_travel_trace_paths; kernels in vrc_travel.hip).  A snapshot owns its memory, is never written after its creator returns, and keeps no
// event and no scratch; what it selects goes into a volume as an edit of that volume (vrc_volume_state.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <new>

#include "../../include/vrc.h"
#include "vrc_components.h"
#include "vrc_distance.h"
#include "vrc_fall.h"
#include "vrc_rigid.h"
#include "vrc_travel.h"
#include "vrc_volume_state.h"

struct vrc_labels {
    int device = 0;
    uint32_t depth = 0;
    uint64_t count = 0;
    uint32_t* d_ids = nullptr;            // 8^depth ids, indexed by key
    vrc_component* d_records = nullptr;   // count records, nullptr when count == 0
};

struct vrc_distance {
    int device = 0;
    uint32_t depth = 0;
    int connectivity = 0;                 // 6 / 26: a travel field made with it; 0: a Euclidean field
    uint32_t* d_field = nullptr;          // 8^depth squared distances (travel field: steps), [(x*S + y)*S + z]
};

namespace {

// The frame of the two creators: the NULL stream, behind the last asynchronous edit of the medium, as commit / download
// are.  *d_array gets the snapshot's 8^depth words (its owner frees them, on failure too), a scratch block of
// `scratch_bytes` lives for the call; run(d_scratch) enqueues the work and reads back the few words the creator needs.
template <class Run>
hipError_t snapshot_run(vrc_volume* medium, uint32_t** d_array, size_t scratch_bytes, Run run)
{
    uint32_t* d_scratch = nullptr;
    hipError_t e = hipSetDevice(medium->device);
    if (e == hipSuccess) e = order_behind_edits(medium, nullptr);
    if (e == hipSuccess) e = hipMalloc((void**)d_array, (size_t)4u << (3u * medium->depth));
    if (e == hipSuccess) e = hipMalloc((void**)&d_scratch, scratch_bytes);
    if (e == hipSuccess) e = run(d_scratch);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (d_scratch) (void)hipFree(d_scratch);
    return e;
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
    const hipError_t e = snapshot_run(medium, &l->d_ids, vrc::components_scratch_bytes(l->depth), [&](uint32_t* d_scratch) {
        vrc::components_roots_run(medium->d_bricks, l->depth, connectivity, through, l->d_ids, d_scratch, nullptr);
        hipError_t run = hipGetLastError();
        if (run == hipSuccess) run = hipMemcpy(&C, vrc::components_total_slot(d_scratch, l->depth), 4, hipMemcpyDeviceToHost);
        if (run == hipSuccess && C) run = hipMalloc((void**)&l->d_records, (size_t)C * sizeof(vrc_component));
        if (run == hipSuccess && C) {
            vrc::components_ids_run(l->depth, l->d_ids, d_scratch, l->d_records, nullptr);
            run = hipGetLastError();
        }
        return run;
    });
    if (e != hipSuccess) {
        (void)vrc_labels_destroy(l);
        return vrc::fail_hip(e, what);
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
    delete l;
    return VRC_OK;
}

extern "C" uint64_t vrc_labels_count(const vrc_labels* l) { return l ? l->count : 0; }
extern "C" uint32_t vrc_labels_depth(const vrc_labels* l) { return l ? l->depth : 0; }
extern "C" uint64_t vrc_labels_bytes(const vrc_labels* l) { return l ? ((uint64_t)4u << (3u * l->depth)) + l->count * sizeof(vrc_component) : 0; }

extern "C" int vrc_labels_components(const vrc_labels* l, uint64_t first, uint64_t capacity, vrc_component* out, int mem, void* stream)
{
    const char* what = "vrc_labels_components";
    if (!l) return vrc::fail(VRC_ERR_INVALID, "%s: null labels", what);
    if (const int rc = check_mem(what, mem)) return rc;
    if (!out && capacity) return vrc::fail(VRC_ERR_INVALID, "%s: null buffer with capacity %llu", what, (unsigned long long)capacity);
    const uint64_t want = first < l->count ? (capacity < l->count - first ? capacity : l->count - first) : 0u;
    if (!want) return VRC_OK;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipSetDevice(l->device);
    if (e == hipSuccess)
        e = hipMemcpyAsync(out, l->d_records + first, (size_t)want * sizeof(vrc_component), mem == VRC_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && mem == VRC_MEM_HOST) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return vrc::fail_hip(e, what);
    return VRC_OK;
}

extern "C" int vrc_labels_at(const vrc_labels* l, uint64_t n, const uint32_t* xyz, uint32_t* ids, int mem, void* stream)
{
    const char* what = "vrc_labels_at";
    if (!l) return vrc::fail(VRC_ERR_INVALID, "%s: null labels", what);
    if (const int rc = check_mem(what, mem)) return rc;
    if (n == 0) return VRC_OK;
    if (!xyz || !ids) return vrc::fail(VRC_ERR_INVALID, "%s: null buffer", what);
    if (n > 0x7fffffffull * 256ull) return vrc::fail(VRC_ERR_INVALID, "%s: too many voxels for one launch", what);
    hipStream_t st = (hipStream_t)stream;
    return staged_call(what, l->device, nullptr, xyz, (size_t)n * 12u, ids, (size_t)n * 4u, mem, st, [&](const void* d_xyz, void* d_ids) {
        vrc::components_at_run(l->d_ids, l->depth, n, (const uint32_t*)d_xyz, (uint32_t*)d_ids, st);
        return hipSuccess;
    });
}

extern "C" int vrc_labels_select(const vrc_labels* l, const uint8_t* keep, vrc_volume* dst, int op, int mem, void* stream)
{
    const char* what = "vrc_labels_select";
    if (!l || !dst) return vrc::fail(VRC_ERR_INVALID, "%s: null argument", what);
    if (const int rc = check_op(what, op)) return rc;
    if (const int rc = check_mem(what, mem)) return rc;
    if (dst->depth != l->depth) return vrc::fail(VRC_ERR_INVALID, "%s: labels of depth %u, volume of depth %u", what, l->depth, dst->depth);
    if (dst->device != l->device) return vrc::fail(VRC_ERR_INVALID, "%s: labels on device %d, volume on device %d", what, l->device, dst->device);
    if (!keep && l->count) return vrc::fail(VRC_ERR_INVALID, "%s: null keep with %llu components", what, (unsigned long long)l->count);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipSetDevice(l->device);
    if (e == hipSuccess) e = order_behind_edits(dst, st);
    const uint8_t* d_keep = keep;
    uint8_t* d_stage = nullptr;
    if (mem == VRC_MEM_HOST && l->count) {
        if (e == hipSuccess) e = hipMalloc((void**)&d_stage, (size_t)l->count);
        if (e == hipSuccess) e = hipMemcpyAsync(d_stage, keep, (size_t)l->count, hipMemcpyHostToDevice, st);
        d_keep = d_stage;
    }
    if (e == hipSuccess) {
        vrc::components_select_run(l->d_ids, l->depth, d_keep, dst->d_bricks, op, st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = finish(dst, mem, st, true);
    if (d_stage) (void)hipFree(d_stage);
    if (e != hipSuccess) return vrc::fail_hip(e, what);
    return VRC_OK;
}

// how far every piece can fall (the rule: include/vrc.h; the passes: vrc_fall.hip).  Synchronous, on the NULL stream.
extern "C" int vrc_fall_drops(const vrc_labels* l, vrc_volume* fixed, int direction, uint32_t drop_limit, int32_t* offsets, int mem, vrc_fall_stats* stats)
{
    const char* what = "vrc_fall_drops";
    if (!l) return vrc::fail(VRC_ERR_INVALID, "%s: null labels", what);
    if (direction < VRC_FACE_XN || direction > VRC_FACE_ZP) return vrc::fail(VRC_ERR_INVALID, "%s: direction %d is not a face code 0..5", what, direction);
    if (const int rc = check_mem(what, mem)) return rc;
    if (fixed && fixed->depth != l->depth) return vrc::fail(VRC_ERR_INVALID, "%s: labels of depth %u, volume of depth %u", what, l->depth, fixed->depth);
    if (fixed && fixed->device != l->device) return vrc::fail(VRC_ERR_INVALID, "%s: labels on device %d, volume on device %d", what, l->device, fixed->device);
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
    if (dst->depth != l->depth) return vrc::fail(VRC_ERR_INVALID, "%s: labels of depth %u, volume of depth %u", what, l->depth, dst->depth);
    if (dst->device != l->device) return vrc::fail(VRC_ERR_INVALID, "%s: labels on device %d, volume on device %d", what, l->device, dst->device);
    if (!offsets && l->count) return vrc::fail(VRC_ERR_INVALID, "%s: null offsets with %llu components", what, (unsigned long long)l->count);
    if (!l->count) return VRC_OK;
    hipStream_t st = (hipStream_t)stream;
    const size_t offset_bytes = (size_t)l->count * 12u;
    hipError_t e = hipSetDevice(l->device);
    if (e == hipSuccess) e = order_behind_edits(dst, st);
    const uint8_t* d_keep = keep;
    const int32_t* d_offsets = offsets;
    uint8_t* d_stage = nullptr;
    if (mem == VRC_MEM_HOST) {                       // staged: the offsets, then the keep bytes
        if (e == hipSuccess) e = hipMalloc((void**)&d_stage, offset_bytes + (keep ? (size_t)l->count : 0u));
        if (e == hipSuccess) e = hipMemcpyAsync(d_stage, offsets, offset_bytes, hipMemcpyHostToDevice, st);
        if (e == hipSuccess && keep) e = hipMemcpyAsync(d_stage + offset_bytes, keep, (size_t)l->count, hipMemcpyHostToDevice, st);
        d_offsets = (const int32_t*)d_stage;
        d_keep = keep ? d_stage + offset_bytes : nullptr;
    }
    if (e == hipSuccess) {
        vrc::place_run(l->d_ids, l->depth, d_keep, d_offsets, dst->d_bricks, op, st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = finish(dst, mem, st, true);
    if (d_stage) (void)hipFree(d_stage);
    if (e != hipSuccess) return vrc::fail_hip(e, what);
    return VRC_OK;
}

// ---- the pieces as rigid bodies with a pose (the rules: include/vrc.h; the kernels: vrc_rigid.hip) ---------------

extern "C" int vrc_rigid_moments(const vrc_labels* l, uint64_t first, uint64_t capacity, vrc_piece_moments* out, int mem, void* stream)
{
    const char* what = "vrc_rigid_moments";
    if (!l) return vrc::fail(VRC_ERR_INVALID, "%s: null labels", what);
    if (const int rc = check_mem(what, mem)) return rc;
    if (!out && capacity) return vrc::fail(VRC_ERR_INVALID, "%s: null buffer with capacity %llu", what, (unsigned long long)capacity);
    const uint64_t want = first < l->count ? (capacity < l->count - first ? capacity : l->count - first) : 0u;
    if (!want) return VRC_OK;
    hipStream_t st = (hipStream_t)stream;
    const size_t bytes = (size_t)want * sizeof(vrc_piece_moments);
    vrc_piece_moments* d_out = out;
    vrc_piece_moments* d_stage = nullptr;
    hipError_t e = hipSetDevice(l->device);
    if (mem == VRC_MEM_HOST) {
        if (e == hipSuccess) e = hipMalloc((void**)&d_stage, bytes);
        d_out = d_stage;
    }
    if (e == hipSuccess) e = vrc::moments_run(l->d_ids, l->depth, first, want, d_out, st);
    if (e == hipSuccess && mem == VRC_MEM_HOST) e = hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && mem == VRC_MEM_HOST) e = hipStreamSynchronize(st);
    if (d_stage) (void)hipFree(d_stage);
    if (e != hipSuccess) return vrc::fail_hip(e, what);
    return VRC_OK;
}

extern "C" int vrc_rigid_place_affine(const vrc_labels* l, const uint8_t* keep, const vrc_affine* maps, const uint32_t* boxes, vrc_volume* dst, int op, int mem,
                                      void* stream)
{
    const char* what = "vrc_rigid_place_affine";
    if (!l || !dst) return vrc::fail(VRC_ERR_INVALID, "%s: null argument", what);
    if (const int rc = check_op(what, op)) return rc;
    if (op == VRC_COPY_REPLACE) return vrc::fail(VRC_ERR_INVALID, "%s: VRC_COPY_REPLACE has no meaning where pieces may overlap", what);
    if (const int rc = check_mem(what, mem)) return rc;
    if (dst->device != l->device) return vrc::fail(VRC_ERR_INVALID, "%s: labels on device %d, volume on device %d", what, l->device, dst->device);
    if (!maps && l->count) return vrc::fail(VRC_ERR_INVALID, "%s: null maps with %llu components", what, (unsigned long long)l->count);
    if (mem == VRC_MEM_HOST)
        for (uint64_t i = 0; i < l->count; ++i)
            if (const int rc = check_affine(what, maps + i, (long long)i)) return rc;
    if (!l->count) return VRC_OK;
    hipStream_t st = (hipStream_t)stream;
    const size_t C = (size_t)l->count, map_bytes = C * sizeof(vrc_affine), box_bytes = boxes ? C * 24u : 0u, keep_bytes = keep ? C : 0u;
    hipError_t e = hipSetDevice(l->device);
    if (e == hipSuccess) e = order_behind_edits(dst, st);
    const uint8_t* d_keep = keep;
    const vrc_affine* d_maps = maps;
    const uint32_t* d_boxes = boxes;
    uint8_t* d_stage = nullptr;
    if (mem == VRC_MEM_HOST) {                       // staged: the maps, then the boxes, then the keep bytes
        if (e == hipSuccess) e = hipMalloc((void**)&d_stage, map_bytes + box_bytes + keep_bytes);
        if (e == hipSuccess) e = hipMemcpyAsync(d_stage, maps, map_bytes, hipMemcpyHostToDevice, st);
        if (e == hipSuccess && boxes) e = hipMemcpyAsync(d_stage + map_bytes, boxes, box_bytes, hipMemcpyHostToDevice, st);
        if (e == hipSuccess && keep) e = hipMemcpyAsync(d_stage + map_bytes + box_bytes, keep, keep_bytes, hipMemcpyHostToDevice, st);
        d_maps = (const vrc_affine*)d_stage;
        d_boxes = boxes ? (const uint32_t*)(d_stage + map_bytes) : nullptr;
        d_keep = keep ? d_stage + map_bytes + box_bytes : nullptr;
    }
    if (e == hipSuccess) {
        vrc::place_affine_run(l->d_ids, l->d_records, l->count, l->depth, d_keep, d_maps, d_boxes, dst->d_bricks, dst->depth, op, st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = finish(dst, mem, st, true);
    if (d_stage) (void)hipFree(d_stage);
    if (e != hipSuccess) return vrc::fail_hip(e, what);
    return VRC_OK;
}

extern "C" int vrc_rigid_contacts(const vrc_labels* l, const uint8_t* keep, const vrc_affine* maps, const uint32_t* boxes, vrc_volume* world,
                                  vrc_piece_contact* out, int mem, void* stream)
{
    const char* what = "vrc_rigid_contacts";
    if (!l || !world) return vrc::fail(VRC_ERR_INVALID, "%s: null argument", what);
    if (const int rc = check_mem(what, mem)) return rc;
    if (world->device != l->device) return vrc::fail(VRC_ERR_INVALID, "%s: labels on device %d, volume on device %d", what, l->device, world->device);
    if (!maps && l->count) return vrc::fail(VRC_ERR_INVALID, "%s: null maps with %llu components", what, (unsigned long long)l->count);
    if (!out && l->count) return vrc::fail(VRC_ERR_INVALID, "%s: null records with %llu components", what, (unsigned long long)l->count);
    if (mem == VRC_MEM_HOST)
        for (uint64_t i = 0; i < l->count; ++i)
            if (const int rc = check_affine(what, maps + i, (long long)i)) return rc;
    if (!l->count) return VRC_OK;
    hipStream_t st = (hipStream_t)stream;
    const size_t C = (size_t)l->count, map_bytes = C * sizeof(vrc_affine), box_bytes = boxes ? C * 24u : 0u, keep_bytes = keep ? C : 0u;
    const size_t out_bytes = C * sizeof(vrc_piece_contact);
    hipError_t e = hipSetDevice(l->device);
    if (e == hipSuccess) e = order_behind_edits(world, st);          // the call reads the world's occupancy, as vrc_volume_count_boxes does
    const uint8_t* d_keep = keep;
    const vrc_affine* d_maps = maps;
    const uint32_t* d_boxes = boxes;
    vrc_piece_contact* d_out = out;
    uint8_t* d_stage = nullptr;
    if (mem == VRC_MEM_HOST) {                       // staged: the records, then the maps, then the boxes, then the keep bytes
        if (e == hipSuccess) e = hipMalloc((void**)&d_stage, out_bytes + map_bytes + box_bytes + keep_bytes);
        if (e == hipSuccess) e = hipMemcpyAsync(d_stage + out_bytes, maps, map_bytes, hipMemcpyHostToDevice, st);
        if (e == hipSuccess && boxes) e = hipMemcpyAsync(d_stage + out_bytes + map_bytes, boxes, box_bytes, hipMemcpyHostToDevice, st);
        if (e == hipSuccess && keep) e = hipMemcpyAsync(d_stage + out_bytes + map_bytes + box_bytes, keep, keep_bytes, hipMemcpyHostToDevice, st);
        d_out = (vrc_piece_contact*)d_stage;
        d_maps = (const vrc_affine*)(d_stage + out_bytes);
        d_boxes = boxes ? (const uint32_t*)(d_stage + out_bytes + map_bytes) : nullptr;
        d_keep = keep ? d_stage + out_bytes + map_bytes + box_bytes : nullptr;
    }
    if (e == hipSuccess) e = vrc::contacts_run(l->d_ids, l->d_records, l->count, l->depth, d_keep, d_maps, d_boxes, world->d_bricks, world->depth, d_out, st);
    if (e == hipSuccess && mem == VRC_MEM_HOST) e = hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = finish(world, mem, st, false);           // not an edit: the world is only read
    if (d_stage) (void)hipFree(d_stage);
    if (e != hipSuccess) return vrc::fail_hip(e, what);
    return VRC_OK;
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
    d->device = medium->device; d->depth = medium->depth;
    unsigned long long host[2] = {0ull, 0ull};
    const hipError_t e = snapshot_run(medium, &d->d_field, vrc::distance_scratch_bytes(d->depth, medium->cu_count), [&](uint32_t* d_scratch) {
        vrc::distance_run(medium->d_bricks, d->depth, to, outside, medium->cu_count, d->d_field, d_scratch, nullptr);
        const hipError_t run = hipGetLastError();
        return run != hipSuccess ? run : hipMemcpy(host, vrc::distance_stats_slots(d_scratch), sizeof host, hipMemcpyDeviceToHost);
    });
    if (e != hipSuccess) {
        (void)vrc_distance_destroy(d);
        return vrc::fail_hip(e, what);
    }
    if (stats) {
        stats->features = host[0];
        stats->max_d2 = 0u; stats->argmax[0] = stats->argmax[1] = stats->argmax[2] = 0u; stats->reserved = 0u;
        if (host[1]) {
            const uint32_t index = ~(uint32_t)host[1], mask = (1u << d->depth) - 1u;
            stats->max_d2 = (uint32_t)(host[1] >> 32);
            stats->argmax[0] = index >> (2u * d->depth); stats->argmax[1] = (index >> d->depth) & mask; stats->argmax[2] = index & mask;
        }
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
    if (n > 0x7fffffffull * 256ull) return vrc::fail(VRC_ERR_INVALID, "%s: too many voxels for one launch", what);
    hipStream_t st = (hipStream_t)stream;
    return staged_call(what, d->device, nullptr, xyz, (size_t)n * 12u, d2, (size_t)n * 4u, mem, st, [&](const void* d_xyz, void* d_d2) {
        vrc::distance_at_run(d->d_field, d->depth, n, (const uint32_t*)d_xyz, (uint32_t*)d_d2, st);
        return hipSuccess;
    });
}

extern "C" int vrc_distance_download(const vrc_distance* d, uint32_t* d2_host)
{
    const char* what = "vrc_distance_download";
    if (!d || !d2_host) return vrc::fail(VRC_ERR_INVALID, "%s: null argument", what);
    hipError_t e = hipSetDevice(d->device);
    if (e == hipSuccess) e = hipMemcpy(d2_host, d->d_field, (size_t)4u << (3u * d->depth), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return vrc::fail_hip(e, what);
    return VRC_OK;
}

extern "C" int vrc_distance_select(const vrc_distance* d, uint32_t lo, uint32_t hi, vrc_volume* dst, int op, void* stream)
{
    const char* what = "vrc_distance_select";
    if (!d || !dst) return vrc::fail(VRC_ERR_INVALID, "%s: null argument", what);
    if (const int rc = check_op(what, op)) return rc;
    if (lo > hi) return vrc::fail(VRC_ERR_INVALID, "%s: lo %u above hi %u", what, lo, hi);
    if (dst->depth != d->depth) return vrc::fail(VRC_ERR_INVALID, "%s: field of depth %u, volume of depth %u", what, d->depth, dst->depth);
    if (dst->device != d->device) return vrc::fail(VRC_ERR_INVALID, "%s: field on device %d, volume on device %d", what, d->device, dst->device);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipSetDevice(d->device);
    if (e == hipSuccess) e = order_behind_edits(dst, st);
    if (e == hipSuccess) {
        vrc::distance_select_run(d->d_field, d->depth, lo, hi, dst->d_bricks, op, st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = finish(dst, VRC_MEM_DEVICE, st, true);
    if (e != hipSuccess) return vrc::fail_hip(e, what);
    return VRC_OK;
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
    if (seeds->depth != medium->depth) return vrc::fail(VRC_ERR_INVALID, "%s: volumes of depths %u and %u", what, seeds->depth, medium->depth);
    if (seeds->device != medium->device) return vrc::fail(VRC_ERR_INVALID, "%s: volumes on devices %d and %d", what, seeds->device, medium->device);
    if (medium->depth < 2 || medium->depth > 10) return vrc::fail(VRC_ERR_INVALID, "%s: depth %u not in [2,10]", what, medium->depth);
    vrc_distance* d = new (std::nothrow) vrc_distance();
    if (!d) return vrc::fail(VRC_ERR_OOM, "out of host memory");
    d->device = medium->device; d->depth = medium->depth; d->connectivity = connectivity;
    unsigned long long host[3] = {0ull, 0ull, 0ull};
    uint32_t sweeps = 0, converged = 0;
    const hipError_t e = snapshot_run(medium, &d->d_field, vrc::travel_scratch_bytes(d->depth), [&](uint32_t* d_scratch) {
        hipError_t run = order_behind_edits(seeds, nullptr);
        if (run == hipSuccess)
            run = vrc::travel_run(seeds->d_bricks, medium->d_bricks, d->depth, connectivity, through, step_limit, d->d_field, d_scratch, nullptr, &sweeps,
                                  &converged);
        return run != hipSuccess ? run : hipMemcpy(host, vrc::travel_stats_slots(d_scratch), sizeof host, hipMemcpyDeviceToHost);
    });
    if (e != hipSuccess) {
        (void)vrc_distance_destroy(d);
        return vrc::fail_hip(e, what);
    }
    if (!converged) {
        (void)vrc_distance_destroy(d);
        return vrc::fail(VRC_ERR_HIP, "%s: internal error: no fixed point within the bound of %u sweeps", what, sweeps);
    }
    if (stats) {
        stats->seeds = host[0]; stats->reached = host[1];
        stats->max_steps = 0u; stats->argmax[0] = stats->argmax[1] = stats->argmax[2] = 0u; stats->sweeps = sweeps; stats->reserved = 0u;
        if (host[2]) {
            const uint32_t index = ~(uint32_t)host[2], mask = (1u << d->depth) - 1u;
            stats->max_steps = (uint32_t)(host[2] >> 32);
            stats->argmax[0] = index >> (2u * d->depth); stats->argmax[1] = (index >> d->depth) & mask; stats->argmax[2] = index & mask;
        }
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
    if (n > 0x7fffffffull * 256ull) return vrc::fail(VRC_ERR_INVALID, "%s: too many starts for one launch", what);
    if (capacity && n > (1ull << 58) / capacity) return vrc::fail(VRC_ERR_INVALID, "%s: %llu routes of capacity %u are too many", what, (unsigned long long)n, capacity);
    hipStream_t st = (hipStream_t)stream;
    const size_t in_bytes = (size_t)n * 12u, len_bytes = (size_t)n * 4u, path_bytes = (size_t)n * capacity * 12u;
    hipError_t e = hipSetDevice(d->device);
    const uint32_t* d_in = start_xyz;
    uint32_t *d_len = lengths, *d_paths = paths_xyz;
    uint8_t* own = nullptr;
    if (mem == VRC_MEM_HOST) {
        // staged: starts, lengths, paths.  The caller's paths go up first, so that what the kernel leaves alone comes back as it was.
        if (e == hipSuccess) e = hipMalloc((void**)&own, in_bytes + len_bytes + path_bytes);
        d_in = (const uint32_t*)own; d_len = (uint32_t*)(own + in_bytes); d_paths = (uint32_t*)(own + in_bytes + len_bytes);
        if (e == hipSuccess) e = hipMemcpyAsync(own, start_xyz, in_bytes, hipMemcpyHostToDevice, st);
        if (e == hipSuccess && path_bytes) e = hipMemcpyAsync(d_paths, paths_xyz, path_bytes, hipMemcpyHostToDevice, st);
    }
    if (e == hipSuccess) {
        vrc::travel_trace_run(d->d_field, d->depth, d->connectivity, n, d_in, capacity, d_paths, d_len, st);
        e = hipGetLastError();
    }
    if (mem == VRC_MEM_HOST) {
        if (e == hipSuccess) e = hipMemcpyAsync(lengths, d_len, len_bytes, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && path_bytes) e = hipMemcpyAsync(paths_xyz, d_paths, path_bytes, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (own) (void)hipFree(own);
    }
    if (e != hipSuccess) return vrc::fail_hip(e, what);
    return VRC_OK;
}
