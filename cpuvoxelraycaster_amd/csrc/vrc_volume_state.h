// vrc_volume_state.h -- what the entry points of the editable volume share (vrc_volume.hip: the volume itself;
// vrc_volume_ops.hip: the calls between two volumes and along their axes; vrc_snapshots.hip: the labels, fields and deltas
// taken from it): the volume's record, the argument checks with one text each, the rule that orders a call behind the last
// asynchronous edit of the volumes it names, the grow-only device block, and the one frame of every call (staged_call, with
// lists of arguments or without).  Which stream every entry point runs on, what it waits for, whether it is recorded as an
// edit and whether it is synchronous: the table in DESIGN.md.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/vrc.h"
#include "vrc_build_grids.h"
#include "vrc_host.h"

struct vrc_volume {
    int device = 0;
    int cu_count = 0;
    uint32_t depth = 0;
    uint32_t* d_bricks = nullptr;     // n^3 brick bytes, addressed as 32-bit words by the edit kernels (n^3 is a multiple of 8)
    uint64_t n_bricks = 0;
    void* d_tex = nullptr;            // 1536 bytes: the albedo tables every committed scene gets
    unsigned long long* d_count = nullptr;
    BuildGrids grids;                 // kept between commits, allocated by the first
    // host-memory form of the edit calls: grow-only staging block
    uint32_t* d_stage = nullptr;
    size_t stage_cap = 0;
    // vrc_volume_flood with this volume as `region`: grow-only tile flags and sweep counters
    uint32_t* d_flood = nullptr;
    size_t flood_cap = 0;
    // vrc_volume_xor_mesh: the mark field, as large as d_bricks, allocated and zeroed by the first call, zero between calls
    uint32_t* d_marks = nullptr;
    // vrc_volume_surface_count / _extract_surface: the per-workgroup face offsets and the totals (vrc_surface.h), allocated
    // by the first call, fixed in size; vrc_voxels_count / _extract use the same slots (vrc_voxels.h)
    unsigned long long* d_surface = nullptr;
    // vrc_rect_count / _extract_rects: the per-workgroup rectangle offsets, the totals and the two row bit fields
    // (vrc_rects.h), allocated by the first call, fixed in size
    unsigned long long* d_rects = nullptr;
    // vrc_pack_volume / vrc_unpack_volume: the totals and the two slot arrays (vrc_pack.h), allocated by the first call, fixed
    // in size
    void* d_pack = nullptr;
    // the last asynchronous edit: commit / download / solid_count run on the NULL stream and wait for it first.  The flag
    // says that the event has been recorded at least once; it is never cleared, because a wait only orders ONE stream
    // behind the edit and the next caller may bring another.
    hipEvent_t edit_done = nullptr;
    bool edit_pending = false;
    // vrc_levels_reduce with this volume as dst and a level difference of 4 and more: the counts of its voxels' cells, grow-only,
    // at most 64^3 of them (vrc_levels.h)
    uint32_t* d_levels = nullptr;
    size_t levels_cap = 0;
    // vrc_morph_apply with this volume as dst: the prepared element (vrc_morph.h), allocated by the first call, fixed in size
    void* d_morph = nullptr;
};

namespace {

// the argument checks: VRC_OK, or the refusal "<what>: ..."
inline int check_mem(const char* what, int mem)
{
    return mem == VRC_MEM_HOST || mem == VRC_MEM_DEVICE ? VRC_OK : vrc::fail(VRC_ERR_INVALID, "%s: bad mem kind %d", what, mem);
}
inline int check_op(const char* what, int op)
{
    return op == VRC_COPY_REPLACE || op == VRC_COPY_OR || op == VRC_COPY_ANDNOT ? VRC_OK : vrc::fail(VRC_ERR_INVALID, "%s: bad op %d", what, op);
}
inline int check_connectivity(const char* what, int connectivity)
{
    const bool ok = connectivity == VRC_CONNECT_FACES || connectivity == VRC_CONNECT_ALL;
    return ok ? VRC_OK : vrc::fail(VRC_ERR_INVALID, "%s: connectivity %d is neither 6 nor 26", what, connectivity);
}
inline int check_through(const char* what, int through)
{
    return through == VRC_FLOOD_SOLID || through == VRC_FLOOD_EMPTY ? VRC_OK : vrc::fail(VRC_ERR_INVALID, "%s: bad through %d", what, through);
}

// labels / field and volume on one device and, with_depth, of one depth; `noun` is what the snapshot is called
inline int check_same(const char* what, const char* noun, uint32_t depth, int device, const vrc_volume* v, bool with_depth = true)
{
    if (with_depth && v->depth != depth) return vrc::fail(VRC_ERR_INVALID, "%s: %s of depth %u, volume of depth %u", what, noun, depth, v->depth);
    if (v->device != device) return vrc::fail(VRC_ERR_INVALID, "%s: %s on device %d, volume on device %d", what, noun, device, v->device);
    return VRC_OK;
}
// Two volumes of one call: not one volume twice, on one device and, same_depth, of one depth.  `a` is printed before `b`;
// vrc_volume_copy_region and vrc_volume_stamp_affine print src first, every other call dst.
inline int check_distinct(const char* what, const vrc_volume* a, const vrc_volume* b)
{
    return a != b ? VRC_OK : vrc::fail(VRC_ERR_INVALID, "%s: source and destination are the same volume", what);
}
inline int check_pair(const char* what, const vrc_volume* a, const vrc_volume* b, bool same_depth)
{
    if (const int rc = check_distinct(what, a, b)) return rc;
    if (same_depth && a->depth != b->depth) return vrc::fail(VRC_ERR_INVALID, "%s: volumes of depths %u and %u", what, a->depth, b->depth);
    if (a->device != b->device) return vrc::fail(VRC_ERR_INVALID, "%s: volumes on devices %d and %d", what, a->device, b->device);
    return VRC_OK;
}
// what one launch takes: a lane per item in 256-lane workgroups, or a workgroup (blockIdx.x) per item
constexpr uint64_t LANE_ITEMS = 0x7fffffffull * 256ull, GROUP_ITEMS = 0x7fffffffull;
inline int check_count(const char* what, uint64_t n, uint64_t limit, const char* items)
{
    return n <= limit ? VRC_OK : vrc::fail(VRC_ERR_INVALID, "%s: too many %s for one launch", what, items);
}

// how many of `count` items the window [first, first + capacity) holds
inline uint64_t window_of(uint64_t first, uint64_t capacity, uint64_t count)
{
    return first < count ? (capacity < count - first ? capacity : count - first) : 0u;
}

// the end of every entry point that called HIP
inline int done(hipError_t e, const char* what) { return e == hipSuccess ? VRC_OK : vrc::fail_hip(e, what); }

// the limits of an affine map that keep s = m (2p + 1) + t below 2^41 and a word's deltas below 2^25 (vrc.h:
// vrc_volume_stamp_affine); `piece` < 0: the call has one map, else the text names the piece
inline int check_affine(const char* what, const vrc_affine* map, long long piece)
{
    char of[40] = "";
    if (piece >= 0) snprintf(of, sizeof of, "piece %lld: ", piece);
    if (map->reserved != 0) return vrc::fail(VRC_ERR_INVALID, "%s: %sreserved is %d, not 0", what, of, map->reserved);
    for (int i = 0; i < 9; ++i)
        if (map->m[i] > (1 << 20) || map->m[i] < -(1 << 20)) return vrc::fail(VRC_ERR_INVALID, "%s: %sm[%d] = %d beyond +-2^20", what, of, i, map->m[i]);
    for (int a = 0; a < 3; ++a)
        if (map->t[a] > (1ll << 40) || map->t[a] < -(1ll << 40))
            return vrc::fail(VRC_ERR_INVALID, "%s: %st[%d] = %lld beyond +-2^40", what, of, a, (long long)map->t[a]);
    return VRC_OK;
}

// orders `st` (nullptr: the NULL stream) behind the last asynchronous edit: for the calls that read the occupancy, and for
// every call that writes the staging block -- the device-memory brush at hits leaves its centres there, in flight on the
// caller's stream
inline hipError_t order_behind_edits(vrc_volume* v, hipStream_t st)
{
    return v->edit_pending ? hipStreamWaitEvent(st, v->edit_done, 0) : hipSuccess;
}

// the end of every call: a host-memory call is synchronous, a device-memory edit is recorded as the volume's last
// asynchronous edit
inline hipError_t finish(vrc_volume* v, int mem, hipStream_t st, bool is_edit)
{
    if (mem == VRC_MEM_HOST) return hipStreamSynchronize(st);
    if (!is_edit) return hipSuccess;
    v->edit_pending = true;            // the NULL stream included: streams made by vrc_stream_create do not wait for it
    return hipEventRecord(v->edit_done, st);
}

// A grow-only device block, at least `need` bytes.  hipFree waits for everything that may still read the old block.
template <class T>
hipError_t reserve(T*& block, size_t& cap, size_t need)
{
    if (cap >= need) return hipSuccess;
    if (block) (void)hipFree(block);
    block = nullptr; cap = 0;
    const hipError_t e = hipMalloc((void**)&block, need);
    if (e == hipSuccess) cap = need;
    return e;
}

// ---- the frame of every call: with lists of arguments in `mem`, or without ----------------------------------------------

// One list: `bytes` at the caller's `p`, read by the launch (IN), written by it (OUT) or both (INOUT: it goes up first,
// so that what the launch leaves alone comes back as it was).  p == nullptr or bytes == 0: the part is absent and its
// device pointer is nullptr.
enum { STAGE_IN = 1, STAGE_OUT = 2, STAGE_INOUT = 3 };
struct StagePart {
    const void* p;
    size_t bytes;
    int dir;
};

// How the call is ordered.  `v`: the volume it reads or writes, nullptr for a call on a snapshot alone.  Only the
// constructors below spell out the flags.
struct Call {
    int device;
    int mem;
    hipStream_t st;
    vrc_volume* v;
    bool is_edit;          // a device-memory call is recorded as v's last asynchronous edit
    bool stage_in_v;       // host memory is staged in v's grow-only block; else in a block of the call's own, freed at the end
    bool wait_always;      // behind v's last asynchronous edit whatever the memory kind: the call reads the occupancy or a
                           // block the volume shares.  false: a list edit waits in host form only, where it writes v's block
    vrc_volume* read;      // a second volume, only read (src, medium, ...): behind its last asynchronous edit in both memory
                           // kinds; nullptr: none
    bool synchronous;      // the stream is synchronised at the end in device form too
};

// An edit that reads one list: staged in the volume's block, recorded as its last edit, and -- unlike every other call on a
// volume -- behind the last asynchronous edit in host form only, where it writes that block; in device form it stays
// unordered against edits on other streams, as it always was.
inline Call edit_call(vrc_volume* v, int mem, void* stream) { return Call{v->device, mem, (hipStream_t)stream, v, true, true, false, nullptr, false}; }
// edit_call through a block the volume shares between calls (vrc_volume_xor_mesh's marks): behind the last edit in both kinds
inline Call shared_edit_call(vrc_volume* v, int mem, void* stream) { return Call{v->device, mem, (hipStream_t)stream, v, true, true, true, nullptr, false}; }
// A query: a list in and a list out through the volume's block, behind the last asynchronous edit whatever the memory kind.
inline Call query_call(vrc_volume* v, int mem, void* stream) { return Call{v->device, mem, (hipStream_t)stream, v, false, true, true, nullptr, false}; }
// a call on a snapshot alone: no volume to wait for, host memory staged in a block of the call's own
inline Call snapshot_call(int device, int mem, void* stream) { return Call{device, mem, (hipStream_t)stream, nullptr, false, false, false, nullptr, false}; }
// a call that reads (is_edit: writes) a volume beside a snapshot or a block the volume shares: behind the volume's last
// asynchronous edit whatever the memory kind, staged in a block of the call's own
inline Call volume_call(int device, int mem, void* stream, vrc_volume* v, bool is_edit) { return Call{device, mem, (hipStream_t)stream, v, is_edit, false, true, nullptr, false}; }
// an edit of dst that reads src: behind the last asynchronous edit of both
inline Call pair_call(vrc_volume* dst, vrc_volume* src, int mem, void* stream) { return Call{dst->device, mem, (hipStream_t)stream, dst, true, false, true, src, false}; }
// A call on the NULL stream whose results the host reads: behind the last asynchronous edit of v and of `read` (nullptr:
// none).  synchronous: the frame synchronises at the end; false where the launch's own blocking read-back has done so.
// is_edit: recorded as v's edit too, because streams made by vrc_stream_create do not wait for the NULL stream.
inline Call null_stream_call(vrc_volume* v, vrc_volume* read, bool is_edit, bool synchronous)
{
    return Call{v->device, VRC_MEM_DEVICE, nullptr, v, is_edit, false, true, read, synchronous};
}

// Device memory: launch(d) gets the caller's pointers and the call stays asynchronous on `st`.  Host memory: the parts are
// laid out in one block in the order given, the IN parts copied up, and after the launch the OUT parts copied down and the
// stream synchronised.  In a block of the call's own every part starts on a multiple of 16 bytes, whatever the order.  In
// v's block the parts are packed, because the block's size is observable (vrc_volume_edit_scratch_bytes) and is exactly the
// sum of the parts; the two calls that put more than one part there give the part with the wider items first.  launch(d)
// enqueues the work on `st` and returns what its HIP calls returned; it does not run after a failure.
template <size_t N, class Launch>
int staged_call(const char* what, const Call& c, const StagePart (&parts)[N], Launch launch)
{
    void* d[N];
    size_t at[N] = {}, total = 0;
    for (size_t i = 0; i < N; ++i) {
        const bool present = parts[i].p && parts[i].bytes;
        d[i] = present ? (void*)parts[i].p : nullptr;
        if (!present) continue;
        if (!c.stage_in_v) total = (total + 15u) & ~(size_t)15u;
        at[i] = total;
        total += parts[i].bytes;
    }
    const bool host = c.mem == VRC_MEM_HOST;
    uint8_t* own = nullptr;
    hipError_t e = hipSetDevice(c.device);
    if (e == hipSuccess && c.read) e = order_behind_edits(c.read, c.st);
    if (e == hipSuccess && c.v && (c.wait_always || host)) e = order_behind_edits(c.v, c.st);
    if (host && total) {
        if (e == hipSuccess) e = c.stage_in_v ? reserve(c.v->d_stage, c.v->stage_cap, total) : hipMalloc((void**)&own, total);
        uint8_t* block = c.stage_in_v ? (uint8_t*)c.v->d_stage : own;
        for (size_t i = 0; i < N; ++i) {
            if (!d[i]) continue;
            d[i] = block + at[i];
            if (e == hipSuccess && (parts[i].dir & STAGE_IN)) e = hipMemcpyAsync(d[i], parts[i].p, parts[i].bytes, hipMemcpyHostToDevice, c.st);
        }
    }
    if (e == hipSuccess) e = launch((void* const*)d);
    if (e == hipSuccess) e = hipGetLastError();
    if (host && total)
        for (size_t i = 0; i < N; ++i)
            if (e == hipSuccess && d[i] && (parts[i].dir & STAGE_OUT)) e = hipMemcpyAsync((void*)parts[i].p, d[i], parts[i].bytes, hipMemcpyDeviceToHost, c.st);
    if (e == hipSuccess) e = finish(c.v, c.mem, c.st, c.is_edit);
    if (e == hipSuccess && c.synchronous && !host) e = hipStreamSynchronize(c.st);
    if (own) (void)hipFree(own);
    return done(e, what);
}

// The frame of a call without lists: set the device, order, launch(), hipGetLastError, finish.  What the call allocates between
// ordering and launch goes into launch(), which returns what its HIP calls returned.
template <class Launch>
int staged_call(const char* what, const Call& c, Launch launch)
{
    const StagePart none[] = {{nullptr, 0u, STAGE_IN}};
    return staged_call(what, c, none, [&](void* const*) { return launch(); });
}

}  // namespace
