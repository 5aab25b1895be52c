// vrc_volume_state.h -- what the entry points of the editable volume share (vrc_volume.hip: the volume itself;
// vrc_snapshots.hip: the labels and distance fields taken from it): the volume's record, the rule that orders a call behind
// the volume's last asynchronous edit, the end of a call that takes a memory kind, the grow-only device block, the
// argument checks with one text each, and the frame of a host-memory call that takes a list in and hands a list back.
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
    // by the first call, fixed in size
    unsigned long long* d_surface = nullptr;
    // vrc_rect_count / _extract_rects: the per-workgroup rectangle offsets, the totals and the two row bit fields
    // (vrc_rects.h), allocated by the first call, fixed in size
    unsigned long long* d_rects = nullptr;
    // the last asynchronous edit: commit / download / solid_count run on the NULL stream and wait for it first.  The flag
    // says that the event has been recorded at least once; it is never cleared, because a wait only orders ONE stream
    // behind the edit and the next caller may bring another.
    hipEvent_t edit_done = nullptr;
    bool edit_pending = false;
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

// the end of every call that takes `mem`: a host-memory call is synchronous, a device-memory edit is recorded as the
// volume's last asynchronous edit
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

// The frame of the calls that take a list in and hand a list back: `in_bytes` at `in`, `out_bytes` at `out`.  Device memory
// is used in place and the call stays asynchronous on `st`.  Host memory is staged, input then output, and the call is
// synchronous: in the grow-only block of `v`, or, for the snapshots (v == nullptr), which deliberately keep no scratch, in
// a block of the call's own.  A call on a volume reads its occupancy and writes its staging block: behind the volume's
// last asynchronous edit whatever the memory kind.  launch(d_in, d_out) enqueues the work on `st` and returns what its
// HIP calls returned.
template <class Launch>
int staged_call(const char* what, int device, vrc_volume* v, const void* in, size_t in_bytes, void* out, size_t out_bytes, int mem, hipStream_t st, Launch launch)
{
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess && v) e = order_behind_edits(v, st);
    const void* d_in = in;
    void* d_out = out;
    void* own = nullptr;
    if (mem == VRC_MEM_HOST) {
        if (e == hipSuccess) e = v ? reserve(v->d_stage, v->stage_cap, in_bytes + out_bytes) : hipMalloc(&own, in_bytes + out_bytes);
        uint8_t* block = v ? (uint8_t*)v->d_stage : (uint8_t*)own;
        d_in = block;
        d_out = block + in_bytes;
        if (e == hipSuccess) e = hipMemcpyAsync(block, in, in_bytes, hipMemcpyHostToDevice, st);
    }
    if (e == hipSuccess) e = launch(d_in, d_out);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess && mem == VRC_MEM_HOST) e = hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && mem == VRC_MEM_HOST) e = hipStreamSynchronize(st);
    if (own) (void)hipFree(own);
    if (e != hipSuccess) return vrc::fail_hip(e, what);
    return VRC_OK;
}

}  // namespace
