// vrc_renderer.cpp -- the renderer of the C ABI (include/vrc.h): its tuning, the frame launches (planned by
// vrc_plan.h), resolve / reset / clear, read-back, statistics and the multi-GPU shard plumbing.
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "vrc_host.h"
#include "vrc_plan.h"

using vrc::Tuning;

struct vrc_renderer {
    const vrc_scene* scene = nullptr;   // must outlive every vrc_render_frame call; the other calls only need r->device
    int device = 0;
    uint32_t depth = 0;                 // of the scene it was created for; vrc_renderer_set_scene takes scenes of this depth
    uint32_t width = 0, height = 0;
    void* d_image = nullptr;  // RGBA8
    void* image_target = nullptr;   // where sharded frames are resolved to instead of d_image (vrc_renderer_set_image_target): a peer's framebuffer
    void* d_accum = nullptr;  // 4 x u32 per pixel
    void* d_stats = nullptr;  // VRC_STATS_BYTES of counter slots, then VRC_QUEUE_BYTES of work-queue heads
    vrc_hit* d_prim = nullptr;
    // two sets of work-queue heads: a stage-synchronous launch takes its units from one set and zeroes the other for the
    // launch after it; queue_zero[s] = set s is known to hold zeros when the next launch reaches it
    bool queue_zero[2] = {false, false};
    uint32_t* d_tile_done = nullptr;   // one arrival counter per 8 x 8 tile (fused resolve), zero between frames
    Tuning tuning;      // snapshot of the process defaults at creation; vrc_renderer_set_* change it
    const char* last_kernel = "";   // symbol of the frame kernel the last vrc_render_frame* launched
};

namespace {

// the process-wide defaults of the scheduling knobs (vrc_plan.h: Tuning), under g_tuning_mu
Tuning g_tuning;
std::mutex g_tuning_mu;

constexpr uint32_t VRC_MAX_SPP = 65536;          // per call; the u32 accumulators hold 255 * 16.8 M samples in total

int apply_sample_chunk(Tuning& t, uint32_t samples_per_unit)
{
    // values above 0xffff0000 set the tail policy of the automatic mode instead (experiments): low 16 bits = units per wave
    if (samples_per_unit >= 0xffff0000u) { t.tail_units_per_wave = samples_per_unit & 0xffffu; return VRC_OK; }
    if (samples_per_unit > VRC_MAX_SPP) return vrc::fail(VRC_ERR_INVALID, "sample chunk %u > %u", samples_per_unit, VRC_MAX_SPP);
    t.sample_chunk = samples_per_unit;
    return VRC_OK;
}
int apply_tuning(Tuning& t, uint32_t blocks_per_cu)
{
    if (blocks_per_cu > 8) return vrc::fail(VRC_ERR_INVALID, "vrc_set_tuning: blocks_per_cu %u > 8", blocks_per_cu);
    t.blocks_per_cu = blocks_per_cu;
    t.blocks_per_cu_set = blocks_per_cu != 0;
    return VRC_OK;
}
// the switches of a renderer that take 0 or 1; `fn` names the entry point in the message
int set_switch(vrc_renderer* r, bool Tuning::*sw, uint32_t on, const char* fn)
{
    if (!r) return fail(VRC_ERR_INVALID, "null renderer");
    if (on > 1) return fail(VRC_ERR_INVALID, "%s: on = %u (0 or 1)", fn, on);
    r->tuning.*sw = on != 0;
    return VRC_OK;
}
// ... and the lane map, 0, 1 or 4: of a renderer (null = there is none) or the process default
int set_lane_samples(Tuning* t, uint32_t samples, const char* fn)
{
    if (!t) return fail(VRC_ERR_INVALID, "null renderer");
    if (samples != 0 && samples != 1 && samples != 4) return fail(VRC_ERR_INVALID, "%s: %u (0, 1 or 4)", fn, samples);
    t->lane_samples = samples;
    return VRC_OK;
}

}  // namespace

extern "C" int vrc_set_sample_chunk(uint32_t samples_per_unit)
{
    std::lock_guard<std::mutex> lk(g_tuning_mu);
    return apply_sample_chunk(g_tuning, samples_per_unit);
}
extern "C" int vrc_set_tuning(uint32_t blocks_per_cu)
{
    std::lock_guard<std::mutex> lk(g_tuning_mu);
    return apply_tuning(g_tuning, blocks_per_cu);
}
extern "C" int vrc_renderer_set_sample_chunk(vrc_renderer* r, uint32_t samples_per_unit)
{
    if (!r) return fail(VRC_ERR_INVALID, "null renderer");
    return apply_sample_chunk(r->tuning, samples_per_unit);
}
extern "C" int vrc_renderer_set_invariant_ray_reuse(vrc_renderer* r, uint32_t on) { return set_switch(r, &Tuning::reuse_invariant, on, "vrc_renderer_set_invariant_ray_reuse"); }
extern "C" int vrc_renderer_set_walk_from_root(vrc_renderer* r, uint32_t on) { return set_switch(r, &Tuning::walk_from_root, on, "vrc_renderer_set_walk_from_root"); }
extern "C" int vrc_renderer_set_quad_walks(vrc_renderer* r, uint32_t on) { return set_switch(r, &Tuning::quad_walks, on, "vrc_renderer_set_quad_walks"); }
extern "C" int vrc_set_lane_samples(uint32_t samples)
{
    std::lock_guard<std::mutex> lk(g_tuning_mu);
    return set_lane_samples(&g_tuning, samples, "vrc_set_lane_samples");
}
extern "C" int vrc_renderer_set_lane_samples(vrc_renderer* r, uint32_t samples) { return set_lane_samples(r ? &r->tuning : nullptr, samples, "vrc_renderer_set_lane_samples"); }
extern "C" const char* vrc_renderer_last_kernel(const vrc_renderer* r) { return r ? r->last_kernel : ""; }
extern "C" int vrc_renderer_set_tuning(vrc_renderer* r, uint32_t blocks_per_cu)
{
    if (!r) return fail(VRC_ERR_INVALID, "null renderer");
    return apply_tuning(r->tuning, blocks_per_cu);
}

extern "C" int vrc_renderer_create(const vrc_scene* s, uint32_t width, uint32_t height, vrc_renderer** out)
{
    if (!s || !out || width == 0 || height == 0) return fail(VRC_ERR_INVALID, "vrc_renderer_create: bad argument");
    if ((uint64_t)width * height > 0x7fffffffull) return fail(VRC_ERR_INVALID, "vrc_renderer_create: frame too large");
    HIP_TRY(hipSetDevice(s->device));
    vrc_renderer* r = new (std::nothrow) vrc_renderer();
    if (!r) return fail(VRC_ERR_OOM, "out of host memory");
    r->scene = s; r->device = s->device; r->depth = s->depth; r->width = width; r->height = height;
    { std::lock_guard<std::mutex> lk(g_tuning_mu); r->tuning = g_tuning; }
    const uint64_t n = (uint64_t)width * height;
    hipError_t e = hipMalloc(&r->d_image, n * 4);
    if (e == hipSuccess) e = hipMalloc(&r->d_accum, n * 16);
    const uint64_t n_tiles = (uint64_t)((width + 3u) / 4u) * ((height + 3u) / 4u);   // of the finest lane map (4 x 4 pixels)
    if (e == hipSuccess) e = hipMalloc(&r->d_stats, vrc::VRC_STATS_BYTES + 2 * vrc::VRC_QUEUE_BYTES);
    if (e == hipSuccess) e = hipMalloc((void**)&r->d_tile_done, n_tiles * 4);
    if (e == hipSuccess) e = hipMemset(r->d_accum, 0, n * 16);
    if (e == hipSuccess) e = hipMemset(r->d_stats, 0, vrc::VRC_STATS_BYTES + 2 * vrc::VRC_QUEUE_BYTES);
    if (e == hipSuccess) e = hipMemset(r->d_tile_done, 0, n_tiles * 4);
    r->queue_zero[0] = r->queue_zero[1] = true;
    if (e == hipSuccess) e = vrc::launch_fill_u32(r->d_image, 0xff000000u, n, nullptr);  // sf::Image::create: opaque black
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        vrc_renderer_destroy(r);
        return vrc::fail_hip(e, "vrc_renderer_create");
    }
    *out = r;
    return VRC_OK;
}

extern "C" int vrc_renderer_destroy(vrc_renderer* r)
{
    if (!r) return VRC_OK;
    (void)hipSetDevice(r->device);   // the scene may already be gone
    (void)hipFree(r->d_image);
    (void)hipFree(r->d_accum);
    (void)hipFree(r->d_stats);
    (void)hipFree(r->d_tile_done);
    delete r;
    return VRC_OK;
}

void vrc::renderer_info(const vrc_renderer* r, int* device, uint32_t* width, uint32_t* height)
{
    *device = r->device; *width = r->width; *height = r->height;
}

// The rebind RayCaster's `const LSVO& svo` (raycaster.hpp:265) has no way to do: the next frame walks another scene.
// Everything else the renderer owns is independent of the scene (the frame kernels get nodes / tex / depth per launch).
extern "C" int vrc_renderer_set_scene(vrc_renderer* r, const vrc_scene* s)
{
    if (!r || !s) return fail(VRC_ERR_INVALID, "vrc_renderer_set_scene: null argument");
    if (s->device != r->device) return fail(VRC_ERR_INVALID, "vrc_renderer_set_scene: the scene lives on device %d, the renderer on %d", s->device, r->device);
    if (s->depth != r->depth) return fail(VRC_ERR_INVALID, "vrc_renderer_set_scene: depth %u != the renderer's %u", s->depth, r->depth);
    r->scene = s;
    return VRC_OK;
}

extern "C" int vrc_renderer_set_primary_capture(vrc_renderer* r, vrc_hit* prim_dev)
{
    if (!r) return fail(VRC_ERR_INVALID, "null renderer");
    r->d_prim = prim_dev;
    return VRC_OK;
}

namespace {
// fused: resolve + pack + reset in the frame kernel (vrc_render_frame_resolved); dst: packed shard rows or NULL
int render_impl(vrc_renderer* r, const vrc_camera* cam, const vrc_frame_params* p, bool fused, void* dst, void* stream)
{
    if (!r || !cam || !p) return fail(VRC_ERR_INVALID, "vrc_render_frame: null argument");
    if (p->gi_bounces > 2) return fail(VRC_ERR_INVALID, "vrc_render_frame: gi_bounces %u > 2 not supported", p->gi_bounces);
    if (p->checker_parity < -1 || p->checker_parity > 1) return fail(VRC_ERR_INVALID, "vrc_render_frame: checker_parity must be -1, 0 or 1");
    if (p->row_block && p->shard_count > 1) {
        if (p->row_block % 8u) return fail(VRC_ERR_INVALID, "vrc_render_frame: row_block must be a multiple of 8");
        if (p->shard_index >= p->shard_count) return fail(VRC_ERR_INVALID, "vrc_render_frame: shard_index >= shard_count");
    }
    if (p->spp > VRC_MAX_SPP) return fail(VRC_ERR_INVALID, "vrc_render_frame: spp %u > %u per call", p->spp, VRC_MAX_SPP);
    const vrc_scene* s = r->scene;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(r->device));
    // the build, the work units and the grid (vrc_plan.h); an error leaves the renderer as it was
    const vrc::PlanInput in{*cam, *p, r->width, r->height, s->depth, s->cu_count, fused, r->d_prim != nullptr, r->tuning};
    vrc::FramePlan plan;
    if (int rc = vrc::plan_frame(in, plan)) return rc;
    if (!plan.kernel) return VRC_OK;
    uint32_t* const heads = (uint32_t*)((uint8_t*)r->d_stats + vrc::VRC_STATS_BYTES);
    uint32_t* sets[2] = {heads, heads + vrc::VRC_QUEUE_BYTES / 4};
    // take a set that is known to be zero (memset one if neither is: after an error exit); the launch zeroes the other
    // set, so the next launch finds its queue ready without a memset or a kernel in between
    const int use = r->queue_zero[0] ? 0 : (r->queue_zero[1] ? 1 : 0);
    if (!r->queue_zero[use]) HIP_TRY(hipMemsetAsync(sets[use], 0, vrc::VRC_QUEUE_BYTES, st));
    // Until the launch is known to have been enqueued neither set counts as zero: the other set is only zeroed BY this
    // launch (its block 0), so an error exit below must not leave it marked ready -- the next frame would take heads that
    // still hold the previous frame's consumed counts, render nothing and resolve a stale image.
    r->queue_zero[0] = r->queue_zero[1] = false;
    vrc::FrameArgs a; memset(&a, 0, sizeof(a));
    a.nodes = (const uint2*)s->d_nodes; a.tex = (const uint8_t*)s->d_tex;
    // a sample-mode frame of a shard may be resolved straight into another renderer's framebuffer (direct peer writes)
    a.image = (uint8_t*)((fused && r->image_target) ? r->image_target : r->d_image);
    a.accum = (uint32_t*)r->d_accum; a.prim = r->d_prim; a.stats = (uint64_t*)r->d_stats;
    a.queue = sets[use]; a.queue_other = sets[1 - use];
    a.depth = s->depth; a.width = r->width; a.height = r->height; a.n_items = plan.n_items; a.checker_wide = plan.checker_wide;
    a.sample_chunk = plan.sample_chunk; a.sample_chunk_tail = plan.sample_chunk_tail; a.tail_tiles = plan.tail_tiles;
    a.fused_resolve = fused ? 1u : 0u; a.reuse_invariant = r->tuning.reuse_invariant ? 1u : 0u;
    a.tile_done = r->d_tile_done; a.resolve_dst = (uint32_t*)dst;
    a.cam = *cam; a.p = plan.p;
    r->last_kernel = plan.kernel->name;
    HIP_TRY(vrc::launch_render(*plan.kernel, a, plan.grid, plan.lds, st));
    r->queue_zero[1 - use] = true;           // zeroed by the launch that is now in the stream
    return VRC_OK;
}
}  // namespace

extern "C" int vrc_render_frame(vrc_renderer* r, const vrc_camera* cam, const vrc_frame_params* p, void* stream) { return render_impl(r, cam, p, false, nullptr, stream); }

// vrc_render_frame + vrc_resolve_shard(row_block, shard_index, shard_count, dst, reset = 1) as ONE launch where the frame
// kernel can do it (stage-synchronous kernel, sample mode, no checkerboard), as those two calls otherwise.
extern "C" int vrc_render_frame_resolved(vrc_renderer* r, const vrc_camera* cam, const vrc_frame_params* p, void* dst_dev, void* stream)
{
    if (!r || !cam || !p) return fail(VRC_ERR_INVALID, "vrc_render_frame_resolved: null argument");
    if (!p->use_samples) return fail(VRC_ERR_INVALID, "vrc_render_frame_resolved: needs use_samples (there is nothing to resolve otherwise)");
    if (p->checker_parity < 0) return render_impl(r, cam, p, true, dst_dev, stream);
    int rc = render_impl(r, cam, p, false, nullptr, stream);
    if (rc) return rc;
    const bool sharded = p->row_block && p->shard_count > 1;
    return vrc_resolve_shard(r, sharded ? p->row_block : 0u, sharded ? p->shard_index : 0u, sharded ? p->shard_count : 1u, dst_dev, 1, stream);
}

extern "C" int vrc_samples_to_image(vrc_renderer* r, void* stream)
{
    if (!r) return fail(VRC_ERR_INVALID, "null renderer");
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(vrc::launch_resolve(r->d_accum, r->d_image, r->width * r->height, (hipStream_t)stream));
    return VRC_OK;
}

extern "C" int vrc_reset_samples(vrc_renderer* r, void* stream)
{
    if (!r) return fail(VRC_ERR_INVALID, "null renderer");
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipMemsetAsync(r->d_accum, 0, (uint64_t)r->width * r->height * 16, (hipStream_t)stream));
    return VRC_OK;
}

extern "C" int vrc_clear_image(vrc_renderer* r, void* stream)
{
    if (!r) return fail(VRC_ERR_INVALID, "null renderer");
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(vrc::launch_fill_u32(r->d_image, 0xff000000u, (uint64_t)r->width * r->height, (hipStream_t)stream));
    return VRC_OK;
}

// direct peer writes (vrc_ipc.cpp): the presenting rank's framebuffer, for the other ranks to open and render into
static_assert(sizeof(hipIpcMemHandle_t) <= sizeof(vrc_ipc_handle), "vrc_ipc_handle too small for hipIpcMemHandle_t");

extern "C" int vrc_ipc_export_image(vrc_renderer* r, vrc_ipc_handle* out)
{
    if (!r || !out) return fail(VRC_ERR_INVALID, "vrc_ipc_export_image: null argument");
    HIP_TRY(hipSetDevice(r->device));
    memset(out, 0, sizeof(*out));
    hipIpcMemHandle_t h;
    HIP_TRY(hipIpcGetMemHandle(&h, r->d_image));
    memcpy(out, &h, sizeof(h));
    return VRC_OK;
}

extern "C" int vrc_renderer_set_image_target(vrc_renderer* r, void* image_dev)
{
    if (!r) return fail(VRC_ERR_INVALID, "null renderer");
    r->image_target = image_dev;
    return VRC_OK;
}

extern "C" void* vrc_image_device_ptr(vrc_renderer* r) { return r ? r->d_image : nullptr; }
extern "C" void* vrc_accum_device_ptr(vrc_renderer* r) { return r ? r->d_accum : nullptr; }

namespace {
// one copy between host memory and a per-pixel buffer of the renderer, waited for; `fn` names the entry point in the message
int host_copy(vrc_renderer* r, void* vrc_renderer::*buf, uint32_t bytes_per_pixel, void* host, bool to_host, const char* fn, void* stream)
{
    if (!r || !host) return fail(VRC_ERR_INVALID, "%s: null argument", fn);
    HIP_TRY(hipSetDevice(r->device));
    const uint64_t bytes = (uint64_t)r->width * r->height * bytes_per_pixel;
    if (to_host) HIP_TRY(hipMemcpyAsync(host, r->*buf, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    else HIP_TRY(hipMemcpyAsync(r->*buf, host, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return VRC_OK;
}
}  // namespace

extern "C" int vrc_read_image(vrc_renderer* r, uint8_t* rgba_host, void* stream) { return host_copy(r, &vrc_renderer::d_image, 4, rgba_host, true, "vrc_read_image", stream); }
extern "C" int vrc_write_image(vrc_renderer* r, const uint8_t* rgba_host, void* stream) { return host_copy(r, &vrc_renderer::d_image, 4, const_cast<uint8_t*>(rgba_host), false, "vrc_write_image", stream); }
extern "C" int vrc_read_accum(vrc_renderer* r, uint32_t* accum_host, void* stream) { return host_copy(r, &vrc_renderer::d_accum, 16, accum_host, true, "vrc_read_accum", stream); }

extern "C" int vrc_get_stats(vrc_renderer* r, vrc_frame_stats* out, int reset, void* stream)
{
    if (!r || !out) return fail(VRC_ERR_INVALID, "vrc_get_stats: null argument");
    HIP_TRY(hipSetDevice(r->device));
    std::vector<uint64_t> slots(vrc::VRC_STAT_SLOTS * 8u);
    HIP_TRY(hipMemcpyAsync(slots.data(), r->d_stats, vrc::VRC_STATS_BYTES, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    uint64_t h[5] = {0, 0, 0, 0, 0};
    for (uint32_t i = 0; i < vrc::VRC_STAT_SLOTS; ++i)
        for (int k = 0; k < 5; ++k) h[k] += slots[8u * i + k];
    out->rays = h[0]; out->sum_complexity = h[1]; out->primary_hits = h[2]; out->pixels = h[3];
    out->iterations_not_executed = h[4];
    if (reset) {
        HIP_TRY(hipMemsetAsync(r->d_stats, 0, vrc::VRC_STATS_BYTES, (hipStream_t)stream));
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    }
    return VRC_OK;
}

// ---------------------------------------------------------------------------
// multi-GPU shard plumbing
// ---------------------------------------------------------------------------

static uint32_t shard_slots(uint32_t height, uint32_t row_block, uint32_t shard_count)
{
    const uint32_t nblocks = (height + row_block - 1) / row_block;
    return (nblocks + shard_count - 1) / shard_count;
}

extern "C" uint64_t vrc_shard_bytes(uint32_t width, uint32_t height, uint32_t row_block, uint32_t shard_count)
{
    if (!row_block || !shard_count) return 0;
    return (uint64_t)shard_slots(height, row_block, shard_count) * row_block * width * 4ull;
}

extern "C" int vrc_pack_shard(vrc_renderer* r, uint32_t row_block, uint32_t shard_index, uint32_t shard_count, void* dst_dev,
                              void* stream)
{
    if (!r || !dst_dev || !row_block || !shard_count || shard_index >= shard_count)
        return fail(VRC_ERR_INVALID, "vrc_pack_shard: bad argument");
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(vrc::launch_pack_shard(r->d_image, r->width, r->height, row_block, shard_index, shard_count,
                                   shard_slots(r->height, row_block, shard_count), dst_dev, (hipStream_t)stream));
    return VRC_OK;
}

extern "C" int vrc_resolve_shard(vrc_renderer* r, uint32_t row_block, uint32_t shard_index, uint32_t shard_count, void* dst_dev,
                                 int reset, void* stream)
{
    if (!r || !shard_count || shard_index >= shard_count) return fail(VRC_ERR_INVALID, "vrc_resolve_shard: bad argument");
    if (shard_count == 1 && row_block == 0) row_block = r->height;     // the whole frame as one block
    if (!row_block) return fail(VRC_ERR_INVALID, "vrc_resolve_shard: row_block is 0");
    HIP_TRY(hipSetDevice(r->device));
    uint32_t* queue = (uint32_t*)((uint8_t*)r->d_stats + vrc::VRC_STATS_BYTES);
    HIP_TRY(vrc::launch_resolve_shard(r->d_accum, r->image_target ? r->image_target : r->d_image, r->width, r->height, row_block, shard_index, shard_count,
                                      shard_slots(r->height, row_block, shard_count), dst_dev, reset ? 1u : 0u, queue,
                                      (hipStream_t)stream));
    if (reset) r->queue_zero[0] = true;     // k_resolve_shard zeroes the first set's heads in the same pass
    return VRC_OK;
}

extern "C" int vrc_unpack_shards(const void* gathered_dev, uint32_t width, uint32_t height, uint32_t row_block,
                                 uint32_t shard_count, void* image_dev, void* stream)
{
    if (!gathered_dev || !image_dev || !row_block || !shard_count || !width || !height)
        return fail(VRC_ERR_INVALID, "vrc_unpack_shards: bad argument");
    {   // no renderer here: launch on the device that owns the destination frame
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, image_dev) == hipSuccess) HIP_TRY(hipSetDevice(attr.device));
        else (void)hipGetLastError();
    }
    HIP_TRY(vrc::launch_unpack_shards(gathered_dev, width, height, row_block, shard_count,
                                      shard_slots(height, row_block, shard_count), image_dev, (hipStream_t)stream));
    return VRC_OK;
}
