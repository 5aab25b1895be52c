// vrc_api.cpp -- the C ABI declared in include/vrc.h: errors, devices, streams, scenes, the per-ray operators and the
// dense grid (the renderer is vrc_renderer.cpp, the cross-process frame flags vrc_ipc.cpp).  Compiled with hipcc into
// libvrc_hip.so together with vrc_kernels.hip and vrc_builder.cpp.  No CPU compute fallback: every entry point that
// casts rays needs a HIP device and fails loudly without one.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <new>

#include "vrc_host.h"

namespace {
thread_local char g_err[512] = "";
}

int vrc::fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

struct vrc_grid {
    int device;
    void* d_cells;
    int32_t X, Y, Z;
};

extern "C" const char* vrc_last_error(void) { return g_err; }

extern "C" int vrc_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return fail(VRC_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    return n;
}

int vrc::require_device(int device, int* cu_count)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(VRC_ERR_NO_DEVICE, "no HIP device available (%s); this library has no CPU fallback",
                    e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    if (device < 0 || device >= n) return fail(VRC_ERR_INVALID, "device %d out of range [0,%d)", device, n);
    HIP_TRY(hipSetDevice(device));
    if (cu_count) {
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, device));
        *cu_count = prop.multiProcessorCount;
    }
    return VRC_OK;
}

using vrc::require_device;

extern "C" int vrc_stream_create(int device, void** stream)
{
    if (!stream) return fail(VRC_ERR_INVALID, "vrc_stream_create: null argument");
    *stream = nullptr;
    if (int rc = require_device(device, nullptr)) return rc;
    hipStream_t st = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    *stream = st;
    return VRC_OK;
}
extern "C" int vrc_stream_destroy(int device, void* stream)
{
    if (!stream) return VRC_OK;
    if (int rc = require_device(device, nullptr)) return rc;
    HIP_TRY(hipStreamDestroy((hipStream_t)stream));
    return VRC_OK;
}
extern "C" int vrc_stream_synchronize(int device, void* stream)
{
    if (int rc = require_device(device, nullptr)) return rc;
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return VRC_OK;
}

// ---------------------------------------------------------------------------
// scene
// ---------------------------------------------------------------------------

extern "C" int vrc_scene_create(const vrc_lnode* lnodes, uint64_t n_nodes, uint32_t depth, int device, vrc_scene** out)
{
    if (!lnodes || !out || n_nodes == 0) return fail(VRC_ERR_INVALID, "vrc_scene_create: null / empty input");
    if (depth < 2 || depth > VRC_MAX_DEPTH) return fail(VRC_ERR_INVALID, "vrc_scene_create: depth %u not in [2,%d]", depth, VRC_MAX_DEPTH);
    if (n_nodes > VRC_MAX_NODES) return fail(VRC_ERR_INVALID, "vrc_scene_create: more than 2^29 nodes (4 GiB) are not addressable by the walk");
    int cus = 0;
    int rc = require_device(device, &cus);
    if (rc) return rc;
    vrc_scene* s = new (std::nothrow) vrc_scene();
    if (!s) return fail(VRC_ERR_OOM, "out of host memory");
    s->device = device; s->cu_count = cus; s->n_nodes = n_nodes; s->depth = depth;
    uint8_t* d_level = nullptr;      // n_nodes bytes of level marks, then one u32 of flags (4-byte aligned)
    const uint64_t flags_off = (n_nodes + 3ull) & ~3ull;
    uint32_t flags = 0;
    hipError_t e = hipMalloc(&s->d_nodes, n_nodes * sizeof(vrc_lnode));
    if (e == hipSuccess) e = hipMalloc(&s->d_tex, 1536);
    if (e == hipSuccess) e = hipMalloc((void**)&d_level, flags_off + 4);
    if (e == hipSuccess) e = hipMemcpy(s->d_nodes, lnodes, n_nodes * sizeof(vrc_lnode), hipMemcpyHostToDevice);
    // stray leaf bits (leaf without child: never read by the walk) are cleared in the device copy, see k_sanitize_nodes
    if (e == hipSuccess) e = vrc::launch_sanitize_nodes(s->d_nodes, n_nodes, nullptr);
    // The walk indexes nodes[parent + child_offset + slot] and its LDS stack by level without bounds checks (and drops
    // lsvo.hpp:72's lower loop bound on the strength of the tree being `depth` levels deep): verify both here, once.
    if (e == hipSuccess) e = hipMemsetAsync(d_level + flags_off, 0, 4, nullptr);
    if (e == hipSuccess) e = vrc::launch_validate_nodes(s->d_nodes, n_nodes, depth, d_level, (uint32_t*)(d_level + flags_off), nullptr);
    if (e == hipSuccess) e = hipMemcpy(&flags, d_level + flags_off, 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemset(s->d_tex, 0xff, 1536);  // sf::Color::White until textures are set
    if (d_level) (void)hipFree(d_level);
    if (e != hipSuccess) {
        vrc::scene_free(s);
        return vrc::fail_hip(e, "vrc_scene_create");
    }
    if (flags) {
        vrc::scene_free(s);
        return fail(VRC_ERR_INVALID, "vrc_scene_create: malformed LNode array:%s%s%s",
                    (flags & 1u) ? " a child block reaches past the end of the array;" : "",
                    (flags & 2u) ? " a non-leaf child below the unit-voxel level (tree deeper than `depth`);" : "",
                    (flags & 4u) ? " a node is reachable at two different levels;" : "");
    }
    *out = s;
    return VRC_OK;
}

void vrc::scene_free(vrc_scene* s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->stage_stream) { (void)hipStreamSynchronize(s->stage_stream); (void)hipStreamDestroy(s->stage_stream); }
    if (s->h_stage) (void)hipHostFree(s->h_stage);
    if (s->d_nodes) (void)hipFree(s->d_nodes);
    if (s->d_tex) (void)hipFree(s->d_tex);
    delete s;
}

extern "C" int vrc_scene_set_textures(vrc_scene* s, const uint8_t top_rgb[768], const uint8_t side_rgb[768])
{
    if (!s || !top_rgb || !side_rgb) return fail(VRC_ERR_INVALID, "vrc_scene_set_textures: null argument");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemcpy(s->d_tex, top_rgb, 768, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy((uint8_t*)s->d_tex + 768, side_rgb, 768, hipMemcpyHostToDevice));
    return VRC_OK;
}

extern "C" int vrc_scene_destroy(vrc_scene* s)
{
    vrc::scene_free(s);
    return VRC_OK;
}

extern "C" uint64_t vrc_scene_node_count(const vrc_scene* s) { return s ? s->n_nodes : 0; }
extern "C" uint32_t vrc_scene_depth(const vrc_scene* s) { return s ? s->depth : 0; }

// ---------------------------------------------------------------------------
// per-ray operator
// ---------------------------------------------------------------------------

namespace {

// Device staging for the host-memory form of the batch operators: one grow-only block per device, kept between calls
// (a hipMalloc / hipFree pair costs more than casting ten thousand rays, and hipFree synchronises the whole device),
// at most VRC_STAGE_CACHE_MAX bytes; a call that finds the block in use by another thread, or needs more than that,
// allocates privately.
constexpr size_t VRC_STAGE_CACHE_MAX = 1ull << 30;
struct StageCache {
    std::mutex mu;
    uint8_t* ptr = nullptr;
    size_t cap = 0;
};
StageCache g_stage_cache[16];

// Stage host ray buffers through device memory around `launch`.
template <class Launch>
int staged_cast(int device, uint64_t n, const float* org, const float* dir, const float* coef, const float* bias, vrc_hit* out,
                hipStream_t st, Launch launch)
{
    // one block: hits (48 B, 16-byte aligned records first) | origins | directions | coef | bias
    const size_t need = n * (sizeof(vrc_hit) + 12 + 12 + 4 + 4);
    StageCache* cache = (device >= 0 && device < 16 && need <= VRC_STAGE_CACHE_MAX) ? &g_stage_cache[device] : nullptr;
    std::unique_lock<std::mutex> lk;
    if (cache) {
        lk = std::unique_lock<std::mutex>(cache->mu, std::try_to_lock);
        if (!lk.owns_lock()) cache = nullptr;
    }
    float *d_org = nullptr, *d_dir = nullptr, *d_coef = nullptr, *d_bias = nullptr;
    vrc_hit* d_out = nullptr;
    uint8_t* arena = nullptr;
    hipError_t e = hipSuccess;
    if (cache) {
        if (cache->cap < need) {
            if (cache->ptr) (void)hipFree(cache->ptr);
            cache->ptr = nullptr; cache->cap = 0;
            e = hipMalloc((void**)&cache->ptr, need);
            if (e == hipSuccess) cache->cap = need;
        }
        arena = cache->ptr;
    } else {
        e = hipMalloc((void**)&arena, need);
    }
    if (e == hipSuccess) {
        d_out = (vrc_hit*)arena;
        d_org = (float*)(arena + n * sizeof(vrc_hit));
        d_dir = d_org + 3 * n;
        if (coef) d_coef = d_dir + 3 * n;
        if (bias) d_bias = d_dir + 4 * n;
    }
    if (e == hipSuccess) e = hipMemcpyAsync(d_org, org, n * 12, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_dir, dir, n * 12, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && coef) e = hipMemcpyAsync(d_coef, coef, n * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && bias) e = hipMemcpyAsync(d_bias, bias, n * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = launch(d_org, d_dir, d_coef, d_bias, d_out);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, n * sizeof(vrc_hit), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (!cache && arena) (void)hipFree(arena);
    if (e != hipSuccess) return vrc::fail_hip(e, "cast_rays");
    return VRC_OK;
}

}  // namespace

extern "C" int vrc_cast_rays(const vrc_scene* s, uint64_t n, const float* org_xyz, const float* dir_xyz, const float* coef,
                             const float* bias, vrc_hit* out, int mem, void* stream)
{
    if (!s) return fail(VRC_ERR_INVALID, "vrc_cast_rays: null scene");
    if (n == 0) return VRC_OK;
    if (!org_xyz || !dir_xyz || !out) return fail(VRC_ERR_INVALID, "vrc_cast_rays: null buffer");
    if (n > 0xffffffffull * 256ull) return fail(VRC_ERR_INVALID, "vrc_cast_rays: too many rays for one launch");
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    if (mem == VRC_MEM_DEVICE) {
        HIP_TRY(vrc::launch_cast_rays(s->d_nodes, (int)s->depth, n, org_xyz, dir_xyz, coef, bias, out, st));
        return VRC_OK;
    }
    if (mem != VRC_MEM_HOST) return fail(VRC_ERR_INVALID, "vrc_cast_rays: bad mem kind %d", mem);
    return staged_cast(s->device, n, org_xyz, dir_xyz, coef, bias, out, st,
                       [&](float* o, float* d, float* c, float* b, vrc_hit* h) {
                           return vrc::launch_cast_rays(s->d_nodes, (int)s->depth, n, o, d, c, b, h, st);
                       });
}

extern "C" int vrc_cast_ray_chains(const vrc_scene* s, uint64_t n, const float* org_a_xyz, const float* dir_a_xyz, const float* org_b_xyz,
                                   const float* dir_b_xyz, float coef_b, vrc_hit* out_a, vrc_hit* out_b, uint32_t* not_executed, void* stream)
{
    if (!s) return fail(VRC_ERR_INVALID, "vrc_cast_ray_chains: null scene");
    if (n == 0) return VRC_OK;
    if (!org_a_xyz || !dir_a_xyz || !org_b_xyz || !dir_b_xyz || !out_a || !out_b) return fail(VRC_ERR_INVALID, "vrc_cast_ray_chains: null buffer");
    if (!(coef_b >= 0.0f && coef_b <= 0.5f)) return fail(VRC_ERR_INVALID, "vrc_cast_ray_chains: coef_b = %g outside [0, 0.5] (the start below the root is proven for those)", (double)coef_b);
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(vrc::launch_cast_ray_chains(s->d_nodes, (int)s->depth, n, org_a_xyz, dir_a_xyz, org_b_xyz, dir_b_xyz, coef_b, out_a, out_b,
                                        not_executed, (hipStream_t)stream));
    return VRC_OK;
}

// Camera::getClosestPoint (camera_controller.hpp:56-60, once per frame, main.cpp:115): the ray goes through the scene's
// pinned slot -- the kernel reads it from host memory and writes the HitPoint back there; the call is a 32-byte store,
// one launch on the scene's own stream, a wait for that stream and a 48-byte load.
extern "C" int vrc_cast_ray(const vrc_scene* cs, const float org[3], const float dir[3], float ray_size_coef,
                            float ray_size_bias, vrc_hit* out)
{
    if (!cs || !org || !dir || !out) return fail(VRC_ERR_INVALID, "vrc_cast_ray: null argument");
    vrc_scene* s = const_cast<vrc_scene*>(cs);
    HIP_TRY(hipSetDevice(s->device));
    std::lock_guard<std::mutex> lk(s->stage_mu);
    if (!s->h_stage) {
        void* p = nullptr;
        HIP_TRY(hipHostMalloc(&p, 128, hipHostMallocMapped));
        hipStream_t st = nullptr;
        hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
        if (e != hipSuccess) { (void)hipHostFree(p); return fail(VRC_ERR_HIP, "vrc_cast_ray: %s", hipGetErrorString(e)); }
        s->h_stage = p; s->stage_stream = st;
    }
    float* in = (float*)s->h_stage;                       // org[3] dir[3] coef bias | (64) vrc_hit
    vrc_hit* res = (vrc_hit*)((uint8_t*)s->h_stage + 64);
    in[0] = org[0]; in[1] = org[1]; in[2] = org[2]; in[3] = dir[0]; in[4] = dir[1]; in[5] = dir[2];
    in[6] = ray_size_coef; in[7] = ray_size_bias;
    void* dev = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&dev, s->h_stage, 0));
    float* din = (float*)dev;
    HIP_TRY(vrc::launch_cast_rays(s->d_nodes, (int)s->depth, 1, din, din + 3, din + 6, din + 7, (vrc_hit*)((uint8_t*)dev + 64), s->stage_stream));
    HIP_TRY(hipStreamSynchronize(s->stage_stream));
    *out = *res;
    return VRC_OK;
}

// ---------------------------------------------------------------------------
// dense grid
// ---------------------------------------------------------------------------

extern "C" int vrc_grid_create(const uint8_t* cells, int32_t X, int32_t Y, int32_t Z, int device, vrc_grid** out)
{
    if (!cells || !out || X <= 0 || Y <= 0 || Z <= 0) return fail(VRC_ERR_INVALID, "vrc_grid_create: bad argument");
    int rc = require_device(device, nullptr);
    if (rc) return rc;
    vrc_grid* g = (vrc_grid*)calloc(1, sizeof(vrc_grid));
    if (!g) return fail(VRC_ERR_OOM, "out of host memory");
    g->device = device; g->X = X; g->Y = Y; g->Z = Z;
    const size_t bytes = (size_t)X * Y * Z;
    hipError_t e = hipMalloc(&g->d_cells, bytes);
    if (e == hipSuccess) e = hipMemcpy(g->d_cells, cells, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (g->d_cells) (void)hipFree(g->d_cells);
        free(g);
        return vrc::fail_hip(e, "vrc_grid_create");
    }
    *out = g;
    return VRC_OK;
}

extern "C" int vrc_grid_destroy(vrc_grid* g)
{
    if (!g) return VRC_OK;
    (void)hipSetDevice(g->device);
    (void)hipFree(g->d_cells);
    free(g);
    return VRC_OK;
}

extern "C" int vrc_grid_cast_rays(const vrc_grid* g, uint64_t n, const float* org_xyz, const float* dir_xyz, vrc_hit* out,
                                  int mem, void* stream)
{
    if (!g) return fail(VRC_ERR_INVALID, "vrc_grid_cast_rays: null grid");
    if (n == 0) return VRC_OK;
    if (!org_xyz || !dir_xyz || !out) return fail(VRC_ERR_INVALID, "vrc_grid_cast_rays: null buffer");
    HIP_TRY(hipSetDevice(g->device));
    hipStream_t st = (hipStream_t)stream;
    if (mem == VRC_MEM_DEVICE) {
        HIP_TRY(vrc::launch_grid_cast((const uint8_t*)g->d_cells, g->X, g->Y, g->Z, n, org_xyz, dir_xyz, out, st));
        return VRC_OK;
    }
    if (mem != VRC_MEM_HOST) return fail(VRC_ERR_INVALID, "vrc_grid_cast_rays: bad mem kind %d", mem);
    return staged_cast(g->device, n, org_xyz, dir_xyz, nullptr, nullptr, out, st,
                       [&](float* o, float* d, float*, float*, vrc_hit* h) {
                           return vrc::launch_grid_cast((const uint8_t*)g->d_cells, g->X, g->Y, g->Z, n, o, d, h, st);
                       });
}

// Host arithmetic only.  position is in [1, 2)^3 and strictly inside the hit cell (lsvo.hpp:156-158), so (p - 1) * S
// is exact in float and its floor is the cell the WALK saw; the walk sees the scene point-reflected through the cube
// centre (child_shift = child_offset ^ mirror_mask, lsvo.hpp:79), hence S-1 - cell in setCell
// coordinates.  The normal points out of the hit face in walk space, i.e. towards -normal in setCell space.
extern "C" int vrc_hit_to_voxel(uint32_t depth, const vrc_hit* hit, uint32_t voxel[3], uint32_t neighbour[3], int* has_neighbour)
{
    if (!hit || !voxel) return fail(VRC_ERR_INVALID, "vrc_hit_to_voxel: null argument");
    if (depth < 2 || depth > VRC_MAX_DEPTH) return fail(VRC_ERR_INVALID, "vrc_hit_to_voxel: depth %u not in [2,%d]", depth, VRC_MAX_DEPTH);
    if ((hit->hit & 0xffu) != 1u) return fail(VRC_ERR_INVALID, "vrc_hit_to_voxel: not a unit-voxel hit (kind %u: 0 = miss, 2 = LOD cut-off)", hit->hit & 0xffu);
    const float S = (float)(1u << depth);
    int32_t cell[3];
    for (int a = 0; a < 3; ++a) {
        const float f = std::floor((hit->position[a] - 1.0f) * S);
        if (!(f >= 0.0f && f < S)) return fail(VRC_ERR_INVALID, "vrc_hit_to_voxel: position outside [1,2)^3");
        cell[a] = (int32_t)(1u << depth) - 1 - (int32_t)f;
        voxel[a] = (uint32_t)cell[a];
    }
    int axis = -1, axes = 0;
    for (int a = 0; a < 3; ++a) if (hit->normal[a] != 0.0f) { axis = a; ++axes; }
    int has = 0;
    if (axes == 1) {
        cell[axis] -= hit->normal[axis] > 0.0f ? 1 : -1;
        has = cell[axis] >= 0 && cell[axis] < (int32_t)(1u << depth);
    }
    if (neighbour) for (int a = 0; a < 3; ++a) neighbour[a] = has ? (uint32_t)cell[a] : 0u;
    if (has_neighbour) *has_neighbour = has;
    return VRC_OK;
}

// Host arithmetic only, in doubles.  rot is vrc_make_rotation's layout (columns), so R[b][a] -- the entry of the INVERSE
// rotation's row a, column b -- is rot[3a + b].  The one body of vrc_affine_place and vrc_affine_place_box: the map, and the
// bounding box of the forward image of the source box [src_lo, src_hi] (continuous coordinates), two voxels wider on every
// side, clipped to dst.  The caller has refused NULLs and bad depths.
static int place_box(const char* what, const float rot[9], float scale, const float src_pivot[3], const float dst_pivot[3], const double src_lo[3],
                     const double src_hi[3], uint32_t dst_depth, vrc_affine* map, uint32_t dst_lo[3], uint32_t dst_hi[3])
{
    bool finite = std::isfinite(scale);
    for (int i = 0; i < 9; ++i) finite = finite && std::isfinite(rot[i]);
    for (int a = 0; a < 3; ++a) finite = finite && std::isfinite(src_pivot[a]) && std::isfinite(dst_pivot[a]);
    if (!finite) return fail(VRC_ERR_INVALID, "%s: NaN or infinite input", what);
    if (!(scale > 0.0f)) return fail(VRC_ERR_INVALID, "%s: scale %g is not positive", what, (double)scale);
    if (scale < 0.0625f) return fail(VRC_ERR_INVALID, "%s: scale %g below 1/16, the smallest scale the map's 2^20 limit admits for a rotation", what, (double)scale);
    vrc_affine out;
    out.reserved = 0;
    for (int a = 0; a < 3; ++a) {
        double sum[3];
        for (int b = 0; b < 3; ++b) {
            const double m = std::nearbyint(65536.0 * (double)rot[3 * a + b] / (double)scale);
            if (!(std::fabs(m) <= 1048576.0)) return fail(VRC_ERR_INVALID, "%s: m[%d] = %g beyond +-2^20", what, 3 * a + b, m);
            out.m[3 * a + b] = (int32_t)m;
            sum[b] = m * 2.0 * (double)dst_pivot[b];
        }
        const double t = std::nearbyint(131072.0 * (double)src_pivot[a] - ((sum[0] + sum[1]) + sum[2]));
        if (!(std::fabs(t) <= 1099511627776.0)) return fail(VRC_ERR_INVALID, "%s: t[%d] = %g beyond +-2^40", what, a, t);
        out.t[a] = (int64_t)t;
    }
    const double Sd = (double)(1u << dst_depth);
    uint32_t lo[3], hi[3];
    bool empty = false;
    for (int r = 0; r < 3; ++r) {
        double least = 0.0, most = 0.0;
        for (int corner = 0; corner < 8; ++corner) {
            double x = (double)dst_pivot[r];
            for (int c = 0; c < 3; ++c)
                x += (double)scale * (double)rot[3 * c + r] * (((corner >> c) & 1 ? src_hi[c] : src_lo[c]) - (double)src_pivot[c]);
            if (corner == 0 || x < least) least = x;
            if (corner == 0 || x > most) most = x;
        }
        double l = std::floor(least) - 2.0, h = std::ceil(most) + 2.0;
        if (l < 0.0) l = 0.0;
        if (h > Sd) h = Sd;
        if (!(l < h)) { empty = true; l = h = 0.0; }
        lo[r] = (uint32_t)l; hi[r] = (uint32_t)h;
    }
    for (int a = 0; a < 3; ++a) { dst_lo[a] = empty ? 0u : lo[a]; dst_hi[a] = empty ? 0u : hi[a]; }
    *map = out;
    return VRC_OK;
}

extern "C" int vrc_affine_place(const float rot[9], float scale, const float src_pivot[3], const float dst_pivot[3], uint32_t src_depth,
                                uint32_t dst_depth, vrc_affine* map, uint32_t dst_lo[3], uint32_t dst_hi[3])
{
    const char* what = "vrc_affine_place";
    if (!rot || !src_pivot || !dst_pivot || !map || !dst_lo || !dst_hi) return fail(VRC_ERR_INVALID, "%s: null argument", what);
    if (src_depth < 2 || src_depth > 10 || dst_depth < 2 || dst_depth > 10)
        return fail(VRC_ERR_INVALID, "%s: depths %u and %u not in [2,10]", what, src_depth, dst_depth);
    const double Ss = (double)(1u << src_depth), lo[3] = {0.0, 0.0, 0.0}, hi[3] = {Ss, Ss, Ss};
    return place_box(what, rot, scale, src_pivot, dst_pivot, lo, hi, dst_depth, map, dst_lo, dst_hi);
}

extern "C" int vrc_affine_place_box(const float rot[9], float scale, const float src_pivot[3], const float dst_pivot[3], const uint32_t src_lo[3],
                                    const uint32_t src_hi[3], uint32_t dst_depth, vrc_affine* map, uint32_t dst_lo[3], uint32_t dst_hi[3])
{
    const char* what = "vrc_affine_place_box";
    if (!rot || !src_pivot || !dst_pivot || !src_lo || !src_hi || !map || !dst_lo || !dst_hi) return fail(VRC_ERR_INVALID, "%s: null argument", what);
    if (dst_depth < 2 || dst_depth > 10) return fail(VRC_ERR_INVALID, "%s: depth %u not in [2,10]", what, dst_depth);
    double lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        if (src_lo[a] > src_hi[a]) return fail(VRC_ERR_INVALID, "%s: source box inverted on axis %d: %u above %u", what, a, src_lo[a], src_hi[a]);
        lo[a] = (double)src_lo[a]; hi[a] = (double)src_hi[a];
    }
    return place_box(what, rot, scale, src_pivot, dst_pivot, lo, hi, dst_depth, map, dst_lo, dst_hi);
}

// The kernels replace some IEEE divisions / square roots by short sequences that are proven equal on the ranges they
// are used on; this runs that proof on the device: every float bit pattern of those ranges (~4.3 x 10^9 evaluations, a
// fraction of a second).  mismatches[0..3]: reciprocal, square root, 1 / sqrt composition, get_rand -- all must be 0.
extern "C" int vrc_selftest_exact_arith(int device, uint64_t mismatches[4])
{
    if (!mismatches) return fail(VRC_ERR_INVALID, "vrc_selftest_exact_arith: null argument");
    int rc = require_device(device, nullptr);
    if (rc) return rc;
    unsigned long long* d = nullptr;
    HIP_TRY(hipMalloc((void**)&d, 32));
    hipError_t e = hipMemset(d, 0, 32);
    if (e == hipSuccess) e = vrc::launch_selftest_exact_arith(d, nullptr);
    if (e == hipSuccess) e = hipMemcpy(mismatches, d, 32, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(VRC_ERR_HIP, "vrc_selftest_exact_arith: %s", hipGetErrorString(e));
    return VRC_OK;
}

// ---------------------------------------------------------------------------
// host helper: generateRotationMatrix (utils.cpp:94-100) = mat3(ry * rx) with
// rx = rotate(I, -angle.x, Y), ry = rotate(I, -angle.y, X); glm::rotate is the
// axis-angle form.  Columns m[0], m[1], m[2].
// ---------------------------------------------------------------------------

namespace {
struct M4 { float c[4][4]; };
M4 m4_identity()
{
    M4 m;
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) m.c[i][j] = (i == j) ? 1.0f : 0.0f;
    return m;
}
M4 m4_rotate(const M4& m, float angle, float ax, float ay, float az)
{
    const float c = std::cos(angle), s = std::sin(angle);
    const float inv = 1.0f / std::sqrt((ax * ax + ay * ay) + az * az);
    ax *= inv; ay *= inv; az *= inv;
    const float tx = (1.0f - c) * ax, ty = (1.0f - c) * ay, tz = (1.0f - c) * az;
    float R[3][3];
    R[0][0] = c + tx * ax;      R[0][1] = tx * ay + s * az; R[0][2] = tx * az - s * ay;
    R[1][0] = ty * ax - s * az; R[1][1] = c + ty * ay;      R[1][2] = ty * az + s * ax;
    R[2][0] = tz * ax + s * ay; R[2][1] = tz * ay - s * ax; R[2][2] = c + tz * az;
    M4 out;
    for (int i = 0; i < 3; ++i)
        for (int r = 0; r < 4; ++r) out.c[i][r] = (m.c[0][r] * R[i][0] + m.c[1][r] * R[i][1]) + m.c[2][r] * R[i][2];
    for (int r = 0; r < 4; ++r) out.c[3][r] = m.c[3][r];
    return out;
}
M4 m4_mul(const M4& A, const M4& B)
{
    M4 out;
    for (int j = 0; j < 4; ++j)
        for (int r = 0; r < 4; ++r)
            out.c[j][r] = ((A.c[0][r] * B.c[j][0] + A.c[1][r] * B.c[j][1]) + A.c[2][r] * B.c[j][2]) + A.c[3][r] * B.c[j][3];
    return out;
}
}  // namespace

extern "C" void vrc_make_rotation(float angle_x, float angle_y, float rot[9])
{
    const M4 rx = m4_rotate(m4_identity(), -angle_x, 0.0f, 1.0f, 0.0f);
    const M4 ry = m4_rotate(m4_identity(), -angle_y, 1.0f, 0.0f, 0.0f);
    const M4 m = m4_mul(ry, rx);
    for (int j = 0; j < 3; ++j)
        for (int r = 0; r < 3; ++r) rot[j * 3 + r] = m.c[j][r];
}
