// hip_raycaster.hpp -- C++ host adapter over the C ABI (include/vrc.h) that
// presents the reference's operator interface for the hot path:
//
//   vrc_host::HipLSVO       <- LSVO<N> : Volumetric   (include/lsvo.hpp:10-33,
//                              include/volumetric.hpp:55-61): castRay / setCell
//   vrc_host::HipRayCaster  <- RayCaster (include/raycaster.hpp:43-283):
//                              setLightPosition, renderRay's per-frame batch
//                              (renderFrame), samples_to_image, resetSamples,
//                              public flags use_gi / use_samples, render_image
//   vrc_host::HipVoxelVolume<- the write half of Volumetric (setCell, volumetric.hpp:59):
//                              batched edits of a device-resident occupancy, commit()
//                              builds a new HipLSVO, HipRayCaster::setScene shows it
//
// Header-only, C++14, no GLM / SFML needed.  When the reference's own headers
// are on the include path, define VRC_WITH_REFERENCE_HEADERS before including
// this file to also get `HipVolumetric`, a real `Volumetric` subclass that can
// be handed to Camera::getClosestPoint and friends unchanged.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <fstream>
#include <iterator>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/vrc.h"

namespace vrc_host {

struct Vec3 { float x, y, z; };   // layout-compatible with glm::vec3
struct Vec2 { float x, y; };

// include/cell.hpp:3-24 -- every LSVO hit reports this one cell (lsvo.hpp:21-23)
struct Cell {
    enum Type { Empty, Solid, Mirror };
    enum Texture { None, Grass, Red, White };
    Type type = Solid;
    Texture texture = Grass;
};

// include/volumetric.hpp:7-22
struct HitPoint {
    Vec3 position{0, 0, 0};
    Vec3 normal{0, 0, 0};
    Vec2 voxel_coord{0, 0};
    const Cell* cell = nullptr;   // nullptr = miss
    float distance = 0.0f;
    uint32_t complexity = 0u;
};

inline void check(int rc, const char* what)
{
    if (rc != VRC_OK) throw std::runtime_error(std::string(what) + ": " + vrc_last_error());
}

// The albedo tables as the reference gets them: sf::Image::loadFromFile("res/grass_top_16x16.bmp") and getPixel(x, y)
// (raycaster.hpp:53-54,239) -- an uncompressed 24- or 32-bpp BMP decoded to RGB rows, top row first.  Returns
// width * height * 3 bytes (768 for the reference's 16 x 16 files); throws on anything else.
inline std::vector<uint8_t> loadBMP(const std::string& path, uint32_t* width = nullptr, uint32_t* height = nullptr)
{
    std::ifstream f(path, std::ios::binary);
    std::vector<uint8_t> d((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    auto u32 = [&](size_t o) { return (uint32_t)d[o] | ((uint32_t)d[o + 1] << 8) | ((uint32_t)d[o + 2] << 16) | ((uint32_t)d[o + 3] << 24); };
    auto u16 = [&](size_t o) { return (uint32_t)d[o] | ((uint32_t)d[o + 1] << 8); };
    if (d.size() < 54 || d[0] != 'B' || d[1] != 'M') throw std::runtime_error("loadBMP: not a BMP file: " + path);
    const uint32_t off = u32(10), bpp = u16(28), comp = u32(30);
    const int32_t w = (int32_t)u32(18), hs = (int32_t)u32(22);
    const uint32_t h = (uint32_t)(hs < 0 ? -hs : hs);
    if (w <= 0 || w > 16384 || h == 0 || h > 16384 || (bpp != 24 && bpp != 32) || (comp != 0 && !(comp == 3 && bpp == 32)))
        throw std::runtime_error("loadBMP: only uncompressed 24 / 32 bpp is supported: " + path);
    const size_t stride = ((size_t)w * (bpp / 8) + 3) & ~(size_t)3;
    if (d.size() < off + stride * h) throw std::runtime_error("loadBMP: truncated file: " + path);
    std::vector<uint8_t> rgb((size_t)w * h * 3);
    for (uint32_t row = 0; row < h; ++row) {
        const uint32_t y = hs < 0 ? row : h - 1 - row;          // positive height: the file's first row is the bottom one
        const uint8_t* line = d.data() + off + stride * row;
        for (int32_t x = 0; x < w; ++x) {
            const uint8_t* px = line + (size_t)x * (bpp / 8);    // B, G, R [, A]
            uint8_t* o = rgb.data() + ((size_t)y * w + x) * 3;
            o[0] = px[2]; o[1] = px[1]; o[2] = px[0];
        }
    }
    if (width) *width = (uint32_t)w;
    if (height) *height = h;
    return rgb;
}

// LSVO<N> (lsvo.hpp:10): immutable, device resident; castRay is const and may be
// called from any number of threads, like the reference's (main.cpp:139-152).
class HipLSVO {
public:
    // LSVO(const SVO<N>&) + compileSVO replaced by a pre-compiled LNode array
    HipLSVO(const vrc_lnode* lnodes, uint64_t n_nodes, uint32_t depth, int device = 0) : device_(device)
    {
        check(vrc_scene_create(lnodes, n_nodes, depth, device, &scene_), "vrc_scene_create");
    }
    // main.cpp:59-88 on the device: FastNoise heights (seed as main.cpp:61) -> voxels -> LSVO, straight into HBM
    static std::unique_ptr<HipLSVO> fromFastNoiseTerrain(int32_t seed, uint32_t depth, int device = 0, float* build_ms = nullptr)
    {
        vrc_scene* s = nullptr;
        check(vrc_scene_build_fastnoise_terrain(seed, depth, device, &s, build_ms), "vrc_scene_build_fastnoise_terrain");
        return std::unique_ptr<HipLSVO>(new HipLSVO(s, device));
    }
    ~HipLSVO() { vrc_scene_destroy(scene_); }
    HipLSVO(const HipLSVO&) = delete;
    HipLSVO& operator=(const HipLSVO&) = delete;

    // lsvo.hpp:26 -- a no-op in the reference too
    void setCell(Cell::Type, Cell::Texture, uint32_t, uint32_t, uint32_t) {}

    // lsvo.hpp:33
    HitPoint castRay(const Vec3& position, Vec3 d, const float ray_size_coef = 0.0f, const float ray_size_bias = 0.0f) const
    {
        vrc_hit h;
        const float o[3] = {position.x, position.y, position.z}, dir[3] = {d.x, d.y, d.z};
        check(vrc_cast_ray(scene_, o, dir, ray_size_coef, ray_size_bias, &h), "vrc_cast_ray");
        return convert(h);
    }

    // batch form: what a GPU-backed Volumetric needs to be useful
    std::vector<HitPoint> castRays(const std::vector<Vec3>& positions, const std::vector<Vec3>& directions,
                                   float ray_size_coef = 0.0f, float ray_size_bias = 0.0f) const
    {
        if (positions.size() != directions.size()) throw std::invalid_argument("castRays: size mismatch");
        const uint64_t n = positions.size();
        std::vector<vrc_hit> raw(n);
        std::vector<float> coef(n, ray_size_coef), bias(n, ray_size_bias);
        check(vrc_cast_rays(scene_, n, &positions[0].x, &directions[0].x, coef.data(), bias.data(), raw.data(),
                            VRC_MEM_HOST, nullptr), "vrc_cast_rays");
        std::vector<HitPoint> out(n);
        for (uint64_t i = 0; i < n; ++i) out[i] = convert(raw[i]);
        return out;
    }

    // the same batch as raw records (include/vrc.h: vrc_hit), e.g. for HipVoxelVolume::fillSpheresAtHits
    std::vector<vrc_hit> castRaysRecords(const std::vector<Vec3>& positions, const std::vector<Vec3>& directions) const
    {
        if (positions.size() != directions.size()) throw std::invalid_argument("castRaysRecords: size mismatch");
        std::vector<vrc_hit> raw(positions.size());
        if (!raw.empty())
            check(vrc_cast_rays(scene_, raw.size(), &positions[0].x, &directions[0].x, nullptr, nullptr, raw.data(), VRC_MEM_HOST, nullptr),
                  "vrc_cast_rays");
        return raw;
    }

    // pairs of casts as RayCaster::castRay chains them (raycaster.hpp:131 -> :153; :194 -> :198), device buffers: ray A, then
    // ray B next to A's hit, started below the root as the frame kernels start their secondary rays (vrc_cast_ray_chains);
    // hits_b[i] equals a cast of ray B alone.  Asynchronous on `stream`.
    void castRayChainsDevice(uint64_t n, const float* org_a_dev, const float* dir_a_dev, const float* org_b_dev, const float* dir_b_dev,
                             float ray_size_coef_b, vrc_hit* hits_a_dev, vrc_hit* hits_b_dev, uint32_t* not_executed_dev = nullptr,
                             void* stream = nullptr) const
    {
        check(vrc_cast_ray_chains(scene_, n, org_a_dev, dir_a_dev, org_b_dev, dir_b_dev, ray_size_coef_b, hits_a_dev, hits_b_dev,
                                  not_executed_dev, stream), "vrc_cast_ray_chains");
    }

    // RayCaster's constructor loads the two 16 x 16 tables relative to the working directory (raycaster.hpp:53-54);
    // here the caller names the files
    void loadTextures(const std::string& top_bmp, const std::string& side_bmp)
    {
        uint32_t w = 0, h = 0;
        const std::vector<uint8_t> top = loadBMP(top_bmp, &w, &h);
        if (w != 16 || h != 16) throw std::runtime_error("loadTextures: " + top_bmp + " is not 16 x 16");
        const std::vector<uint8_t> side = loadBMP(side_bmp, &w, &h);
        if (w != 16 || h != 16) throw std::runtime_error("loadTextures: " + side_bmp + " is not 16 x 16");
        check(vrc_scene_set_textures(scene_, top.data(), side.data()), "vrc_scene_set_textures");
    }

    vrc_scene* handle() const { return scene_; }
    uint32_t depth() const { return vrc_scene_depth(scene_); }
    int device() const { return device_; }
    Cell cell;   // lsvo.hpp:289

private:
    HitPoint convert(const vrc_hit& h) const
    {
        HitPoint p;
        p.position = {h.position[0], h.position[1], h.position[2]};
        p.normal = {h.normal[0], h.normal[1], h.normal[2]};
        p.voxel_coord = {h.voxel_coord[0], h.voxel_coord[1]};
        p.cell = h.hit ? &cell : nullptr;
        p.distance = h.distance;
        p.complexity = h.complexity;
        return p;
    }
    friend class HipVoxelVolume;
    HipLSVO(vrc_scene* adopted, int device) : scene_(adopted), device_(device) {}
    vrc_scene* scene_ = nullptr;
    int device_ = 0;
};

class HipVoxelVolume;
class HipVoxelDistance;
class HipVoxelDelta;

// mass, centre of mass (continuous voxel coordinates) and inertia tensor about it (row-major) of one piece, a voxel being a
// unit cube of unit mass (include/vrc.h: vrc_rigid_moments).  Mass and centre are the exact values rounded once; an inertia
// entry goes through long double (a numerator of up to 82 bits, a division, a sum) before it is rounded to double: within one
// unit in the last place of the exact value, not the correctly rounded one the Python layer's rationals give.
struct HipMassProperties {
    double mass = 0.0;
    double centre[3] = {0.0, 0.0, 0.0};
    double inertia[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
};

// The pieces of a volume, named (include/vrc.h: vrc_volume_label_components): a snapshot on the device that later edits
// of the volume do not change.  Ids run 0 .. count() - 1 by ascending key of each piece's first voxel.  Movable, RAII.
class HipVoxelLabels {
public:
    ~HipVoxelLabels() { vrc_labels_destroy(l_); }
    HipVoxelLabels(HipVoxelLabels&& o) noexcept : l_(o.l_) { o.l_ = nullptr; }
    HipVoxelLabels& operator=(HipVoxelLabels&& o) noexcept
    {
        if (this != &o) { vrc_labels_destroy(l_); l_ = o.l_; o.l_ = nullptr; }
        return *this;
    }
    HipVoxelLabels(const HipVoxelLabels&) = delete;
    HipVoxelLabels& operator=(const HipVoxelLabels&) = delete;

    uint64_t count() const { return vrc_labels_count(l_); }
    uint32_t depth() const { return vrc_labels_depth(l_); }
    uint64_t bytes() const { return vrc_labels_bytes(l_); }
    // the records [first, first + capacity) that exist, in id order
    std::vector<vrc_component> components(uint64_t first = 0, uint64_t capacity = ~0ull) const
    {
        const uint64_t C = count(), n = first < C ? std::min(capacity, C - first) : 0;
        std::vector<vrc_component> out((size_t)n);
        if (n) check(vrc_labels_components(l_, first, n, out.data(), VRC_MEM_HOST, nullptr), "vrc_labels_components");
        return out;
    }
    // the piece of each of n voxels (xyz: n x 3), VRC_NO_COMPONENT outside M or outside the volume
    std::vector<uint32_t> at(const uint32_t* xyz, uint64_t n) const
    {
        std::vector<uint32_t> ids((size_t)n);
        check(vrc_labels_at(l_, n, xyz, ids.data(), VRC_MEM_HOST, nullptr), "vrc_labels_at");
        return ids;
    }
    // dst becomes (VRC_COPY_REPLACE) / gains (_OR) / loses (_ANDNOT) the voxels of the pieces with keep[id] != 0
    inline void select(const std::vector<uint8_t>& keep, HipVoxelVolume& dst, int op = VRC_COPY_REPLACE) const;
    // How far every piece can fall as a rigid body along `direction` (a VRC_FACE_* code: on the terrain generator's scenes
    // down is VRC_FACE_YN) before it meets a solid voxel of `fixed` (nullptr: nothing), the volume's face, drop_limit
    // (0 = none) or a piece that has come to rest (include/vrc.h: vrc_fall_drops): count() x 3 offsets D_i * g.
    inline std::vector<int32_t> fall(HipVoxelVolume* fixed, int direction, uint32_t drop_limit = 0, vrc_fall_stats* stats = nullptr) const;
    // dst gains (VRC_COPY_OR) or loses (VRC_COPY_ANDNOT) every voxel of the pieces with keep[id] != 0 (nullptr: all), each
    // piece moved by its own offset; what leaves the volume is dropped
    inline void place(const std::vector<int32_t>& offsets, HipVoxelVolume& dst, int op = VRC_COPY_OR, const std::vector<uint8_t>* keep = nullptr) const;
    // the raw moments of the pieces [first, first + capacity) that exist (include/vrc.h: vrc_rigid_moments), exact integers
    std::vector<vrc_piece_moments> moments(uint64_t first = 0, uint64_t capacity = ~0ull) const
    {
        const uint64_t C = count(), n = first < C ? std::min(capacity, C - first) : 0;
        std::vector<vrc_piece_moments> out((size_t)n);
        if (n) check(vrc_rigid_moments(l_, first, n, out.data(), VRC_MEM_HOST, nullptr), "vrc_rigid_moments");
        return out;
    }
    // labels made by HipVoxelVolume::fracture: the site whose cell each piece of [first, first + capacity) lies in,
    // VRC_NO_COMPONENT for "none" (include/vrc.h: vrc_fracture_piece_sites)
    std::vector<uint32_t> pieceSites(uint64_t first = 0, uint64_t capacity = ~0ull) const
    {
        const uint64_t C = count(), n = first < C ? std::min(capacity, C - first) : 0;
        std::vector<uint32_t> out((size_t)n);
        check(vrc_fracture_piece_sites(l_, first, n, n ? out.data() : nullptr, VRC_MEM_HOST, nullptr), "vrc_fracture_piece_sites");
        return out;
    }
    // what a physics engine starts from: the integer sums combined in 128-bit integers, then long double (see HipMassProperties)
    std::vector<HipMassProperties> massProperties(uint64_t first = 0, uint64_t capacity = ~0ull) const
    {
        const std::vector<vrc_piece_moments> mo = moments(first, capacity);
        std::vector<HipMassProperties> out(mo.size());
        static const int pair[6][2] = {{0, 0}, {1, 1}, {2, 2}, {0, 1}, {0, 2}, {1, 2}};
        for (size_t i = 0; i < mo.size(); ++i) {
            const vrc_piece_moments& m = mo[i];
            if (!m.voxels) continue;
            const long double n = (long double)m.voxels;
            long double central[6];            // sum of r_a r_b about the centre of mass: (n s2_ab - s1_a s1_b) / (4n)
            for (int j = 0; j < 6; ++j) {
                const __int128 num = (__int128)m.voxels * (__int128)m.s2[j] - (__int128)m.s1[pair[j][0]] * (__int128)m.s1[pair[j][1]];
                central[j] = (long double)num / (4.0L * n);
            }
            HipMassProperties& o = out[i];
            o.mass = (double)n;
            for (int a = 0; a < 3; ++a) {
                o.centre[a] = (double)((long double)m.s1[a] / (2.0L * n));
                o.inertia[4 * a] = (double)(central[(a + 1) % 3] + central[(a + 2) % 3] + n / 6.0L);
            }
            o.inertia[1] = o.inertia[3] = (double)-central[3];
            o.inertia[2] = o.inertia[6] = (double)-central[4];
            o.inertia[5] = o.inertia[7] = (double)-central[5];
        }
        return out;
    }
    // The maps and boxes of placeAffine (vrc_affine_place_box of every piece's record box): every piece turned by `rot`
    // (vrc_make_rotation's layout) and resized by `scale` about src_pivots[3i..] -- its centre of mass with nullptr -- which
    // lands on dst_pivots[3i..], continuous voxel coordinates of a volume of dst_depth.  boxes gets count() x 6 numbers.
    std::vector<vrc_affine> poses(const float rot[9], const std::vector<float>& dst_pivots, uint32_t dst_depth, std::vector<uint32_t>& boxes,
                                  float scale = 1.0f, const std::vector<float>* src_pivots = nullptr) const
    {
        const size_t C = (size_t)count();
        if (dst_pivots.size() != 3 * C) throw std::invalid_argument("HipVoxelLabels::poses: dst_pivots must have three entries per component");
        if (src_pivots && src_pivots->size() != 3 * C) throw std::invalid_argument("HipVoxelLabels::poses: src_pivots must have three entries per component");
        const std::vector<vrc_component> records = components();
        std::vector<HipMassProperties> mass;
        if (!src_pivots) mass = massProperties();
        std::vector<vrc_affine> maps(C);
        boxes.assign(6 * C, 0u);
        for (size_t i = 0; i < C; ++i) {
            float pivot[3];
            for (int a = 0; a < 3; ++a) pivot[a] = src_pivots ? (*src_pivots)[3 * i + a] : (float)mass[i].centre[a];
            check(vrc_affine_place_box(rot, scale, pivot, &dst_pivots[3 * i], records[i].lo, records[i].hi, dst_depth, &maps[i], &boxes[6 * i], &boxes[6 * i + 3]),
                  "vrc_affine_place_box");
        }
        return maps;
    }
    // dst (any depth) gains (VRC_COPY_OR) or loses (VRC_COPY_ANDNOT) every piece with keep[id] != 0 (nullptr: all), each read
    // through its own inverse map inside its own box of dst (count() x 6, lo then hi; nullptr: all of dst) --
    // include/vrc.h: vrc_rigid_place_affine
    inline void placeAffine(const std::vector<vrc_affine>& maps, HipVoxelVolume& dst, int op = VRC_COPY_OR, const std::vector<uint32_t>* boxes = nullptr,
                            const std::vector<uint8_t>* keep = nullptr) const;
    // One record per piece: piece i read through its own inverse map inside its own box of `world` (count() x 6, lo then hi;
    // nullptr: all of world), as placeAffine would write it, against the solid voxels of world and its faces: the posed voxels,
    // those inside the solid (overlap) and those face to face with it (touch), each with the sum of c = 2p + 1 and of the voxel
    // normals -- include/vrc.h: vrc_rigid_contacts.  A piece with keep[id] == 0 (nullptr: all kept) has an all-zero record.
    // world is only read (its queued cells are flushed first) and nothing is excluded from it.
    inline std::vector<vrc_piece_contact> contacts(const std::vector<vrc_affine>& maps, HipVoxelVolume& world, const std::vector<uint32_t>* boxes = nullptr,
                                                   const std::vector<uint8_t>* keep = nullptr) const;
    // The broad phase of pairContacts (include/vrc.h: vrc_rigid_box_pairs): the ordered pairs (a, b), a != b, of kept pieces whose
    // boxes (count() x 6, lo then hi), clipped to a posed volume of posed_depth, meet when one is grown by a voxel; both orders,
    // ascending, two numbers a pair.
    inline std::vector<uint32_t> candidatePairs(const std::vector<uint32_t>& boxes, uint32_t posed_depth, const std::vector<uint8_t>* keep = nullptr) const;
    // One record per ordered pair (a, b) of `pairs` (two numbers a pair): piece a, posed as placeAffine would write it into a
    // volume of posed_depth, against piece b posed the same way -- no world, no walls -- include/vrc.h: vrc_rigid_pair_contacts.
    inline std::vector<vrc_piece_contact> pairContacts(const std::vector<vrc_affine>& maps, const std::vector<uint32_t>& pairs, uint32_t posed_depth,
                                                       const std::vector<uint32_t>* boxes = nullptr, const std::vector<uint8_t>* keep = nullptr) const;
    // One record per piece: `field` (Euclidean or travel, any depth) read at the voxels of piece i posed as contacts() poses it
    // into a volume of the field's depth -- their count, how many hold VRC_DISTANCE_NONE, the sum of the finite values, and the
    // least and greatest one with the voxel of smallest dense index that holds it -- include/vrc.h: vrc_rigid_clearance.  A
    // piece with keep[id] == 0 (nullptr: all kept) has the record of the empty set: min_value VRC_DISTANCE_NONE, the rest 0.
    inline std::vector<vrc_piece_clearance> clearance(const std::vector<vrc_affine>& maps, const HipVoxelDistance& field,
                                                      const std::vector<uint32_t>* boxes = nullptr, const std::vector<uint8_t>* keep = nullptr) const;
    vrc_labels* handle() const { return l_; }

private:
    friend class HipVoxelVolume;
    explicit HipVoxelLabels(vrc_labels* adopted) : l_(adopted) {}
    vrc_labels* l_ = nullptr;
};

// The squared Euclidean distance of every voxel to the feature set (include/vrc.h: vrc_volume_distance_field): a snapshot
// on the device, S^3 uint32 in [(x*S + y)*S + z] order, that later edits of the volume do not change.  Movable, RAII.
// HipVoxelVolume::travelField makes the same object with the steps from the seeds in place of the squared distance
// (vrc_travel_field): connectivity() is then 6 or 26, travelStats() holds what the call reported, tracePaths() reads routes.
// sight() walks straight segments over either kind and visibleFrom() makes the field of what an eye sees (vrc_sight_*).
class HipVoxelDistance {
public:
    ~HipVoxelDistance() { vrc_distance_destroy(d_); }
    HipVoxelDistance(HipVoxelDistance&& o) noexcept : d_(o.d_), stats_(o.stats_), travel_(o.travel_), sight_(o.sight_) { o.d_ = nullptr; }
    HipVoxelDistance& operator=(HipVoxelDistance&& o) noexcept
    {
        if (this != &o) { vrc_distance_destroy(d_); d_ = o.d_; stats_ = o.stats_; travel_ = o.travel_; sight_ = o.sight_; o.d_ = nullptr; }
        return *this;
    }
    HipVoxelDistance(const HipVoxelDistance&) = delete;
    HipVoxelDistance& operator=(const HipVoxelDistance&) = delete;

    const vrc_distance_stats& stats() const { return stats_; }
    const vrc_travel_stats& travelStats() const { return travel_; }      // of a travel field; zero for a Euclidean one
    const vrc_sight_stats& sightStats() const { return sight_; }         // of a sight field (visibleFrom); zero otherwise
    int connectivity() const { return vrc_travel_connectivity(d_); }   // 6 / 26: a travel field; 0: a Euclidean one
    uint32_t depth() const { return vrc_distance_depth(d_); }
    uint64_t bytes() const { return vrc_distance_bytes(d_); }
    const uint32_t* data() const { return vrc_distance_data(d_); }     // DEVICE pointer
    // the squared distance at each of n voxels (xyz: n x 3), VRC_DISTANCE_NONE outside the volume
    std::vector<uint32_t> at(const uint32_t* xyz, uint64_t n) const
    {
        std::vector<uint32_t> d2((size_t)n);
        check(vrc_distance_at(d_, n, xyz, d2.data(), VRC_MEM_HOST, nullptr), "vrc_distance_at");
        return d2;
    }
    std::vector<uint32_t> download() const
    {
        std::vector<uint32_t> d2((size_t)1 << (3u * depth()));
        check(vrc_distance_download(d_, d2.data()), "vrc_distance_download");
        return d2;
    }
    // dst becomes (VRC_COPY_REPLACE) / gains (_OR) / loses (_ANDNOT) the voxels with lo <= D <= hi
    inline void select(uint32_t lo, uint32_t hi, HipVoxelVolume& dst, int op = VRC_COPY_REPLACE) const;
    // Routes off a travel field (vrc_travel_trace_paths) from n start voxels (xyz: n x 3): lengths[i] = the field at start
    // i, and where that is finite the route's voxels 0 .. min(length, capacity - 1) at paths[(i*capacity + k)*3 ..]; rows
    // of starts without a value, and what lies behind a route's end, keep `fill`.
    void tracePaths(const uint32_t* xyz, uint64_t n, uint32_t capacity, std::vector<uint32_t>& paths, std::vector<uint32_t>& lengths,
                    uint32_t fill = VRC_DISTANCE_NONE) const
    {
        paths.assign((size_t)n * capacity * 3u, fill);
        lengths.assign((size_t)n, VRC_DISTANCE_NONE);
        check(vrc_travel_trace_paths(d_, n, xyz, capacity, capacity ? paths.data() : nullptr, lengths.data(), VRC_MEM_HOST, nullptr),
              "vrc_travel_trace_paths");
    }
    // Straight walks over the field (vrc_sight_segments) for n segments (n x 6: voxel a, voxel b): a record per segment --
    // VRC_SIGHT_CLEAR when every visited voxel has lo <= value <= hi, VRC_SIGHT_BLOCKED with the first that has not and the
    // voxel visited before it, VRC_SIGHT_OUTSIDE for an endpoint outside the volume.  flags: VRC_SIGHT_TOUCH for the
    // supercover, VRC_SIGHT_PLAIN to never stride.  lo = r * r + 1 on the field to the solid asks for a ball of radius r.
    std::vector<vrc_sight> sight(const int32_t* segments, uint64_t n, uint32_t lo = 1u, uint32_t hi = VRC_DISTANCE_NONE, int flags = VRC_SIGHT_THIN) const
    {
        std::vector<vrc_sight> out((size_t)n);
        check(vrc_sight_segments(d_, n, segments, lo, hi, flags, out.data(), VRC_MEM_HOST, nullptr), "vrc_sight_segments");
        return out;
    }
    // What an eye at voxel `eye` sees (vrc_sight_field): a new field holding |p - eye|^2 at every voxel p within `radius` (0:
    // no limit) whose walk from the eye is clear up to, not counting, p itself, VRC_DISTANCE_NONE elsewhere; sightStats()
    // holds what the call reported.  One walk per voxel in range.  Synchronous.
    HipVoxelDistance visibleFrom(const uint32_t eye[3], uint32_t radius = 0u, uint32_t lo = 1u, uint32_t hi = VRC_DISTANCE_NONE, int flags = VRC_SIGHT_THIN) const
    {
        vrc_distance* d = nullptr;
        vrc_sight_stats stats{};
        check(vrc_sight_field(d_, eye, radius, lo, hi, flags, &d, &stats), "vrc_sight_field");
        return HipVoxelDistance(d, stats);
    }
    vrc_distance* handle() const { return d_; }

private:
    friend class HipVoxelVolume;
    HipVoxelDistance(vrc_distance* adopted, const vrc_distance_stats& stats) : d_(adopted), stats_(stats) {}
    HipVoxelDistance(vrc_distance* adopted, const vrc_sight_stats& sight) : d_(adopted), sight_(sight) {}
    HipVoxelDistance(vrc_distance* adopted, const vrc_travel_stats& travel) : d_(adopted), travel_(travel) {}
    vrc_distance* d_ = nullptr;
    vrc_distance_stats stats_{};
    vrc_travel_stats travel_{};
    vrc_sight_stats sight_{};
};

// The difference of two volumes (include/vrc.h: vrc_delta_diff): a snapshot on the device, one record {word, bits} per
// occupancy word that differs, in ascending word order.  HipVoxelVolume::applyDelta flips the changed voxels, so one delta
// serves undo and redo.  Movable, RAII.
class HipVoxelDelta {
public:
    // from caller records (n x 2 uint32: word, bits; another rank's, a saved history's), held to the rule on the device
    static HipVoxelDelta fromRecords(uint32_t depth, const std::vector<uint32_t>& records, int device = 0)
    {
        if (records.size() & 1u) throw std::invalid_argument("HipVoxelDelta::fromRecords: records must have two entries per record");
        vrc_delta* d = nullptr;
        check(vrc_delta_create(depth, device, records.size() / 2, records.empty() ? nullptr : records.data(), VRC_MEM_HOST, &d, nullptr), "vrc_delta_create");
        return HipVoxelDelta(d);
    }
    ~HipVoxelDelta() { vrc_delta_destroy(d_); }
    HipVoxelDelta(HipVoxelDelta&& o) noexcept : d_(o.d_) { o.d_ = nullptr; }
    HipVoxelDelta& operator=(HipVoxelDelta&& o) noexcept
    {
        if (this != &o) { vrc_delta_destroy(d_); d_ = o.d_; o.d_ = nullptr; }
        return *this;
    }
    HipVoxelDelta(const HipVoxelDelta&) = delete;
    HipVoxelDelta& operator=(const HipVoxelDelta&) = delete;

    uint64_t count() const { return vrc_delta_count(d_); }
    uint32_t depth() const { return vrc_delta_depth(d_); }
    uint64_t bytes() const { return vrc_delta_bytes(d_); }
    // records, changed voxels and their box (hi exclusive); the host copy kept in the object
    vrc_delta_stats stats() const
    {
        vrc_delta_stats s{};
        check(vrc_delta_get_stats(d_, &s), "vrc_delta_get_stats");
        return s;
    }
    // the records [first, first + capacity) that exist: word, bits, word, bits, ...
    std::vector<uint32_t> records(uint64_t first = 0, uint64_t capacity = ~0ull) const
    {
        const uint64_t C = count(), n = first < C ? std::min(capacity, C - first) : 0;
        std::vector<uint32_t> out((size_t)n * 2u);
        if (n) check(vrc_delta_records(d_, first, n, out.data(), VRC_MEM_HOST, nullptr), "vrc_delta_records");
        return out;
    }
    vrc_delta* handle() const { return d_; }

private:
    friend class HipVoxelVolume;
    explicit HipVoxelDelta(vrc_delta* adopted) : d_(adopted) {}
    vrc_delta* d_ = nullptr;
};

// What SVO::setCell + compileSVO are to the reference (svo.hpp:72, lsvo_utils.cpp:4), on the device and repeatable: the
// occupancy of the S^3 volume stays resident, setCell() queues edits, commit() applies them and builds a NEW HipLSVO
// (bit-identical to compileSVO of the voxel set).  A scene in use is never touched: keep the old HipLSVO until the frames
// that walk it are done, then drop it.  Not re-entrant.  INTEGRATION.md section 2a.
class HipVoxelVolume {
public:
    explicit HipVoxelVolume(uint32_t depth, int device = 0) : device_(device) { check(vrc_volume_create(depth, device, &v_), "vrc_volume_create"); }
    // makes an existing scene (e.g. HipLSVO::fromFastNoiseTerrain) editable; takes over its albedo tables
    static std::unique_ptr<HipVoxelVolume> fromScene(const HipLSVO& svo)
    {
        vrc_volume* v = nullptr;
        check(vrc_volume_from_scene(svo.handle(), &v), "vrc_volume_from_scene");
        return std::unique_ptr<HipVoxelVolume>(new HipVoxelVolume(v, svo.device()));
    }
    ~HipVoxelVolume() { vrc_volume_destroy(v_); }
    HipVoxelVolume(const HipVoxelVolume&) = delete;
    HipVoxelVolume& operator=(const HipVoxelVolume&) = delete;

    // Volumetric::setCell (volumetric.hpp:59): Empty clears, every other type sets (the tree has one cell kind,
    // lsvo.hpp:21-23).  Queued on the host; flush() / commit() send the queue as batches.
    void setCell(Cell::Type type, Cell::Texture, uint32_t x, uint32_t y, uint32_t z)
    {
        const bool solid = type != Cell::Empty;
        if (!queue_.empty() && solid != queue_solid_) flush();   // a batch carries one value; order between values is kept
        queue_solid_ = solid;
        queue_.push_back(x); queue_.push_back(y); queue_.push_back(z);
    }
    // [lo, hi) per axis, clipped to the volume
    void fillBox(uint32_t x0, uint32_t y0, uint32_t z0, uint32_t x1, uint32_t y1, uint32_t z1, bool solid)
    {
        flush();
        const uint32_t box[6] = {x0, y0, z0, x1, y1, z1};
        check(vrc_volume_fill_boxes(v_, 1, box, solid ? 1 : 0, VRC_MEM_HOST, nullptr), "vrc_volume_fill_boxes");
    }
    void flush()
    {
        if (queue_.empty()) return;
        check(vrc_volume_set_voxels(v_, queue_.size() / 3, queue_.data(), queue_solid_ ? 1 : 0, VRC_MEM_HOST, nullptr), "vrc_volume_set_voxels");
        queue_.clear();
    }
    // Brushes, copies and queries (include/vrc.h).  Host-memory forms are synchronous; the *Device forms read device
    // memory in place and are asynchronous on `stream`.  Every one of them sends the setCell queue first.
    struct Sphere { int32_t x, y, z, radius; };
    void fillSpheres(const std::vector<Sphere>& spheres, bool solid)
    {
        flush();
        check(vrc_volume_fill_spheres(v_, spheres.size(), spheres.empty() ? nullptr : &spheres[0].x, solid ? 1 : 0, VRC_MEM_HOST, nullptr),
              "vrc_volume_fill_spheres");
    }
    void fillSpheresDevice(uint64_t n, const int32_t* centre_radius_dev, bool solid, void* stream = nullptr)
    {
        flush();
        check(vrc_volume_fill_spheres(v_, n, centre_radius_dev, solid ? 1 : 0, VRC_MEM_DEVICE, stream), "vrc_volume_fill_spheres");
    }
    // one sphere at every record: solid = false digs at the voxel hit, true builds at the empty cell in front of it
    void fillSpheresAtHits(const std::vector<vrc_hit>& hits, int32_t radius, bool solid)
    {
        flush();
        check(vrc_volume_fill_spheres_at_hits(v_, hits.size(), hits.data(), radius, solid ? 1 : 0, VRC_MEM_HOST, nullptr),
              "vrc_volume_fill_spheres_at_hits");
    }
    // the records vrc_cast_rays(..., VRC_MEM_DEVICE, stream) left on the device: same stream, no host copy of a hit
    void fillSpheresAtHitsDevice(uint64_t n, const vrc_hit* hits_dev, int32_t radius, bool solid, void* stream = nullptr)
    {
        flush();
        check(vrc_volume_fill_spheres_at_hits(v_, n, hits_dev, radius, solid ? 1 : 0, VRC_MEM_DEVICE, stream), "vrc_volume_fill_spheres_at_hits");
    }
    // Capsules (include/vrc.h: vrc_stroke_*): the voxels within `radius` of the segment a-b by the exact integer rule;
    // reserved stays 0
    struct Capsule { int32_t ax, ay, az, bx, by, bz, radius, reserved; };
    void fillCapsules(const std::vector<Capsule>& items, bool solid)
    {
        flush();
        check(vrc_stroke_fill_capsules(v_, items.size(), items.empty() ? nullptr : &items[0].ax, solid ? 1 : 0, VRC_MEM_HOST, nullptr),
              "vrc_stroke_fill_capsules");
    }
    void fillCapsulesDevice(uint64_t n, const int32_t* items_dev, bool solid, void* stream = nullptr)
    {
        flush();
        check(vrc_stroke_fill_capsules(v_, n, items_dev, solid ? 1 : 0, VRC_MEM_DEVICE, stream), "vrc_stroke_fill_capsules");
    }
    void fillLine(const int32_t a[3], const int32_t b[3], int32_t radius, bool solid)
    {
        const Capsule c = {a[0], a[1], a[2], b[0], b[1], b[2], radius, 0};
        fillCapsules(std::vector<Capsule>(1, c), solid);
    }
    // points: x y z per point; one capsule per pair of successive points (and from the last back to the first when closed) in
    // one call; a single point is its ball
    void fillPolyline(const std::vector<int32_t>& points, int32_t radius, bool solid, bool closed = false)
    {
        const size_t n = points.size() / 3;
        if (n == 0) return;
        const size_t links = n == 1 ? 1 : (closed ? n : n - 1);
        std::vector<Capsule> items(links);
        for (size_t i = 0; i < links; ++i) {
            const int32_t* a = &points[3 * i];
            const int32_t* b = &points[3 * ((i + 1) % n)];
            const Capsule c = {a[0], a[1], a[2], b[0], b[1], b[2], radius, 0};
            items[i] = c;
        }
        fillCapsules(items, solid);
    }
    // the gapless stroke through the records: the centres of fillSpheresAtHits, each joined to the next by a capsule; a record
    // without a centre breaks the stroke, and so does a step of more than max_gap voxels (0: no limit)
    void strokeAtHits(const std::vector<vrc_hit>& hits, int32_t radius, bool solid, uint32_t max_gap = 0)
    {
        flush();
        check(vrc_stroke_fill_at_hits(v_, hits.size(), hits.data(), radius, max_gap, solid ? 1 : 0, VRC_MEM_HOST, nullptr), "vrc_stroke_fill_at_hits");
    }
    void strokeAtHitsDevice(uint64_t n, const vrc_hit* hits_dev, int32_t radius, bool solid, uint32_t max_gap = 0, void* stream = nullptr)
    {
        flush();
        check(vrc_stroke_fill_at_hits(v_, n, hits_dev, radius, max_gap, solid ? 1 : 0, VRC_MEM_DEVICE, stream), "vrc_stroke_fill_at_hits");
    }
    // voxels src_lo + d of `src` -> dst_lo + d of this volume for 0 <= d < size, clipped to both; op = VRC_COPY_*
    void copyRegion(HipVoxelVolume& src, const uint32_t src_lo[3], const uint32_t size[3], const int32_t dst_lo[3],
                    int op = VRC_COPY_REPLACE, void* stream = nullptr)
    {
        flush();
        src.flush();
        check(vrc_volume_copy_region(v_, src.v_, src_lo, size, dst_lo, op, stream), "vrc_volume_copy_region");
    }
    // Stamps `src` into this volume through the inverse map (include/vrc.h: vrc_volume_stamp_affine): every voxel p of the
    // box [dst_lo, dst_hi) -- the whole volume with nullptr -- takes (op) the src voxel (m (2p + 1) + t) >> 17.
    void stampAffine(HipVoxelVolume& src, const vrc_affine& map, const uint32_t dst_lo[3] = nullptr, const uint32_t dst_hi[3] = nullptr,
                     int op = VRC_COPY_REPLACE, void* stream = nullptr)
    {
        flush();
        src.flush();
        const uint32_t S = 1u << depth();
        const uint32_t zero[3] = {0, 0, 0}, all[3] = {S, S, S};
        check(vrc_volume_stamp_affine(v_, src.v_, &map, dst_lo ? dst_lo : zero, dst_hi ? dst_hi : all, op, stream), "vrc_volume_stamp_affine");
    }
    // Places `src` turned by rot (vrc_make_rotation's layout) and resized by scale about the pivots (continuous voxel
    // coordinates; nullptr = the volume's centre): vrc_affine_place, then the stamp of the box it names.  Returns the map.
    vrc_affine stampPlaced(HipVoxelVolume& src, const float rot[9], float scale = 1.0f, const float src_pivot[3] = nullptr,
                           const float dst_pivot[3] = nullptr, int op = VRC_COPY_OR, void* stream = nullptr)
    {
        const float sc = (float)(1u << (src.depth() - 1u)), dc = (float)(1u << (depth() - 1u));
        const float src_centre[3] = {sc, sc, sc}, dst_centre[3] = {dc, dc, dc};
        vrc_affine map;
        uint32_t lo[3], hi[3];
        check(vrc_affine_place(rot, scale, src_pivot ? src_pivot : src_centre, dst_pivot ? dst_pivot : dst_centre, src.depth(), depth(), &map, lo, hi),
              "vrc_affine_place");
        stampAffine(src, map, lo, hi, op, stream);
        return map;
    }
    std::unique_ptr<HipVoxelVolume> clone()
    {
        flush();
        vrc_volume* v = nullptr;
        check(vrc_volume_clone(v_, &v), "vrc_volume_clone");
        return std::unique_ptr<HipVoxelVolume>(new HipVoxelVolume(v, device_));
    }
    // what changed from this volume to `after` (same depth and device); both are only read.  Synchronous.
    HipVoxelDelta diff(HipVoxelVolume& after)
    {
        flush();
        after.flush();
        vrc_delta* d = nullptr;
        check(vrc_delta_diff(v_, after.v_, &d, nullptr), "vrc_delta_diff");
        return HipVoxelDelta(d);
    }
    // word ^= bits for every record: on the `before` of a diff it gives `after`, on `after` it gives `before`
    void applyDelta(const HipVoxelDelta& delta, void* stream = nullptr)
    {
        flush();
        check(vrc_delta_apply(delta.handle(), v_, stream), "vrc_delta_apply");
    }
    // One step of the neighbour-count automaton (include/vrc.h: vrc_cells_step) from this volume into dst, which is written
    // whole: with c the solid ones among a voxel's 6 or 26 neighbours (those beyond the faces solid with `outside`), a
    // solid voxel stays if bit c of survive_mask is set and an empty one becomes solid if bit c of birth_mask is.
    // changed = nullptr: asynchronous on `stream`; else *changed = the voxels that differ, and the call is synchronous.
    void cellStep(HipVoxelVolume& dst, uint32_t birth_mask, uint32_t survive_mask, int neighbours = VRC_CELLS_ALL, bool outside = false,
                  uint64_t* changed = nullptr, void* stream = nullptr)
    {
        flush();
        dst.flush();
        check(vrc_cells_step(dst.v_, v_, neighbours, birth_mask, survive_mask, outside ? 1 : 0, changed, VRC_MEM_HOST, stream), "vrc_cells_step");
    }
    // Up to `steps` steps in place, ping-pong with one scratch volume; ends early at a step that changes nothing.  Returns
    // the number of steps that changed a voxel.
    uint32_t automaton(uint32_t steps, uint32_t birth_mask, uint32_t survive_mask, int neighbours = VRC_CELLS_ALL, bool outside = false)
    {
        if (!steps) return 0;
        HipVoxelVolume scratch(depth(), device_);
        HipVoxelVolume *src = this, *dst = &scratch;
        uint32_t taken = 0;
        while (taken < steps) {
            uint64_t changed = 0;
            src->cellStep(*dst, birth_mask, survive_mask, neighbours, outside, &changed);
            if (!changed) break;                 // dst equals src
            std::swap(src, dst);
            ++taken;
        }
        if (src != this) {
            const uint32_t S = 1u << depth();
            const uint32_t zero[3] = {0, 0, 0}, all[3] = {S, S, S};
            const int32_t at[3] = {0, 0, 0};
            copyRegion(scratch, zero, all, at);  // the scratch volume's destructor waits for it
        }
        return taken;
    }
    // the majority of the 27 cells around every voxel, itself included, `iterations` times in place
    void smooth(uint32_t iterations = 1, bool outside = false) { automaton(iterations, 0x7FFC000u, 0x7FFE000u, VRC_CELLS_ALL, outside); }
    // clears the solid voxels without a solid face neighbour
    void removeSpecks() { automaton(1, 0u, 0x7Eu, VRC_CELLS_FACES, false); }
    // A seeded random voxel set R, the hash of (seed, x, y, z) below round(density 2^32) (include/vrc.h:
    // vrc_cells_fill_random): inside box (lo x y z, hi x y z exclusive; nullptr = the whole volume) this volume takes (op) R.
    void fillRandom(uint32_t seed, double density, const uint32_t box[6] = nullptr, int op = VRC_COPY_OR, void* stream = nullptr)
    {
        flush();
        if (!(density >= 0.0 && density <= 1.0)) throw std::invalid_argument("HipVoxelVolume::fillRandom: density not in [0, 1]");
        check(vrc_cells_fill_random(v_, seed, (uint64_t)std::llround(density * 4294967296.0), box, op, stream), "vrc_cells_fill_random");
    }
    // caves from a seed: the fill of the whole volume, then `steps` rounds of smooth with everything beyond the faces solid
    void caves(uint32_t seed, double density, uint32_t steps)
    {
        fillRandom(seed, density, nullptr, VRC_COPY_REPLACE);
        smooth(steps, true);
    }
    // Along an axis (include/vrc.h: vrc_columns_*).  direction = 2 * axis + side, side 0 travels towards smaller coordinates;
    // rect = (u_lo, v_lo, u_hi, v_hi) over the other two axes in x < y < z order, nullptr = the whole face; maps are dense
    // U x V arrays, column (u, v) at (u - u_lo) * V + (v - v_lo).
    // what every column of the rect holds: first / last solid voxel met, solid voxels, runs.  Synchronous.
    std::vector<vrc_column> columnProfile(int direction, const uint32_t rect[4] = nullptr)
    {
        flush();
        const uint32_t S = 1u << depth();
        const uint64_t U = rect ? (rect[2] > rect[0] ? rect[2] - rect[0] : 0u) : S, V = rect ? (rect[3] > rect[1] ? rect[3] - rect[1] : 0u) : S;
        std::vector<vrc_column> out(std::max<uint64_t>(U * V, 1u));          // an empty rect is refused by the library, by its text
        check(vrc_columns_profile(v_, direction, rect, out.data(), VRC_MEM_HOST, nullptr), "vrc_columns_profile");
        return out;
    }
    // the coordinate of the first solid voxel met in every column of the whole face, `none` in an empty one
    std::vector<int32_t> heightMap(int direction, int32_t none = -1)
    {
        const std::vector<vrc_column> p = columnProfile(direction);
        std::vector<int32_t> out(p.size());
        for (size_t i = 0; i < p.size(); ++i) out[i] = p[i].count ? (int32_t)p[i].first : none;
        return out;
    }
    // the solid voxels of every column along `axis`: the X-ray image
    std::vector<uint32_t> thicknessMap(int axis)
    {
        const std::vector<vrc_column> p = columnProfile(2 * axis);
        std::vector<uint32_t> out(p.size());
        for (size_t i = 0; i < p.size(); ++i) out[i] = p[i].count;
        return out;
    }
    // no column has a second run met along `direction`; grounded: and every run reaches the exit face
    bool isHeightField(int direction, bool grounded = false)
    {
        const uint32_t exit_at = (direction & 1) ? (1u << depth()) - 1u : 0u;
        for (const vrc_column& c : columnProfile(direction))
            if (c.runs > 1u || (grounded && c.runs == 1u && c.last != exit_at)) return false;
        return true;
    }
    // every column of the rect takes (op) its span [lo, hi) along `axis`: lo from lo_map (nullptr: lo_const), hi likewise,
    // clamped to [0, S]; under VRC_COPY_REPLACE the rest of the column is cleared.  Synchronous.
    void fillColumns(int axis, const int32_t* lo_map, int32_t lo_const, const int32_t* hi_map, int32_t hi_const, const uint32_t rect[4] = nullptr,
                     int op = VRC_COPY_OR)
    {
        flush();
        check(vrc_columns_fill(v_, axis, rect, lo_map, lo_const, hi_map, hi_const, op, VRC_MEM_HOST, nullptr), "vrc_columns_fill");
    }
    // the same with the maps in device memory, asynchronous on `stream`
    void fillColumnsDevice(int axis, const int32_t* lo_map_dev, int32_t lo_const, const int32_t* hi_map_dev, int32_t hi_const,
                           const uint32_t rect[4] = nullptr, int op = VRC_COPY_OR, void* stream = nullptr)
    {
        flush();
        check(vrc_columns_fill(v_, axis, rect, lo_map_dev, lo_const, hi_map_dev, hi_const, op, VRC_MEM_DEVICE, stream), "vrc_columns_fill");
    }
    // main.cpp:65-72 as an editable volume: column (x, z) solid for S/2 + 1 <= y < S/2 + clamp(heights[x * S + z], 16, S), the
    // rest cleared.  heights: S x S.
    void raiseTerrain(const std::vector<int32_t>& heights)
    {
        const int32_t S = (int32_t)(1u << depth());
        if (heights.size() != (size_t)S * (size_t)S) throw std::invalid_argument("HipVoxelVolume::raiseTerrain: heights are not S x S");
        std::vector<int32_t> hi(heights.size());
        for (size_t i = 0; i < hi.size(); ++i) hi[i] = S / 2 + std::max(16, std::min(S, heights[i]));
        fillColumns(1, nullptr, S / 2 + 1, hi.data(), 0, nullptr, VRC_COPY_REPLACE);
    }
    // dst takes (op) the voxels with lo <= P < hi, P the solid voxels met before the voxel along `direction`, that are solid
    // (VRC_COLUMNS_SOLID), empty (VRC_COLUMNS_EMPTY) or either (both bits).  This volume is only read.  Asynchronous on `stream`.
    void selectColumns(HipVoxelVolume& dst, int direction, uint32_t lo, uint32_t hi, int of, int op = VRC_COPY_REPLACE, void* stream = nullptr)
    {
        flush();
        dst.flush();
        check(vrc_columns_select(dst.v_, v_, direction, lo, hi, of, op, stream), "vrc_columns_select");
    }
    // the solid voxels a parallel light along `direction` reaches; the first k solid voxels of every column; the empty
    // voxels behind a solid one.  Each replaces what dst held.
    void skyLit(HipVoxelVolume& dst, int direction) { selectColumns(dst, direction, 0u, 1u, VRC_COLUMNS_SOLID); }
    void topLayers(HipVoxelVolume& dst, int direction, uint32_t k) { selectColumns(dst, direction, 0u, k, VRC_COLUMNS_SOLID); }
    void sheltered(HipVoxelVolume& dst, int direction) { selectColumns(dst, direction, 1u, (1u << depth()) + 1u, VRC_COLUMNS_EMPTY); }
    // Morphology by a structuring element (include/vrc.h: vrc_morph_apply).  An element is x y z per offset, every component
    // within +-VRC_MORPH_REACH.
    typedef std::vector<int32_t> Element;
    // the offsets with d^2 <= r^2: the ball of dilate(r)
    static Element elementBall(int32_t r)
    {
        Element e;
        for (int32_t x = -r; x <= r; ++x)
            for (int32_t y = -r; y <= r; ++y)
                for (int32_t z = -r; z <= r; ++z)
                    if (x * x + y * y + z * z <= r * r) { e.push_back(x); e.push_back(y); e.push_back(z); }
        return e;
    }
    // the a x b x c box whose voxel `anchor` is the pivot (nullptr: a / 2, b / 2, c / 2)
    static Element elementBox(int32_t a, int32_t b, int32_t c, const int32_t anchor[3] = nullptr)
    {
        const int32_t at[3] = {anchor ? anchor[0] : a / 2, anchor ? anchor[1] : b / 2, anchor ? anchor[2] : c / 2};
        Element e;
        for (int32_t x = 0; x < a; ++x)
            for (int32_t y = 0; y < b; ++y)
                for (int32_t z = 0; z < c; ++z) { e.push_back(x - at[0]); e.push_back(y - at[1]); e.push_back(z - at[2]); }
        return e;
    }
    // the pivot and its six face neighbours
    static Element elementCross()
    {
        const int32_t o[21] = {0, 0, 0, -1, 0, 0, 1, 0, 0, 0, -1, 0, 0, 1, 0, 0, 0, -1, 0, 0, 1};
        return Element(o, o + 21);
    }
    // the offsets lo .. hi (both included) along `axis`
    static Element elementLine(int axis, int32_t lo, int32_t hi)
    {
        Element e;
        for (int32_t t = lo; t <= hi; ++t)
            for (int a = 0; a < 3; ++a) e.push_back(a == axis ? t : 0);
        return e;
    }
    static Element reflect(const Element& element)
    {
        Element e(element);
        for (size_t i = 0; i < e.size(); ++i) e[i] = -e[i];
        return e;
    }
    // dst takes (op) K = A (+) E (what = VRC_MORPH_DILATE) or A (-) E (VRC_MORPH_ERODE), A the solid voxels of this volume
    // (its empty ones with of_empty) and, with `outside`, everything beyond the faces.  This volume is only read.  Synchronous.
    void morph(HipVoxelVolume& dst, int what, const Element& element, bool of_empty = false, bool outside = false, int op = VRC_COPY_REPLACE,
               const int32_t origin[3] = nullptr)
    {
        flush();
        dst.flush();
        check(vrc_morph_apply(dst.v_, v_, what, of_empty ? VRC_MORPH_EMPTY : VRC_MORPH_SOLID, element.size() / 3, element.data(), origin, outside ? 1 : 0, op,
                              VRC_MEM_HOST, nullptr),
              "vrc_morph_apply");
    }
    // the same with n offsets in device memory (a list of vrc_voxels_extract as it is, origin its pivot), asynchronous on `stream`
    void morphDevice(HipVoxelVolume& dst, int what, uint64_t n, const int32_t* offsets_dev, const int32_t origin[3] = nullptr, bool of_empty = false,
                     bool outside = false, int op = VRC_COPY_REPLACE, void* stream = nullptr)
    {
        flush();
        dst.flush();
        check(vrc_morph_apply(dst.v_, v_, what, of_empty ? VRC_MORPH_EMPTY : VRC_MORPH_SOLID, n, offsets_dev, origin, outside ? 1 : 0, op, VRC_MEM_DEVICE, stream),
              "vrc_morph_apply");
    }
    void morphInPlace(int what, const Element& element, bool outside)
    {
        HipVoxelVolume scratch(depth(), device_);
        morph(scratch, what, element, false, outside);
        const uint32_t S = 1u << depth();
        const uint32_t zero[3] = {0, 0, 0}, all[3] = {S, S, S};
        const int32_t at[3] = {0, 0, 0};
        copyRegion(scratch, zero, all, at);      // the scratch volume's destructor waits for it
    }
    // In place through a scratch volume.  Minkowski sums compose: a box is three lines in a row, a + b + c offsets for a b c.
    void dilateBy(const Element& element) { morphInPlace(VRC_MORPH_DILATE, element, false); }
    // open_border: everything beyond the faces counts as empty, so the erosion eats from the faces as well
    void erodeBy(const Element& element, bool open_border = false) { morphInPlace(VRC_MORPH_ERODE, element, !open_border); }
    void openBy(const Element& element) { erodeBy(element); dilateBy(element); }
    void closeBy(const Element& element) { dilateBy(element); erodeBy(element); }
    // dst becomes the pivots at which the shape stands free of the solid voxels and inside the volume
    void fitsAt(HipVoxelVolume& dst, const Element& element) { morph(dst, VRC_MORPH_ERODE, element, true, false); }
    // hit-or-miss: dst becomes the p with p + s solid for every s of solid_offsets and p + t empty for every t of empty_offsets
    void match(HipVoxelVolume& dst, const Element& solid_offsets, const Element& empty_offsets, bool outside = false)
    {
        morph(dst, VRC_MORPH_ERODE, solid_offsets, false, outside);
        morph(dst, VRC_MORPH_DILATE, reflect(empty_offsets), false, outside, VRC_COPY_ANDNOT);
    }
    // Between depths (include/vrc.h: vrc_levels_*).  A cell of level k is the cube of 2^k voxels per axis at a multiple of 2^k.
    // the density grid: the solid voxels of every cell of level k, 1 <= k <= depth, (S >> k)^3 counts with cell (X, Y, Z) at
    // (X * Sc + Y) * Sc + Z.  Synchronous.
    std::vector<uint32_t> cellCounts(uint32_t k)
    {
        flush();
        const uint32_t d = depth();
        std::vector<uint32_t> out((size_t)1u << (3u * (k <= d ? d - k : 0u)));          // a k beyond the depth is refused by the library, by its text
        check(vrc_levels_counts(v_, k, out.data(), VRC_MEM_HOST, nullptr), "vrc_levels_counts");
        return out;
    }
    // the band [lo, hi) of counts that a rule keeps at level k: at least one voxel of the cell, every one, at least half
    enum class LevelRule { Any, All, Majority };
    static void countRange(LevelRule rule, uint32_t k, uint32_t* lo, uint32_t* hi)
    {
        const uint32_t full = 1u << (3u * k);
        *lo = rule == LevelRule::Any ? 1u : rule == LevelRule::All ? full : full / 2u;
        *hi = full + 1u;
    }
    // dst, of a smaller depth, takes (op) the voxels whose cell of this volume holds lo <= count < hi solid voxels.  This
    // volume is only read.  Asynchronous on `stream`.
    void reduceInto(HipVoxelVolume& dst, uint32_t lo, uint32_t hi, int op = VRC_COPY_REPLACE, void* stream = nullptr)
    {
        flush();
        dst.flush();
        check(vrc_levels_reduce(dst.v_, v_, lo, hi, op, stream), "vrc_levels_reduce");
    }
    // a new volume of the smaller `depth` reduced by the rule
    std::unique_ptr<HipVoxelVolume> reduced(uint32_t depth, LevelRule rule = LevelRule::Any)
    {
        std::unique_ptr<HipVoxelVolume> out(new HipVoxelVolume(depth, device_));
        uint32_t lo = 0, hi = 0;
        countRange(rule, this->depth() > depth ? this->depth() - depth : 0u, &lo, &hi);
        reduceInto(*out, lo, hi);
        return out;
    }
    // dst, of a greater depth, takes (op) this volume with every voxel repeated 2^k times per axis.  Asynchronous on `stream`.
    void expandInto(HipVoxelVolume& dst, int op = VRC_COPY_REPLACE, void* stream = nullptr)
    {
        flush();
        dst.flush();
        check(vrc_levels_expand(dst.v_, v_, op, stream), "vrc_levels_expand");
    }
    std::unique_ptr<HipVoxelVolume> expanded(uint32_t depth)
    {
        std::unique_ptr<HipVoxelVolume> out(new HipVoxelVolume(depth, device_));
        expandInto(*out);
        return out;
    }
    // xyz: n x 3 coordinates -> 0 / 1 each (0 outside the volume)
    std::vector<uint8_t> getVoxels(const std::vector<uint32_t>& xyz)
    {
        flush();
        std::vector<uint8_t> out(xyz.size() / 3);
        check(vrc_volume_get_voxels(v_, out.size(), xyz.data(), out.data(), VRC_MEM_HOST, nullptr), "vrc_volume_get_voxels");
        return out;
    }
    // lo_hi: n x 6 as for fillBox -> solid voxels per box
    std::vector<uint64_t> countBoxes(const std::vector<uint32_t>& lo_hi)
    {
        flush();
        std::vector<uint64_t> out(lo_hi.size() / 6);
        check(vrc_volume_count_boxes(v_, out.size(), lo_hi.data(), out.data(), VRC_MEM_HOST, nullptr), "vrc_volume_count_boxes");
        return out;
    }
    // Flood fill by connectivity (include/vrc.h: vrc_volume_flood): this volume's solid voxels are the seeds; afterwards it
    // holds exactly the voxels of `medium` (its solid ones, or its empty ones with through_empty) joined to a seed by face
    // neighbours (6) or face / edge / corner neighbours (26).  max_sweeps = 0 runs to convergence; a capped call may return
    // converged == 0 with a valid partial result, and calling again continues.  Synchronous.
    vrc_flood_stats flood(HipVoxelVolume& medium, int connectivity = VRC_CONNECT_FACES, bool through_empty = false, uint32_t max_sweeps = 0)
    {
        flush();
        medium.flush();
        vrc_flood_stats st;
        check(vrc_volume_flood(v_, medium.v_, connectivity, through_empty ? VRC_FLOOD_EMPTY : VRC_FLOOD_SOLID, max_sweeps, &st), "vrc_volume_flood");
        return st;
    }
    // Drops what no longer holds on to the anchors (lo_hi: n x 6 as for fillBox): afterwards this volume holds only the solid
    // voxels joined to a solid voxel inside an anchor box, and the rest -- the debris -- is returned as a new volume.
    std::unique_ptr<HipVoxelVolume> keepConnected(const std::vector<uint32_t>& anchor_lo_hi, int connectivity = VRC_CONNECT_FACES)
    {
        flush();
        const uint32_t d = depth(), S = 1u << d;
        const uint32_t zero[3] = {0, 0, 0}, all[3] = {S, S, S};
        const int32_t at[3] = {0, 0, 0};
        HipVoxelVolume supported(d, device_);
        if (!anchor_lo_hi.empty())
            check(vrc_volume_fill_boxes(supported.v_, anchor_lo_hi.size() / 6, anchor_lo_hi.data(), 1, VRC_MEM_HOST, nullptr), "vrc_volume_fill_boxes");
        supported.flood(*this, connectivity);
        std::unique_ptr<HipVoxelVolume> debris = clone();
        debris->copyRegion(supported, zero, all, at, VRC_COPY_ANDNOT);
        copyRegion(supported, zero, all, at, VRC_COPY_REPLACE);
        return debris;       // `supported` is destroyed behind the copies: vrc_volume_destroy waits for the device
    }
    // Every connected piece of the solid voxels (of the empty ones with through_empty) named in one call.  Synchronous.
    HipVoxelLabels labelComponents(int connectivity = VRC_CONNECT_FACES, bool through_empty = false)
    {
        flush();
        vrc_labels* l = nullptr;
        check(vrc_volume_label_components(v_, connectivity, through_empty ? VRC_FLOOD_EMPTY : VRC_FLOOD_SOLID, &l, nullptr), "vrc_volume_label_components");
        return HipVoxelLabels(l);
    }
    // Voronoi fracture (include/vrc.h: vrc_fracture_label): the pieces of the solid voxels (the empty ones with through_empty)
    // cut along the Voronoi cells of the sites (x y z int32 each); voxels farther than max_distance from every site (d^2 > r^2;
    // negative: no limit) keep the cell "none" and stay whole.  Nothing is removed.  Synchronous.
    HipVoxelLabels fracture(const std::vector<int32_t>& sites_xyz, int connectivity = VRC_CONNECT_FACES, bool through_empty = false, int64_t max_distance = -1)
    {
        flush();
        vrc_labels* l = nullptr;
        const uint64_t r = (uint64_t)std::min<int64_t>(max_distance, 65535);       // finite distances are below 2^22
        const uint32_t max_d2 = max_distance < 0 ? VRC_DISTANCE_NONE : (uint32_t)(r * r);
        check(vrc_fracture_label(v_, connectivity, through_empty ? VRC_FLOOD_EMPTY : VRC_FLOOD_SOLID, sites_xyz.size() / 3, sites_xyz.data(), max_d2,
                                 VRC_MEM_HOST, &l, nullptr),
              "vrc_fracture_label");
        return HipVoxelLabels(l);
    }
    // Dig, let the debris fall, commit: what no longer holds on to a solid voxel inside one of the n anchor boxes falls piece
    // by piece along `direction` (a VRC_FACE_* code) until it lands, at most drop_limit cells (0 = no limit); afterwards the
    // volume holds the supported part plus every loose piece where it came to rest.
    vrc_fall_stats dropLoose(const uint32_t* anchor_lo_hi, size_t n, int direction, int connectivity = VRC_CONNECT_FACES, uint32_t drop_limit = 0)
    {
        std::unique_ptr<HipVoxelVolume> debris = keepConnected(std::vector<uint32_t>(anchor_lo_hi, anchor_lo_hi + 6 * n), connectivity);
        HipVoxelLabels labels = debris->labelComponents(connectivity);
        vrc_fall_stats stats;
        const std::vector<int32_t> offsets = labels.fall(this, direction, drop_limit, &stats);
        labels.place(offsets, *this, VRC_COPY_OR);
        return stats;
    }
    // Clears every solid piece of fewer than min_voxels voxels; returns how many pieces that were.
    uint64_t removeSmallPieces(uint64_t min_voxels, int connectivity = VRC_CONNECT_FACES)
    {
        HipVoxelLabels labels = labelComponents(connectivity);
        const std::vector<vrc_component> records = labels.components();
        std::vector<uint8_t> small(records.size());
        uint64_t removed = 0;
        for (size_t i = 0; i < records.size(); ++i) removed += small[i] = records[i].voxels < min_voxels ? 1 : 0;
        if (removed) labels.select(small, *this, VRC_COPY_ANDNOT);
        return removed;
    }
    // The least number of steps from the solid voxels of `seeds` to every voxel through this volume's solid voxels (its
    // empty ones with through_empty), VRC_DISTANCE_NONE where nothing arrives or, with step_limit, beyond it
    // (include/vrc.h: vrc_travel_field).  `seeds` may be this volume.  Synchronous.
    HipVoxelDistance travelField(HipVoxelVolume& seeds, int connectivity = VRC_CONNECT_FACES, bool through_empty = false, uint32_t step_limit = 0)
    {
        flush();
        seeds.flush();
        vrc_distance* d = nullptr;
        vrc_travel_stats stats{};
        check(vrc_travel_field(seeds.v_, v_, connectivity, through_empty ? VRC_FLOOD_EMPTY : VRC_FLOOD_SOLID, step_limit, &d, &stats),
              "vrc_travel_field");
        return HipVoxelDistance(d, stats);
    }
    // The exact squared Euclidean distance of every voxel to the nearest solid voxel (to the nearest empty one with
    // to_empty; with outside, everything beyond the faces is a feature as well).  Synchronous.
    HipVoxelDistance distanceField(bool to_empty = false, bool outside = false)
    {
        flush();
        vrc_distance* d = nullptr;
        vrc_distance_stats stats{};
        check(vrc_volume_distance_field(v_, to_empty ? VRC_FLOOD_EMPTY : VRC_FLOOD_SOLID, outside ? 1 : 0, &d, &stats), "vrc_volume_distance_field");
        return HipVoxelDistance(d, stats);
    }
    // Grow / shrink by r voxels, with the rule of fillSphere (d^2 <= r^2); open_border: beyond the faces counts as empty.
    void dilate(uint32_t r)
    {
        r = std::min(r, 65535u);
        distanceField().select(0u, r * r, *this, VRC_COPY_OR);
    }
    void erode(uint32_t r, bool open_border = false)
    {
        r = std::min(r, 65535u);
        distanceField(true, open_border).select(0u, r * r, *this, VRC_COPY_ANDNOT);
    }
    // Clears the solid voxels farther than t from the empty ones: a shell t voxels thick is left.
    void hollow(uint32_t t)
    {
        t = std::min(t, 65535u);
        distanceField(true).select(t * t + 1u, VRC_DISTANCE_NONE, *this, VRC_COPY_ANDNOT);
    }
    // Solid voxelisation by crossing parity (include/vrc.h: vrc_volume_xor_mesh): n x 9 int32 triangles in setCell
    // coordinates with VRC_MESH_FRAC_BITS fractional bits; every voxel whose centre lies under an odd number of them is
    // flipped, so a closed mesh in an empty volume gives its inside.  Synchronous.
    void xorMesh(const std::vector<int32_t>& tris_fixed)
    {
        flush();
        check(vrc_volume_xor_mesh(v_, tris_fixed.size() / 9, tris_fixed.data(), VRC_MEM_HOST, nullptr), "vrc_volume_xor_mesh");
    }
    void xorMeshDevice(uint64_t n, const int32_t* tris_dev, void* stream = nullptr)
    {
        flush();
        check(vrc_volume_xor_mesh(v_, n, tris_dev, VRC_MEM_DEVICE, stream), "vrc_volume_xor_mesh");
    }
    // n x 3 vertices in voxels -> fixed point, llrint((v * scale + offset) * 64), each VERTEX once: a vertex shared by
    // several faces stays one point, so a closed mesh stays closed
    static std::vector<int64_t> quantiseMesh(const std::vector<double>& verts, double scale = 1.0, double ox = 0.0, double oy = 0.0, double oz = 0.0)
    {
        const double off[3] = {ox, oy, oz}, unit = (double)(1 << VRC_MESH_FRAC_BITS);
        std::vector<int64_t> fixed(verts.size());
        for (size_t i = 0; i < verts.size(); ++i) {
            const double q = std::nearbyint((verts[i] * scale + off[i % 3]) * unit);
            if (!(std::fabs(q) <= 131072.0)) throw std::invalid_argument("quantiseMesh: a vertex lies beyond +-2048 voxels");
            fixed[i] = (int64_t)std::llrint(q);
        }
        return fixed;
    }
    // XORs the solid of the indexed mesh (verts n x 3 in voxels, faces m x 3 indices) into the volume
    void voxelizeMesh(const std::vector<double>& verts, const std::vector<uint32_t>& faces, double scale = 1.0,
                      double ox = 0.0, double oy = 0.0, double oz = 0.0)
    {
        const int64_t zero[3] = {0, 0, 0};
        xorMesh(meshSoup(quantiseMesh(verts, scale, ox, oy, oz), faces, zero));
    }
    // Surface voxelisation (include/vrc.h: vrc_raster_mesh): n x 9 int32 triangles in xorMesh's fixed point.  mode
    // VRC_RASTER_TOUCHED selects every voxel whose closed cube meets a triangle, VRC_RASTER_THIN the voxel that holds each
    // crossing of a voxel-centre line; the selected voxels are all set or all cleared.  Synchronous.
    void rasterMesh(const std::vector<int32_t>& tris_fixed, int mode = VRC_RASTER_TOUCHED, bool solid = true)
    {
        flush();
        check(vrc_raster_mesh(v_, tris_fixed.size() / 9, tris_fixed.data(), mode, solid ? 1 : 0, VRC_MEM_HOST, nullptr), "vrc_raster_mesh");
    }
    void rasterMeshDevice(uint64_t n, const int32_t* tris_dev, int mode = VRC_RASTER_TOUCHED, bool solid = true, void* stream = nullptr)
    {
        flush();
        check(vrc_raster_mesh(v_, n, tris_dev, mode, solid ? 1 : 0, VRC_MEM_DEVICE, stream), "vrc_raster_mesh");
    }
    // Sets (or clears) the voxels the indexed mesh touches, or with thin its thin shell; the mesh need not be closed
    void shellMesh(const std::vector<double>& verts, const std::vector<uint32_t>& faces, bool thin = false, bool solid = true, double scale = 1.0,
                   double ox = 0.0, double oy = 0.0, double oz = 0.0)
    {
        const int64_t zero[3] = {0, 0, 0};
        rasterMesh(meshSoup(quantiseMesh(verts, scale, ox, oy, oz), faces, zero), thin ? VRC_RASTER_THIN : VRC_RASTER_TOUCHED, solid);
    }
    // What an editor does with a model: voxelises it into a clipboard volume of the smallest depth that holds its bounding
    // box and copies that box into this volume with op (VRC_COPY_OR pastes, _ANDNOT carves, _REPLACE overwrites the box)
    void stampMesh(const std::vector<double>& verts, const std::vector<uint32_t>& faces, int op = VRC_COPY_OR, double scale = 1.0,
                   double ox = 0.0, double oy = 0.0, double oz = 0.0)
    {
        flush();
        const std::vector<int64_t> fixed = quantiseMesh(verts, scale, ox, oy, oz);
        if (fixed.size() < 3) return;
        int64_t lo[3], hi[3];
        for (int a = 0; a < 3; ++a) lo[a] = hi[a] = fixed[a];
        for (size_t i = 0; i < fixed.size(); ++i) {
            if (fixed[i] < lo[i % 3]) lo[i % 3] = fixed[i];
            if (fixed[i] > hi[i % 3]) hi[i % 3] = fixed[i];
        }
        uint32_t size[3], largest = 1;
        int32_t at[3];
        int64_t origin[3];
        for (int a = 0; a < 3; ++a) {
            const int64_t l = lo[a] >> VRC_MESH_FRAC_BITS, h = -((-hi[a]) >> VRC_MESH_FRAC_BITS);   // floor, ceil
            size[a] = (uint32_t)(h - l > 1 ? h - l : 1);
            if (size[a] > largest) largest = size[a];
            at[a] = (int32_t)l;
            origin[a] = l * (1 << VRC_MESH_FRAC_BITS);
        }
        uint32_t d = 2;
        while ((1u << d) < largest) ++d;
        if (d > 10) throw std::invalid_argument("stampMesh: the mesh's bounding box exceeds 1024 voxels");
        HipVoxelVolume clip(d, device_);
        clip.xorMesh(meshSoup(fixed, faces, origin));       // whole voxels: the same triangles, moved
        const uint32_t zero[3] = {0, 0, 0};
        copyRegion(clip, zero, size, at, op);               // `clip` is destroyed behind the copy: vrc_volume_destroy waits
    }
    // Getting the world out (include/vrc.h: vrc_volume_extract_surface): the exposed faces of the voxel set in their
    // canonical order.  closed: the volume's own faces count as exposed, the mesh is closed and xorMesh of its triangles
    // into an empty volume gives the voxel set back.  counts[d], d = VRC_FACE_*: faces per direction.
    std::vector<uint64_t> surfaceCount(bool closed = true)
    {
        flush();
        std::vector<uint64_t> counts(6);
        check(vrc_volume_surface_count(v_, closed ? 1 : 0, counts.data()), "vrc_volume_surface_count");
        return counts;
    }
    // n x 4: x y z d of every exposed face (first / capacity: a window of the canonical order, in faces)
    std::vector<uint32_t> surfaceFaces(bool closed = true, uint64_t first = 0, uint64_t capacity = ~0ull)
    {
        return extractSurface<uint32_t>(VRC_SURFACE_FACES, 4, closed, first, capacity);
    }
    // 2n x 9: two triangles per face in xorMesh's fixed point, wound outwards
    std::vector<int32_t> surfaceTriangles(bool closed = true, uint64_t first = 0, uint64_t capacity = ~0ull)
    {
        return extractSurface<int32_t>(VRC_SURFACE_TRIANGLES, 18, closed, first, capacity);
    }
    // the same into device memory, asynchronous on `stream`; total_dev (may be null): a device uint64_t that receives the
    // number of faces in stream order
    void extractSurfaceDevice(int format, uint64_t first, uint64_t capacity, void* out_dev, uint64_t* total_dev, bool closed = true,
                              void* stream = nullptr)
    {
        flush();
        check(vrc_volume_extract_surface(v_, closed ? 1 : 0, format, first, capacity, out_dev, total_dev, VRC_MEM_DEVICE, stream),
              "vrc_volume_extract_surface");
    }
    // The same surface with coplanar faces merged into rectangles (include/vrc.h: vrc_extract_rects), in the order
    // (d, c_a, s0, r0).  counts[d]: rectangles per direction.
    std::vector<uint64_t> rectCount(bool closed = true)
    {
        flush();
        std::vector<uint64_t> counts(6);
        check(vrc_rect_count(v_, closed ? 1 : 0, counts.data()), "vrc_rect_count");
        return counts;
    }
    // n x 4: x y z of the rectangle's voxel of smallest coordinates and d | (nr - 1) << 8 | (ns - 1) << 20
    std::vector<uint32_t> surfaceRects(bool closed = true, uint64_t first = 0, uint64_t capacity = ~0ull)
    {
        return extractRects<uint32_t>(VRC_SURFACE_FACES, 4, closed, first, capacity);
    }
    // 2n x 9: two triangles per rectangle in xorMesh's fixed point, wound outwards
    std::vector<int32_t> rectTriangles(bool closed = true, uint64_t first = 0, uint64_t capacity = ~0ull)
    {
        return extractRects<int32_t>(VRC_SURFACE_TRIANGLES, 18, closed, first, capacity);
    }
    // the same into device memory, asynchronous on `stream`; total_dev (may be null): a device uint64_t that receives the
    // number of rectangles in stream order
    void extractRectsDevice(int format, uint64_t first, uint64_t capacity, void* out_dev, uint64_t* total_dev, bool closed = true,
                            void* stream = nullptr)
    {
        flush();
        check(vrc_extract_rects(v_, closed ? 1 : 0, format, first, capacity, out_dev, total_dev, VRC_MEM_DEVICE, stream),
              "vrc_extract_rects");
    }
    // Wavefront OBJ of the exposed faces: one `v` line per distinct corner (voxel units), one `f` line per face with four
    // 1-based indices, wound outwards.  merged: one `f` line per rectangle of surfaceRects instead; rectangles share the
    // corners they have in common.  Returns the number of `f` lines.
    uint64_t toObj(const std::string& path, bool closed = true, bool merged = false)
    {
        const std::vector<uint32_t> faces = merged ? surfaceRects(closed) : surfaceFaces(closed);
        const uint64_t n = faces.size() / 4, side = (1ull << depth()) + 1;
        std::vector<uint64_t> corner(4 * n);          // (x * side + y) * side + z of each face's corners, in winding order
        for (uint64_t i = 0; i < n; ++i) {
            const uint32_t d = faces[4 * i + 3] & 0xffu, a = d >> 1, s = d & 1, u = (a + 1) % 3, w = (a + 2) % 3;
            // the extents: 1 along a, nr along the run axis (z, or y for the z faces), ns along the stack axis
            uint32_t e[3] = {1, 1, 1};
            const uint32_t r = a == 2 ? 1 : 2;
            e[r] = ((faces[4 * i + 3] >> 8) & 0x3ffu) + 1;
            e[3 - a - r] = ((faces[4 * i + 3] >> 20) & 0x3ffu) + 1;
            static const uint32_t du[4] = {0, 1, 1, 0}, dw[4] = {0, 0, 1, 1};
            for (uint32_t k = 0; k < 4; ++k) {
                const uint32_t j = s ? k : (4 - k) % 4;      // q0 q1 q2 q3 towards +axis, q0 q3 q2 q1 towards -axis
                uint64_t q[3];
                q[a] = faces[4 * i + a] + s;
                q[u] = faces[4 * i + u] + du[j] * e[u];
                q[w] = faces[4 * i + w] + dw[j] * e[w];
                corner[4 * i + k] = (q[0] * side + q[1]) * side + q[2];
            }
        }
        std::vector<uint64_t> verts(corner);
        std::sort(verts.begin(), verts.end());
        verts.erase(std::unique(verts.begin(), verts.end()), verts.end());
        std::ofstream f(path);
        if (!f) throw std::runtime_error("toObj: cannot open " + path);
        for (size_t i = 0; i < verts.size(); ++i)
            f << "v " << verts[i] / (side * side) << ' ' << verts[i] / side % side << ' ' << verts[i] % side << '\n';
        for (uint64_t i = 0; i < n; ++i) {
            f << 'f';
            for (uint32_t k = 0; k < 4; ++k)
                f << ' ' << (std::lower_bound(verts.begin(), verts.end(), corner[4 * i + k]) - verts.begin()) + 1;
            f << '\n';
        }
        if (!f.flush()) throw std::runtime_error("toObj: write to " + path + " failed");
        return n;
    }
    std::unique_ptr<HipLSVO> commit(float* build_ms = nullptr)
    {
        flush();
        vrc_scene* s = nullptr;
        check(vrc_volume_commit(v_, &s, build_ms), "vrc_volume_commit");
        return std::unique_ptr<HipLSVO>(new HipLSVO(s, device_));
    }
    uint64_t solidCount()
    {
        flush();
        uint64_t n = 0;
        check(vrc_volume_solid_count(v_, &n), "vrc_volume_solid_count");
        return n;
    }
    // The volume as its sparse tile stream (include/vrc.h: vrc_pack_volume; format version 1) and back.  packInfo: what pack
    // would write, the count and scan passes alone.  unpack replaces the whole occupancy; a stream that breaks a canonical
    // rule throws with the rule's name and leaves the volume as it was.  All synchronous.
    vrc_pack_info packInfo()
    {
        flush();
        vrc_pack_info info;
        check(vrc_pack_volume(v_, nullptr, 0, &info, VRC_MEM_HOST), "vrc_pack_volume");
        return info;
    }
    std::vector<uint8_t> pack()
    {
        vrc_pack_info info = packInfo();
        std::vector<uint8_t> out((size_t)info.bytes);
        check(vrc_pack_volume(v_, out.data(), out.size(), &info, VRC_MEM_HOST), "vrc_pack_volume");
        return out;
    }
    void unpack(const uint8_t* data, uint64_t bytes)
    {
        flush();
        check(vrc_unpack_volume(v_, data, bytes, VRC_MEM_HOST), "vrc_unpack_volume");
    }
    void unpack(const std::vector<uint8_t>& stream) { unpack(stream.data(), stream.size()); }
    void save(const std::string& path)
    {
        const std::vector<uint8_t> stream = pack();
        std::ofstream f(path, std::ios::binary);
        f.write((const char*)stream.data(), (std::streamsize)stream.size());
        if (!f.flush()) throw std::runtime_error("save: write to " + path + " failed");
    }
    // a new volume from a file written by save(); the depth is the header's (vrc_pack_header)
    static std::unique_ptr<HipVoxelVolume> load(const std::string& path, int device = 0)
    {
        std::ifstream f(path, std::ios::binary);
        if (!f) throw std::runtime_error("load: cannot open " + path);
        const std::vector<uint8_t> stream((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        vrc_pack_info info;
        uint8_t head[64] = {0};
        std::copy(stream.begin(), stream.begin() + std::min<size_t>(64, stream.size()), head);
        check(vrc_pack_header(head, stream.size(), &info), "vrc_pack_header");
        std::unique_ptr<HipVoxelVolume> volume(new HipVoxelVolume(info.depth, device));
        volume->unpack(stream);
        return volume;
    }
    uint64_t editScratchBytes() const
    {
        uint64_t n = 0;
        check(vrc_volume_edit_scratch_bytes(v_, &n), "vrc_volume_edit_scratch_bytes");
        return n;
    }
    uint32_t depth() const { return vrc_volume_depth(v_); }
    vrc_volume* handle() const { return v_; }

private:
    template <class T>
    std::vector<T> extractSurface(int format, size_t per_face, bool closed, uint64_t first, uint64_t capacity)
    {
        flush();
        uint64_t total = 0;
        check(vrc_volume_extract_surface(v_, closed ? 1 : 0, format, 0, 0, nullptr, &total, VRC_MEM_HOST, nullptr), "vrc_volume_extract_surface");
        const uint64_t n = first < total ? std::min(capacity, total - first) : 0;
        std::vector<T> out((size_t)n * per_face);
        if (n) check(vrc_volume_extract_surface(v_, closed ? 1 : 0, format, first, n, out.data(), nullptr, VRC_MEM_HOST, nullptr), "vrc_volume_extract_surface");
        return out;
    }
    template <class T>
    std::vector<T> extractRects(int format, size_t per_rect, bool closed, uint64_t first, uint64_t capacity)
    {
        flush();
        uint64_t total = 0;
        check(vrc_extract_rects(v_, closed ? 1 : 0, format, 0, 0, nullptr, &total, VRC_MEM_HOST, nullptr), "vrc_extract_rects");
        const uint64_t n = first < total ? std::min(capacity, total - first) : 0;
        std::vector<T> out((size_t)n * per_rect);
        if (n) check(vrc_extract_rects(v_, closed ? 1 : 0, format, first, n, out.data(), nullptr, VRC_MEM_HOST, nullptr), "vrc_extract_rects");
        return out;
    }
    static std::vector<int32_t> meshSoup(const std::vector<int64_t>& fixed, const std::vector<uint32_t>& faces, const int64_t origin[3])
    {
        std::vector<int32_t> tris(faces.size() * 3);
        for (size_t i = 0; i < faces.size(); ++i) {
            if ((size_t)faces[i] * 3 + 2 >= fixed.size()) throw std::invalid_argument("mesh: a face names a vertex that does not exist");
            for (int a = 0; a < 3; ++a) tris[3 * i + a] = (int32_t)(fixed[(size_t)faces[i] * 3 + a] - origin[a]);
        }
        return tris;
    }
    HipVoxelVolume(vrc_volume* adopted, int device) : v_(adopted), device_(device) {}
    vrc_volume* v_ = nullptr;
    int device_ = 0;
    std::vector<uint32_t> queue_;
    bool queue_solid_ = true;
};

// Undo and redo for a HipVoxelVolume at the cost of what each step changed: one shadow clone and two stacks of deltas.  Edit
// the volume with any call, then record(); only record() reads the two occupancies.  max_bytes (0: no limit) bounds the
// record bytes of both stacks: record() drops the oldest undo steps beyond it, never the one it has just taken.  The volume
// must outlive the history.  The pointers returned stay owned by the history and hold until its next call.
class HipVoxelHistory {
public:
    explicit HipVoxelHistory(HipVoxelVolume& volume, uint64_t max_bytes = 0) : volume_(volume), shadow_(volume.clone()), max_bytes_(max_bytes) {}
    // the step from the state at the last record / undo / redo to the volume as it is now, or nullptr when nothing changed
    const HipVoxelDelta* record()
    {
        HipVoxelDelta delta = shadow_->diff(volume_);
        if (!delta.count()) return nullptr;
        shadow_->applyDelta(delta);
        undo_.push_back(std::move(delta));
        redo_.clear();
        while (max_bytes_ && undo_.size() > 1 && bytes() > max_bytes_) undo_.erase(undo_.begin());
        return &undo_.back();
    }
    // takes the last recorded step back (its stats name the box to redraw); nullptr with nothing to undo
    const HipVoxelDelta* undo() { return move(undo_, redo_); }
    const HipVoxelDelta* redo() { return move(redo_, undo_); }
    size_t undoCount() const { return undo_.size(); }
    size_t redoCount() const { return redo_.size(); }
    // record bytes held by both stacks (the shadow clone's occupancy is not counted)
    uint64_t bytes() const
    {
        uint64_t n = 0;
        for (const HipVoxelDelta& d : undo_) n += d.bytes();
        for (const HipVoxelDelta& d : redo_) n += d.bytes();
        return n;
    }

private:
    const HipVoxelDelta* move(std::vector<HipVoxelDelta>& source, std::vector<HipVoxelDelta>& sink)
    {
        if (source.empty()) return nullptr;
        volume_.applyDelta(source.back());
        shadow_->applyDelta(source.back());
        sink.push_back(std::move(source.back()));
        source.pop_back();
        return &sink.back();
    }
    HipVoxelVolume& volume_;
    std::unique_ptr<HipVoxelVolume> shadow_;
    uint64_t max_bytes_ = 0;
    std::vector<HipVoxelDelta> undo_, redo_;
};

inline void HipVoxelLabels::select(const std::vector<uint8_t>& keep, HipVoxelVolume& dst, int op) const
{
    if (keep.size() != count()) throw std::invalid_argument("HipVoxelLabels::select: keep must have one byte per component");
    dst.flush();
    check(vrc_labels_select(l_, keep.empty() ? nullptr : keep.data(), dst.handle(), op, VRC_MEM_HOST, nullptr), "vrc_labels_select");
}

inline std::vector<int32_t> HipVoxelLabels::fall(HipVoxelVolume* fixed, int direction, uint32_t drop_limit, vrc_fall_stats* stats) const
{
    if (fixed) fixed->flush();
    std::vector<int32_t> offsets((size_t)count() * 3u);
    check(vrc_fall_drops(l_, fixed ? fixed->handle() : nullptr, direction, drop_limit, offsets.empty() ? nullptr : offsets.data(), VRC_MEM_HOST, stats),
          "vrc_fall_drops");
    return offsets;
}

inline void HipVoxelLabels::place(const std::vector<int32_t>& offsets, HipVoxelVolume& dst, int op, const std::vector<uint8_t>* keep) const
{
    if (offsets.size() != count() * 3u) throw std::invalid_argument("HipVoxelLabels::place: offsets must have three entries per component");
    if (keep && keep->size() != count()) throw std::invalid_argument("HipVoxelLabels::place: keep must have one byte per component");
    dst.flush();
    check(vrc_fall_place(l_, keep && !keep->empty() ? keep->data() : nullptr, offsets.empty() ? nullptr : offsets.data(), dst.handle(), op, VRC_MEM_HOST, nullptr),
          "vrc_fall_place");
}

inline void HipVoxelLabels::placeAffine(const std::vector<vrc_affine>& maps, HipVoxelVolume& dst, int op, const std::vector<uint32_t>* boxes,
                                        const std::vector<uint8_t>* keep) const
{
    if (maps.size() != count()) throw std::invalid_argument("HipVoxelLabels::placeAffine: maps must have one entry per component");
    if (boxes && boxes->size() != count() * 6u) throw std::invalid_argument("HipVoxelLabels::placeAffine: boxes must have six entries per component");
    if (keep && keep->size() != count()) throw std::invalid_argument("HipVoxelLabels::placeAffine: keep must have one byte per component");
    dst.flush();
    check(vrc_rigid_place_affine(l_, keep && !keep->empty() ? keep->data() : nullptr, maps.empty() ? nullptr : maps.data(),
                                 boxes && !boxes->empty() ? boxes->data() : nullptr, dst.handle(), op, VRC_MEM_HOST, nullptr),
          "vrc_rigid_place_affine");
}

inline std::vector<vrc_piece_contact> HipVoxelLabels::contacts(const std::vector<vrc_affine>& maps, HipVoxelVolume& world, const std::vector<uint32_t>* boxes,
                                                               const std::vector<uint8_t>* keep) const
{
    if (maps.size() != count()) throw std::invalid_argument("HipVoxelLabels::contacts: maps must have one entry per component");
    if (boxes && boxes->size() != count() * 6u) throw std::invalid_argument("HipVoxelLabels::contacts: boxes must have six entries per component");
    if (keep && keep->size() != count()) throw std::invalid_argument("HipVoxelLabels::contacts: keep must have one byte per component");
    world.flush();
    std::vector<vrc_piece_contact> out((size_t)count());
    check(vrc_rigid_contacts(l_, keep && !keep->empty() ? keep->data() : nullptr, maps.empty() ? nullptr : maps.data(),
                             boxes && !boxes->empty() ? boxes->data() : nullptr, world.handle(), out.empty() ? nullptr : out.data(), VRC_MEM_HOST, nullptr),
          "vrc_rigid_contacts");
    return out;
}

inline std::vector<uint32_t> HipVoxelLabels::candidatePairs(const std::vector<uint32_t>& boxes, uint32_t posed_depth, const std::vector<uint8_t>* keep) const
{
    if (boxes.size() != count() * 6u) throw std::invalid_argument("HipVoxelLabels::candidatePairs: boxes must have six entries per component");
    if (keep && keep->size() != count()) throw std::invalid_argument("HipVoxelLabels::candidatePairs: keep must have one byte per component");
    const uint8_t* k = keep && !keep->empty() ? keep->data() : nullptr;
    const uint32_t* b = boxes.empty() ? nullptr : boxes.data();
    uint64_t n = 0;
    check(vrc_rigid_box_pair_count(l_, k, b, posed_depth, &n, VRC_MEM_HOST, nullptr), "vrc_rigid_box_pair_count");
    std::vector<uint32_t> pairs((size_t)n * 2u);
    if (n) check(vrc_rigid_box_pairs(l_, k, b, posed_depth, 0, n, pairs.data(), VRC_MEM_HOST, nullptr), "vrc_rigid_box_pairs");
    return pairs;
}

inline std::vector<vrc_piece_contact> HipVoxelLabels::pairContacts(const std::vector<vrc_affine>& maps, const std::vector<uint32_t>& pairs, uint32_t posed_depth,
                                                                   const std::vector<uint32_t>* boxes, const std::vector<uint8_t>* keep) const
{
    if (maps.size() != count()) throw std::invalid_argument("HipVoxelLabels::pairContacts: maps must have one entry per component");
    if (boxes && boxes->size() != count() * 6u) throw std::invalid_argument("HipVoxelLabels::pairContacts: boxes must have six entries per component");
    if (keep && keep->size() != count()) throw std::invalid_argument("HipVoxelLabels::pairContacts: keep must have one byte per component");
    if (pairs.size() & 1u) throw std::invalid_argument("HipVoxelLabels::pairContacts: pairs must have two entries per pair");
    std::vector<vrc_piece_contact> out(pairs.size() / 2u);
    check(vrc_rigid_pair_contacts(l_, keep && !keep->empty() ? keep->data() : nullptr, maps.empty() ? nullptr : maps.data(),
                                  boxes && !boxes->empty() ? boxes->data() : nullptr, posed_depth, out.size(), pairs.empty() ? nullptr : pairs.data(),
                                  out.empty() ? nullptr : out.data(), VRC_MEM_HOST, nullptr),
          "vrc_rigid_pair_contacts");
    return out;
}

inline std::vector<vrc_piece_clearance> HipVoxelLabels::clearance(const std::vector<vrc_affine>& maps, const HipVoxelDistance& field,
                                                                  const std::vector<uint32_t>* boxes, const std::vector<uint8_t>* keep) const
{
    if (maps.size() != count()) throw std::invalid_argument("HipVoxelLabels::clearance: maps must have one entry per component");
    if (boxes && boxes->size() != count() * 6u) throw std::invalid_argument("HipVoxelLabels::clearance: boxes must have six entries per component");
    if (keep && keep->size() != count()) throw std::invalid_argument("HipVoxelLabels::clearance: keep must have one byte per component");
    std::vector<vrc_piece_clearance> out((size_t)count());
    check(vrc_rigid_clearance(l_, keep && !keep->empty() ? keep->data() : nullptr, maps.empty() ? nullptr : maps.data(),
                              boxes && !boxes->empty() ? boxes->data() : nullptr, field.handle(), out.empty() ? nullptr : out.data(), VRC_MEM_HOST, nullptr),
          "vrc_rigid_clearance");
    return out;
}

inline void HipVoxelDistance::select(uint32_t lo, uint32_t hi, HipVoxelVolume& dst, int op) const
{
    dst.flush();
    check(vrc_distance_select(d_, lo, hi, dst.handle(), op, nullptr), "vrc_distance_select");
}

// Camera values Camera::getRay reads (camera_controller.hpp:16-49); the Camera /
// FlyController classes themselves stay untouched on the host.
struct CameraState {
    Vec3 position{0, 0, 0};
    Vec2 view_angle{0, 0};
    float aperture = 0.0f, focal_length = 1.0f, fov = 1.0f;
    vrc_camera to_abi() const
    {
        vrc_camera c;
        c.position[0] = position.x; c.position[1] = position.y; c.position[2] = position.z;
        vrc_make_rotation(view_angle.x, view_angle.y, c.rot);   // generateRotationMatrix, utils.cpp:94-100
        c.fov = fov; c.aperture = aperture; c.focal_length = focal_length;
        return c;
    }
};

// RayCaster (raycaster.hpp:43-283).  render_image and the Sample accumulators
// live in HBM; renderFrame replaces the swarm lambda of main.cpp:139-152.
class HipRayCaster {
public:
    HipRayCaster(const HipLSVO& svo, uint32_t width, uint32_t height) : width_(width), height_(height)
    {
        check(vrc_renderer_create(svo.handle(), width, height, &r_), "vrc_renderer_create");
    }
    ~HipRayCaster() { vrc_renderer_destroy(r_); }
    HipRayCaster(const HipRayCaster&) = delete;
    HipRayCaster& operator=(const HipRayCaster&) = delete;

    void setLightPosition(const Vec3& position) { light_ = position; }   // raycaster.hpp:62
    // the rebind `const LSVO<N>& svo` (raycaster.hpp:265) cannot do: the following frames walk `svo` (same depth, same
    // device, e.g. HipVoxelVolume::commit()'s); image, accumulators and counters are kept
    void setScene(const HipLSVO& svo) { check(vrc_renderer_set_scene(r_, svo.handle()), "vrc_renderer_set_scene"); }

    // One frame: Camera::getRay + renderRay for every selected pixel (main.cpp:139-152).
    // checker_board_offset = -1 renders every pixel; 0 / 1 as main.cpp:137,143.
    // Multi-GPU: this process renders the row blocks b (of `row_block` rows) with b % shard_count == shard_index.
    void setShard(uint32_t row_block, uint32_t shard_index, uint32_t shard_count)
    {
        row_block_ = row_block; shard_index_ = shard_index; shard_count_ = shard_count ? shard_count : 1;
    }

    void renderFrame(const CameraState& camera, int32_t checker_board_offset = -1, uint32_t spp = 1, void* stream = nullptr)
    {
        vrc_frame_params p{};
        p.row_block = row_block_; p.shard_index = shard_index_; p.shard_count = shard_count_;
        p.light_position[0] = light_.x; p.light_position[1] = light_.y; p.light_position[2] = light_.z;
        p.use_gi = use_gi; p.use_samples = use_samples;
        p.shadow_samples = 0; p.gi_bounces = 1;
        p.checker_parity = checker_board_offset; p.spp = spp;
        p.seed = seed; p.frame_index = frame_index_;
        const vrc_camera c = camera.to_abi();
        check(vrc_render_frame(r_, &c, &p, stream), "vrc_render_frame");
        frame_index_ += spp;
    }

    // One progressive frame in one launch: renderFrame (sample mode, every pixel) + samples_to_image + resetSamples, the
    // resolved rows also written to `shard_dev` (device, may be null) as the multi-GPU exchange expects them.
    void renderFrameResolved(const CameraState& camera, uint32_t spp, void* shard_dev = nullptr, void* stream = nullptr)
    {
        vrc_frame_params p{};
        p.row_block = row_block_; p.shard_index = shard_index_; p.shard_count = shard_count_;
        p.light_position[0] = light_.x; p.light_position[1] = light_.y; p.light_position[2] = light_.z;
        p.use_gi = use_gi; p.use_samples = 1;
        p.shadow_samples = 0; p.gi_bounces = 1;
        p.checker_parity = -1; p.spp = spp;
        p.seed = seed; p.frame_index = frame_index_;
        const vrc_camera c = camera.to_abi();
        check(vrc_render_frame_resolved(r_, &c, &p, shard_dev, stream), "vrc_render_frame_resolved");
        frame_index_ += spp;
    }

    // Frames kept in flight: a work unit = all `spp` samples of a tile ...
    void setSampleChunk(uint32_t samples_per_unit) { check(vrc_renderer_set_sample_chunk(r_, samples_per_unit), "vrc_renderer_set_sample_chunk"); }
    // ... and, beyond the reference, the sample-invariant primary / shadow walks of a pinhole camera done once per unit
    void setInvariantRayReuse(bool on) { check(vrc_renderer_set_invariant_ray_reuse(r_, on ? 1u : 0u), "vrc_renderer_set_invariant_ray_reuse"); }
    void setLaneSamples(uint32_t samples) { check(vrc_renderer_set_lane_samples(r_, samples), "vrc_renderer_set_lane_samples"); }
    void setQuadWalks(bool on) { check(vrc_renderer_set_quad_walks(r_, on ? 1u : 0u), "vrc_renderer_set_quad_walks"); }
    void setWalkFromRoot(bool on) { check(vrc_renderer_set_walk_from_root(r_, on ? 1u : 0u), "vrc_renderer_set_walk_from_root"); }

    void samples_to_image(void* stream = nullptr) { check(vrc_samples_to_image(r_, stream), "vrc_samples_to_image"); }   // raycaster.hpp:94
    void resetSamples(void* stream = nullptr) { check(vrc_reset_samples(r_, stream), "vrc_reset_samples"); }            // raycaster.hpp:105
    // samples_to_image for this shard's rows, written into `shard_dev` (device, vrc_shard_bytes) as the all-gather
    // expects it; `reset` also clears those rows' accumulators (= resetSamples) in the same pass
    void resolveShard(void* shard_dev, bool reset, void* stream = nullptr)
    {
        check(vrc_resolve_shard(r_, row_block_, shard_index_, shard_count_, shard_dev, reset ? 1 : 0, stream), "vrc_resolve_shard");
    }

    // render_image (raycaster.hpp:261) copied to host RGBA8, row-major
    std::vector<uint8_t> render_image() const
    {
        std::vector<uint8_t> img((size_t)width_ * height_ * 4);
        check(vrc_read_image(r_, img.data(), nullptr), "vrc_read_image");
        return img;
    }

    vrc_frame_stats stats(bool reset = false)
    {
        vrc_frame_stats s;
        check(vrc_get_stats(r_, &s, reset ? 1 : 0, nullptr), "vrc_get_stats");
        return s;
    }

    // Direct peer writes: the presenting process exports its framebuffer, the others resolve
    // their shards of the frame straight into it
    vrc_ipc_handle exportImage() const { vrc_ipc_handle h; check(vrc_ipc_export_image(r_, &h), "vrc_ipc_export_image"); return h; }
    void setImageTarget(void* image_dev) { check(vrc_renderer_set_image_target(r_, image_dev), "vrc_renderer_set_image_target"); }

    vrc_renderer* handle() const { return r_; }
    // sample counter of the next frame (the RNG key: frame_index + sample); renderFrame* advance it by spp
    void setFrameIndex(uint32_t frame_index) { frame_index_ = frame_index; }
    uint32_t frameIndex() const { return frame_index_; }
    std::vector<uint8_t> render_image(void* stream) const     // the same copy, ordered after (and waiting for) `stream` only
    {
        std::vector<uint8_t> img((size_t)width_ * height_ * 4);
        check(vrc_read_image(r_, img.data(), stream), "vrc_read_image");
        return img;
    }
    vrc_frame_stats stats(bool reset, void* stream)
    {
        vrc_frame_stats s;
        check(vrc_get_stats(r_, &s, reset ? 1 : 0, stream), "vrc_get_stats");
        return s;
    }

    bool use_gi = false;        // raycaster.hpp:274
    bool use_samples = false;   // raycaster.hpp:275
    uint32_t seed = 0x9E3779B9u;

private:
    vrc_renderer* r_ = nullptr;
    uint32_t width_, height_;
    uint32_t frame_index_ = 0;
    uint32_t row_block_ = 0, shard_index_ = 0, shard_count_ = 1;
    Vec3 light_{0, 0, 0};
};

// Progressive frames kept in flight -- for hosts that do not need frame i before they issue
// frame i + 1: an offline render, a replay (readReplay below), a multi-GPU shard.  `frames_in_flight` renderers and
// streams take turns; a work unit is a tile's whole sample set and the resolve is fused into the frame kernel, which is the
// fastest form once launches overlap.  submit() returns at once; image(slot) waits for that slot's frame only.  Frame n
// is the frame a single HipRayCaster would render n-th with the same spp (frame_index = n * spp), bit for bit.
class HipFramePipeline {
public:
    HipFramePipeline(const HipLSVO& svo, uint32_t width, uint32_t height, uint32_t spp, uint32_t frames_in_flight = 3, int device = 0)
        : device_(device), spp_(spp ? spp : 1)
    {
        if (frames_in_flight == 0) frames_in_flight = 1;
        for (uint32_t i = 0; i < frames_in_flight; ++i) {
            slots_.emplace_back(new HipRayCaster(svo, width, height));
            slots_.back()->setSampleChunk(spp_);
            void* st = nullptr;
            check(vrc_stream_create(device, &st), "vrc_stream_create");
            streams_.push_back(st);
        }
    }
    ~HipFramePipeline()
    {
        for (void* st : streams_) { vrc_stream_synchronize(device_, st); vrc_stream_destroy(device_, st); }
    }
    HipFramePipeline(const HipFramePipeline&) = delete;
    HipFramePipeline& operator=(const HipFramePipeline&) = delete;

    void setLightPosition(const Vec3& position) { for (auto& r : slots_) r->setLightPosition(position); }
    void setUseGI(bool on) { for (auto& r : slots_) r->use_gi = on; }
    void setSeed(uint32_t seed) { for (auto& r : slots_) r->seed = seed; }
    void setInvariantRayReuse(bool on) { for (auto& r : slots_) r->setInvariantRayReuse(on); }
    void setShard(uint32_t row_block, uint32_t shard_index, uint32_t shard_count)
    {
        for (auto& r : slots_) r->setShard(row_block, shard_index, shard_count);
    }
    uint32_t framesInFlight() const { return (uint32_t)slots_.size(); }

    // Issues frame number `submitted()` and returns its slot.  The slot's previous frame (F submits ago) is overwritten:
    // read it first.  `shard_dev`: where the resolved rows also go (device; multi-GPU exchange buffer), may be null.
    uint32_t submit(const CameraState& camera, void* shard_dev = nullptr)
    {
        const uint32_t slot = (uint32_t)(n_ % slots_.size());
        slots_[slot]->setFrameIndex((uint32_t)(n_ * spp_));
        slots_[slot]->renderFrameResolved(camera, spp_, shard_dev, streams_[slot]);
        ++n_;
        return slot;
    }
    uint64_t submitted() const { return n_; }
    uint32_t nextSlot() const { return (uint32_t)(n_ % slots_.size()); }     // the slot (and stream) the next submit() uses
    void wait(uint32_t slot) { check(vrc_stream_synchronize(device_, streams_[slot]), "vrc_stream_synchronize"); }
    void waitAll() { for (uint32_t i = 0; i < slots_.size(); ++i) wait(i); }
    // waitAll() for streams that wait for peers' frame flags (direct peer writes): never a blind synchronize -- a stream-ordered
    // wait has no timeout.  Polls the streams, the peers' process ids and a deadline (vrc_ipc_stream_wait); when a peer is gone
    // every wait on the flags is released in every process and this throws (VRC_ERR_PEER).
    void waitAllWatched(vrc_ipc_flags* flags, const std::vector<int32_t>& peer_pids, uint32_t timeout_ms = 120000)
    {
        int first = 0;
        std::string why;
        for (void* st : streams_) {
            // after a failure the remaining streams are still drained (each call holds the release while its stream empties): a
            // process must not leave with a wait pending on the device
            const int rc = vrc_ipc_stream_wait(flags, st, peer_pids.data(), (uint32_t)peer_pids.size(), timeout_ms);
            if (rc != 0 && first == 0) { first = rc; why = vrc_last_error(); }
        }
        if (first != 0) throw std::runtime_error("vrc_ipc_stream_wait: " + why);
    }
    std::vector<uint8_t> image(uint32_t slot) { return slots_[slot]->render_image(streams_[slot]); }   // waits for that slot
    void* image_device_ptr(uint32_t slot) const { return vrc_image_device_ptr(slots_[slot]->handle()); }
    void* stream(uint32_t slot) const { return streams_[slot]; }
    HipRayCaster& raycaster(uint32_t slot) { return *slots_[slot]; }
    // counters of the frames rendered on `slot` since the last reset (waits for that slot)
    vrc_frame_stats stats(uint32_t slot, bool reset = false) { return slots_[slot]->stats(reset, streams_[slot]); }

private:
    int device_;
    uint32_t spp_;
    uint64_t n_ = 0;
    std::vector<std::unique_ptr<HipRayCaster>> slots_;
    std::vector<void*> streams_;
};

// The blend / upscale chain main.cpp runs on render_image after every frame (main.cpp:160-182: render_tex,
// denoised_tex, final_sprite), device resident.  present() replaces lines 160-181; the window image stays in HBM
// (window_device_ptr) or is copied out (window()).
class HipPresenter {
public:
    HipPresenter(uint32_t render_width, uint32_t render_height, uint32_t win_width, uint32_t win_height, int device = 0)
        : out_w_(win_width), out_h_(win_height)
    {
        check(vrc_presenter_create(device, render_width, render_height, win_width, win_height, &p_), "vrc_presenter_create");
    }
    ~HipPresenter() { vrc_presenter_destroy(p_); }
    HipPresenter(const HipPresenter&) = delete;
    HipPresenter& operator=(const HipPresenter&) = delete;

    // old_value_conservation as main.cpp:161 computes it from raycaster.use_samples
    void present(HipRayCaster& raycaster, uint32_t median = 0, void* stream = nullptr)
    {
        const float old_value_conservation = raycaster.use_samples ? 0.0f : 0.1f;
        check(vrc_present(p_, raycaster.handle(), old_value_conservation, median, stream), "vrc_present");
        last_stream_ = stream;
    }
    void* window_device_ptr() const { return vrc_presenter_window_ptr(p_); }
    // Copies the window image out, ordered after the last present(): the read runs on THAT call's stream (frame streams are
    // non-blocking, the NULL stream does not wait for them).
    std::vector<uint8_t> window() const
    {
        std::vector<uint8_t> img((size_t)out_w_ * out_h_ * 4);
        check(vrc_presenter_read(p_, img.data(), nullptr, last_stream_), "vrc_presenter_read");
        return img;
    }

private:
    vrc_presenter* p_ = nullptr;
    uint32_t out_w_, out_h_;
    void* last_stream_ = nullptr;
};

// Camera-path replay files.  The format is the one include/replay.hpp:8-35 reads: whitespace-separated numbers, six per
// tick (time, position x y z, view angles x y); a tick counts only when all six parse, reading ends at the first word that
// is not a number, a missing file gives no ticks (pinned against the reference's reader: tests/golden/replay_cases.json).
// Here a tick is what the renderer consumes -- a time and a camera pose; the lens values, which the file does not carry,
// come from the caller.  The reference has the reader but no caller; this one feeds deterministic multi-frame runs
// (tests/cpp/replay_main.cpp; tools/replay_bench.py speaks the same format).
struct ReplayTick {
    float time = 0.0f;
    CameraState pose;
};

inline std::vector<ReplayTick> readReplay(const std::string& path, float aperture = 0.0f, float focal_length = 1.0f, float fov = 1.0f)
{
    std::vector<ReplayTick> ticks;
    std::ifstream in(path);
    for (;;) {
        float v[6];
        int got = 0;
        while (got < 6 && (in >> v[got])) ++got;
        if (got < 6) break;
        ReplayTick t;
        t.time = v[0];
        t.pose.position = {v[1], v[2], v[3]};
        t.pose.view_angle = {v[4], v[5]};
        t.pose.aperture = aperture; t.pose.focal_length = focal_length; t.pose.fov = fov;
        ticks.push_back(t);
    }
    return ticks;
}

}  // namespace vrc_host

#ifdef VRC_WITH_REFERENCE_HEADERS
// Drop-in Volumetric (needs the reference's include/ and GLM on the include path).
#include "volumetric.hpp"
class HipVolumetric : public Volumetric {
public:
    HipVolumetric(const vrc_lnode* lnodes, uint64_t n_nodes, uint32_t depth, int device = 0) : impl_(lnodes, n_nodes, depth, device)
    {
        cell_.type = Cell::Solid; cell_.texture = Cell::Grass;
    }
    HitPoint castRay(const glm::vec3& position, glm::vec3 direction, const float coef, const float bias) const override
    {
        const vrc_host::HitPoint h = impl_.castRay({position.x, position.y, position.z}, {direction.x, direction.y, direction.z}, coef, bias);
        HitPoint out;
        out.position = glm::vec3(h.position.x, h.position.y, h.position.z);
        out.normal = glm::vec3(h.normal.x, h.normal.y, h.normal.z);
        out.voxel_coord = glm::vec2(h.voxel_coord.x, h.voxel_coord.y);
        out.cell = h.cell ? &cell_ : nullptr;
        out.distance = h.distance;
        out.complexity = h.complexity;
        return out;
    }
    void setCell(Cell::Type, Cell::Texture, uint32_t, uint32_t, uint32_t) override {}
    const vrc_host::HipLSVO& impl() const { return impl_; }
private:
    vrc_host::HipLSVO impl_;
    Cell cell_;
};
#endif
