// Exercises the column methods of the C++ host adapter (cpuvoxelraycaster_amd/host/hip_raycaster.hpp) at 32^3: the profile of
// a seeded fill along every direction and in a rect, the maps made from it, fillColumns with maps and constants under the
// three ops, raiseTerrain, selectColumns and its one-liners.  FNV-1a hashes of the records and downloads are printed, and the
// pytest wrapper compares them with the numpy model's.  Then one column of 512^3 that holds 256 runs of one voxel, whose record
// is printed field by field for both sides: beyond the 128 runs that 32^3 .. 128^3 can hold.
#include <cstdio>
#include <vector>

#include "../../cpuvoxelraycaster_amd/host/hip_raycaster.hpp"

static unsigned long long fnv1a(const void* p, size_t n)
{
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
    return h;
}

template <class T>
static unsigned long long hash_of(const std::vector<T>& v) { return fnv1a(v.data(), v.size() * sizeof(T)); }

static unsigned long long hash_of(vrc_host::HipVoxelVolume& v)
{
    std::vector<uint8_t> solid((size_t)1 << (3u * v.depth()));
    vrc_host::check(vrc_volume_download(v.handle(), solid.data()), "vrc_volume_download");
    return fnv1a(solid.data(), solid.size());
}

int main()
{
    try {
        const int32_t S = 32;
        vrc_host::HipVoxelVolume world(5), other(5);
        world.fillRandom(7, 0.45);
        for (int d = 0; d < 6; ++d) std::printf("profile%d=%llu\n", d, hash_of(world.columnProfile(d)));
        const uint32_t rect[4] = {3, 5, 30, 18};
        std::printf("rect=%llu\n", hash_of(world.columnProfile(2, rect)));
        std::printf("height=%llu thickness=%llu field=%d\n", hash_of(world.heightMap(2, -7)), hash_of(world.thicknessMap(0)), (int)world.isHeightField(2));

        // lo(u, v) = u - 3, hi(u, v) = 2 v - 9 over the rect: negative, crossing and beyond S
        std::vector<int32_t> lo, hi;
        for (int32_t u = 3; u < 30; ++u)
            for (int32_t v = 5; v < 18; ++v) { lo.push_back(u - 3); hi.push_back(2 * v - 9); }
        world.fillColumns(0, lo.data(), 0, hi.data(), 0, rect, VRC_COPY_REPLACE);
        std::printf("replace=%llu\n", hash_of(world));
        world.fillColumns(2, nullptr, 4, hi.data(), 0, rect, VRC_COPY_OR);
        std::printf("or=%llu\n", hash_of(world));
        world.fillColumns(1, lo.data(), 0, nullptr, 20, rect, VRC_COPY_ANDNOT);
        std::printf("andnot=%llu\n", hash_of(world));
        world.fillColumns(1, nullptr, 30, nullptr, 31);
        std::printf("slab=%llu\n", hash_of(world));

        std::vector<int32_t> heights((size_t)S * S);
        for (int32_t x = 0; x < S; ++x)
            for (int32_t z = 0; z < S; ++z) heights[(size_t)x * S + z] = (x * 7 + z * 5) % 41 - 4;
        other.raiseTerrain(heights);
        std::printf("terrain=%llu field=%d grounded=%d\n", hash_of(other), (int)other.isHeightField(2), (int)other.isHeightField(2, true));

        world.selectColumns(other, 5, 2, 6, VRC_COLUMNS_SOLID | VRC_COLUMNS_EMPTY, VRC_COPY_OR);
        std::printf("select=%llu source=%llu\n", hash_of(other), hash_of(world));
        world.skyLit(other, 2);
        std::printf("lit=%llu\n", hash_of(other));
        world.topLayers(other, 1, 3);
        std::printf("top=%llu\n", hash_of(other));
        world.sheltered(other, 4);
        std::printf("sheltered=%llu\n", hash_of(other));

        // the column (x, z) = (301, 77) of 512^3 along y: solid at y = 1, 3, .. 511
        vrc_host::HipVoxelVolume tall(9);
        for (uint32_t y = 1; y < 512; y += 2) tall.fillBox(301, y, 77, 302, y + 1, 78, true);
        const uint32_t one[4] = {301, 77, 302, 78};
        for (int side = 0; side < 2; ++side) {
            const std::vector<vrc_column> c = tall.columnProfile(2 + side, one);
            std::printf("comb%d=%u,%u,%u,%u size=%zu\n", side, c[0].first, c[0].last, c[0].count, c[0].runs, c.size());
        }
        std::printf("comb_solid=%llu\n", (unsigned long long)tall.solidCount());
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 1;
    }
    return 0;
}
