// Exercises the morphology methods of the C++ host adapter (cpuvoxelraycaster_amd/host/hip_raycaster.hpp) at 32^3: morph with
// every element helper, an origin and the three ops, dilateBy / erodeBy / openBy / closeBy in place, fitsAt and match.
// FNV-1a hashes of the downloads are printed, and the pytest wrapper compares them with the numpy model's.
#include <cstdio>
#include <vector>

#include "../../cpuvoxelraycaster_amd/host/hip_raycaster.hpp"

typedef vrc_host::HipVoxelVolume V;

static unsigned long long fnv1a(const void* p, size_t n)
{
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
    return h;
}

static unsigned long long hash_of(V& v)
{
    std::vector<uint8_t> solid((size_t)1 << (3u * v.depth()));
    vrc_host::check(vrc_volume_download(v.handle(), solid.data()), "vrc_volume_download");
    return fnv1a(solid.data(), solid.size());
}

int main()
{
    try {
        V world(5), out(5);
        world.fillRandom(7, 0.2);
        std::printf("world=%llu\n", hash_of(world));

        out.fillBox(0, 0, 0, 32, 32, 32, true);                    // whatever dst holds is overwritten
        world.morph(out, VRC_MORPH_DILATE, V::elementBall(3));
        std::printf("ball=%llu\n", hash_of(out));
        const int32_t anchor[3] = {0, 4, 1};
        world.morph(out, VRC_MORPH_ERODE, V::elementBox(3, 5, 3, anchor), true, false);
        std::printf("box=%llu\n", hash_of(out));
        world.morph(out, VRC_MORPH_DILATE, V::elementCross(), false, true, VRC_COPY_OR);
        std::printf("cross=%llu\n", hash_of(out));
        world.morph(out, VRC_MORPH_DILATE, V::reflect(V::elementLine(2, 0, 16)), true, false, VRC_COPY_ANDNOT);
        std::printf("line=%llu\n", hash_of(out));
        const int32_t pivot[3] = {9, 1, 30};
        V::Element listed = V::elementBox(2, 3, 2);
        for (size_t i = 0; i < listed.size(); ++i) listed[i] += pivot[i % 3];
        world.morph(out, VRC_MORPH_ERODE, listed, true, true, VRC_COPY_REPLACE, pivot);
        std::printf("origin=%llu source=%llu\n", hash_of(out), hash_of(world));

        V shape(5);
        shape.fillRandom(9, 0.5);
        shape.dilateBy(V::elementLine(0, -2, 1));
        std::printf("dilate_by=%llu\n", hash_of(shape));
        shape.erodeBy(V::elementBox(2, 2, 2));
        std::printf("erode_by=%llu\n", hash_of(shape));
        shape.erodeBy(V::elementCross(), true);
        std::printf("erode_open=%llu\n", hash_of(shape));
        shape.fillRandom(13, 0.6, nullptr, VRC_COPY_REPLACE);
        shape.openBy(V::elementBall(1));
        std::printf("open_by=%llu\n", hash_of(shape));
        shape.closeBy(V::elementBox(2, 1, 3));
        std::printf("close_by=%llu\n", hash_of(shape));

        world.fitsAt(out, V::elementBox(2, 3, 2));
        std::printf("fits=%llu\n", hash_of(out));
        const int32_t solid_at[6] = {0, 0, 0, 0, -1, 0}, empty_at[6] = {1, 0, 0, 0, 0, 1};
        world.match(out, V::Element(solid_at, solid_at + 6), V::Element(empty_at, empty_at + 6));
        std::printf("match=%llu\n", hash_of(out));
        world.match(out, V::Element(solid_at, solid_at + 6), V::Element(empty_at, empty_at + 6), true);
        std::printf("match_walled=%llu\n", hash_of(out));
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 1;
    }
    return 0;
}
