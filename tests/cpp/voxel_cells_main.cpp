// Exercises the cell methods of the C++ host adapter (cpuvoxelraycaster_amd/host/hip_raycaster.hpp) at 32^3: the seeded
// fill whole and in a box, one step with both neighbourhoods and its count, the automaton to a fixed point, smooth,
// removeSpecks and caves.  FNV-1a hashes of the downloads are printed, and the pytest wrapper compares them with the numpy
// model's.
#include <cstdio>
#include <vector>

#include "../../cpuvoxelraycaster_amd/host/hip_raycaster.hpp"

static unsigned long long fnv1a(const void* p, size_t n)
{
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
    return h;
}

static unsigned long long hash_of(vrc_host::HipVoxelVolume& v)
{
    std::vector<uint8_t> solid((size_t)1 << (3u * v.depth()));
    vrc_host::check(vrc_volume_download(v.handle(), solid.data()), "vrc_volume_download");
    return fnv1a(solid.data(), solid.size());
}

int main()
{
    try {
        vrc_host::HipVoxelVolume world(5), next(5);
        world.fillRandom(7, 0.45);
        std::printf("filled=%llu\n", hash_of(world));
        const uint32_t box[6] = {3, 5, 7, 30, 21, 18};
        world.fillRandom(11, 0.5, box, VRC_COPY_ANDNOT);
        std::printf("boxed=%llu\n", hash_of(world));

        uint64_t changed = 0;
        next.fillBox(0, 0, 0, 32, 32, 32, true);                   // whatever dst holds is overwritten
        world.cellStep(next, 0x1E0u, 0x7FF0u, VRC_CELLS_ALL, true, &changed);
        std::printf("all=%llu changed_all=%llu\n", hash_of(next), (unsigned long long)changed);
        world.cellStep(next, 1u << 3, 0x7Cu, VRC_CELLS_FACES, false, &changed);
        std::printf("faces=%llu changed_faces=%llu source=%llu\n", hash_of(next), (unsigned long long)changed, hash_of(world));
        world.cellStep(next, 1u << 3, 0x7Cu, VRC_CELLS_FACES);     // asynchronous, no count
        std::printf("async=%llu\n", hash_of(next));

        const uint32_t taken = world.automaton(3, 0x7FFC000u, 0x7FFE000u, VRC_CELLS_ALL, false);
        std::printf("taken=%u automaton=%llu\n", taken, hash_of(world));
        const uint32_t all = world.automaton(100, 0x7FFC000u, 0x7FFE000u, VRC_CELLS_ALL, false);
        std::printf("to_fixed=%u fixed=%llu\n", all, hash_of(world));

        vrc_host::HipVoxelVolume dust(5);
        dust.fillRandom(3, 0.1);
        dust.removeSpecks();
        std::printf("specks=%llu\n", hash_of(dust));
        dust.fillRandom(5, 0.5, nullptr, VRC_COPY_REPLACE);
        dust.smooth(2, true);
        std::printf("smooth=%llu\n", hash_of(dust));
        dust.caves(1337, 0.48, 4);
        std::printf("caves=%llu\n", hash_of(dust));
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 1;
    }
    return 0;
}
