// Exercises the distance field of the C++ host adapter (cpuvoxelraycaster_amd/host/hip_raycaster.hpp) at 64^3 on the scene
// of voxel_components_main.cpp (two boxes, a voxel at the corner of one, a speck): the stats, a few probes, a shell selected
// into a fresh volume, and the solid counts after dilate(2), then erode(2), then hollow(1) are printed, and the pytest
// wrapper compares the numbers with the numpy model's.
//   usage: voxel_distance_main <to_empty> <outside>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../cpuvoxelraycaster_amd/host/hip_raycaster.hpp"

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    const bool to_empty = atoi(argv[1]) != 0, outside = atoi(argv[2]) != 0;
    try {
        vrc_host::HipVoxelVolume vol(6);
        vol.fillBox(3, 4, 5, 13, 10, 9, true);           // 10 x 6 x 4
        vol.fillBox(30, 30, 30, 35, 33, 34, true);       // 5 x 3 x 4, across the tile border at 32
        vol.fillBox(35, 33, 34, 36, 34, 35, true);       // one voxel at its corner
        vol.setCell(vrc_host::Cell::Solid, vrc_host::Cell::Grass, 60, 1, 62);   // a speck, still in the queue when the transform starts
        vrc_host::HipVoxelDistance field = vol.distanceField(to_empty, outside);
        const vrc_distance_stats& s = field.stats();
        std::printf("features=%llu max_d2=%u argmax=%u,%u,%u reserved=%u depth=%u bytes=%llu data=%d\n", (unsigned long long)s.features, s.max_d2,
                    s.argmax[0], s.argmax[1], s.argmax[2], s.reserved, field.depth(), (unsigned long long)field.bytes(), field.data() != nullptr);
        const uint32_t xyz[15] = {3, 4, 5, 34, 32, 33, 0, 0, 0, 63, 63, 0, 64, 0, 0};
        const std::vector<uint32_t> d2 = field.at(xyz, 5);
        std::printf("at=%u,%u,%u,%u,%u\n", d2[0], d2[1], d2[2], d2[3], d2[4]);
        const std::vector<uint32_t> all = field.download();
        unsigned long long sum = 0;
        for (uint32_t v : all) sum += v == VRC_DISTANCE_NONE ? 0u : v;
        std::printf("voxels=%zu sum=%llu\n", all.size(), sum);
        vrc_host::HipVoxelVolume shell(6);
        field.select(1, 4, shell);
        std::printf("shell=%llu\n", (unsigned long long)shell.solidCount());

        const uint64_t before = vol.solidCount();
        vol.dilate(2);
        const uint64_t grown = vol.solidCount();
        vol.erode(2, outside);
        const uint64_t shrunk = vol.solidCount();
        vol.hollow(1);
        std::printf("before=%llu dilate=%llu erode=%llu hollow=%llu\n", (unsigned long long)before, (unsigned long long)grown, (unsigned long long)shrunk,
                    (unsigned long long)vol.solidCount());
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 1;
    }
    return 0;
}
