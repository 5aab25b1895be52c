// Exercises HipVoxelVolume::fracture and HipVoxelLabels::pieceSites of the C++ host adapter
// (cpuvoxelraycaster_amd/host/hip_raycaster.hpp) at 64^3: a wall on a slab, broken round five sites within 12 voxels, one
// of the sites outside the volume and two of them equal; then the same sites without a limit.  The pytest wrapper compares the
// printed records and cells with the numpy model's.
#include <cstdio>
#include <vector>

#include "../../cpuvoxelraycaster_amd/host/hip_raycaster.hpp"

static void print(const char* tag, vrc_host::HipVoxelLabels& labels)
{
    const std::vector<vrc_component> records = labels.components();
    const std::vector<uint32_t> cells = labels.pieceSites();
    std::printf("%s_count=%llu,%llu\n", tag, (unsigned long long)labels.count(), (unsigned long long)labels.bytes());
    for (size_t i = 0; i < records.size(); ++i) {
        const vrc_component& c = records[i];
        std::printf("%s=%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%llu,%u\n", tag, c.first[0], c.first[1], c.first[2], c.lo[0], c.lo[1], c.lo[2], c.hi[0], c.hi[1], c.hi[2],
                    c.reserved, (unsigned long long)c.voxels, cells[i]);
    }
    const std::vector<uint32_t> window = labels.pieceSites(1, 2);
    std::printf("%s_window=%llu\n", tag, (unsigned long long)window.size());
}

int main()
{
    try {
        vrc_host::HipVoxelVolume world(6);
        world.fillBox(0, 0, 0, 64, 3, 64, true);              // the slab
        world.fillBox(10, 3, 28, 54, 40, 33, true);           // the wall
        const std::vector<int32_t> sites = {30, 20, 30, 36, 25, 31, -4, 20, 30, 30, 20, 30, 33, 14, 29};
        vrc_host::HipVoxelLabels near = world.fracture(sites, 6, false, 12);
        print("near", near);
        vrc_host::HipVoxelLabels all = world.fracture(sites, 26);
        print("all", all);
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 1;
    }
    return 0;
}
