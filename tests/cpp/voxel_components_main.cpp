// Exercises the connected components of the C++ host adapter (cpuvoxelraycaster_amd/host/hip_raycaster.hpp) at 64^3: two
// boxes and a speck are three pieces; their records, the piece under a few voxels, a select of one piece into a fresh volume
// and removeSmallPieces are printed, and the pytest wrapper compares the numbers with the numpy model's.
//   usage: voxel_components_main <connectivity>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../cpuvoxelraycaster_amd/host/hip_raycaster.hpp"

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    const int connectivity = atoi(argv[1]);
    try {
        vrc_host::HipVoxelVolume vol(6);
        vol.fillBox(3, 4, 5, 13, 10, 9, true);           // 10 x 6 x 4
        vol.fillBox(30, 30, 30, 35, 33, 34, true);       // 5 x 3 x 4, across the tile border at 32
        vol.fillBox(35, 33, 34, 36, 34, 35, true);       // one voxel at its corner: joined under 26 only
        vol.setCell(vrc_host::Cell::Solid, vrc_host::Cell::Grass, 60, 1, 62);   // a speck, still in the queue when the labelling starts
        vrc_host::HipVoxelLabels labels = vol.labelComponents(connectivity);
        const std::vector<vrc_component> records = labels.components();
        std::printf("count=%llu depth=%u bytes=%llu\n", (unsigned long long)labels.count(), labels.depth(), (unsigned long long)labels.bytes());
        for (const vrc_component& c : records)
            std::printf("record first=%u,%u,%u lo=%u,%u,%u hi=%u,%u,%u reserved=%u voxels=%llu\n", c.first[0], c.first[1], c.first[2], c.lo[0], c.lo[1],
                        c.lo[2], c.hi[0], c.hi[1], c.hi[2], c.reserved, (unsigned long long)c.voxels);
        const uint32_t xyz[15] = {3, 4, 5, 34, 32, 33, 35, 33, 34, 60, 1, 62, 0, 0, 0};
        const std::vector<uint32_t> ids = labels.at(xyz, 5);
        std::printf("at=%u,%u,%u,%u,%u\n", ids[0], ids[1], ids[2], ids[3], ids[4]);
        const std::vector<vrc_component> window = labels.components(1, 1);
        std::printf("window=%zu first=%u,%u,%u\n", window.size(), window[0].first[0], window[0].first[1], window[0].first[2]);

        std::vector<uint8_t> keep(labels.count(), 0);
        keep[1] = 1;
        vrc_host::HipVoxelVolume piece(6);
        labels.select(keep, piece);
        std::printf("piece=%llu\n", (unsigned long long)piece.solidCount());

        const uint64_t before = vol.solidCount();
        const uint64_t removed = vol.removeSmallPieces(2, connectivity);
        std::printf("before=%llu removed=%llu after=%llu\n", (unsigned long long)before, (unsigned long long)removed, (unsigned long long)vol.solidCount());
        vrc_host::HipVoxelLabels again = vol.labelComponents(connectivity);
        std::printf("again=%llu snapshot=%llu\n", (unsigned long long)again.count(), (unsigned long long)labels.count());
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 1;
    }
    return 0;
}
