// Exercises the travel-distance field of the C++ host adapter (cpuvoxelraycaster_amd/host/hip_raycaster.hpp) at 16^3: a solid
// L-shaped corridor with a side room and a speck that nothing reaches, seeded at the corridor's start.  The stats, a few
// probes, the voxels within 5 steps selected into a fresh volume and one traced route are printed, and the pytest wrapper
// compares the numbers with the breadth-first model's.
//   usage: voxel_travel_main <connectivity>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../cpuvoxelraycaster_amd/host/hip_raycaster.hpp"

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    const int connectivity = atoi(argv[1]);
    try {
        vrc_host::HipVoxelVolume vol(4), seeds(4);
        vol.fillBox(1, 1, 1, 14, 2, 2, true);            // along x
        vol.fillBox(13, 1, 1, 14, 12, 2, true);          // then along y
        vol.fillBox(5, 2, 1, 8, 5, 3, true);             // a room at the corridor's side, 3 x 3 x 2
        vol.setCell(vrc_host::Cell::Solid, vrc_host::Cell::Grass, 13, 12, 1);   // the last voxel, still in the queue when the field starts
        vol.fillBox(2, 10, 10, 3, 11, 11, true);         // a speck nothing reaches
        seeds.setCell(vrc_host::Cell::Solid, vrc_host::Cell::Grass, 1, 1, 1);
        seeds.setCell(vrc_host::Cell::Solid, vrc_host::Cell::Grass, 0, 0, 0);    // a seed outside M: dropped
        vrc_host::HipVoxelDistance field = vol.travelField(seeds, connectivity);
        const vrc_travel_stats& s = field.travelStats();
        std::printf("seeds=%llu reached=%llu max_steps=%u argmax=%u,%u,%u sweeps=%u reserved=%u depth=%u bytes=%llu connectivity=%d\n",
                    (unsigned long long)s.seeds, (unsigned long long)s.reached, s.max_steps, s.argmax[0], s.argmax[1], s.argmax[2], s.sweeps, s.reserved,
                    field.depth(), (unsigned long long)field.bytes(), field.connectivity());
        const uint32_t xyz[15] = {1, 1, 1, 13, 12, 1, 7, 4, 2, 2, 10, 10, 16, 0, 0};
        const std::vector<uint32_t> at = field.at(xyz, 5);
        std::printf("at=%u,%u,%u,%u,%u\n", at[0], at[1], at[2], at[3], at[4]);
        vrc_host::HipVoxelVolume near(4);
        field.select(0, 5, near);
        std::printf("near=%llu\n", (unsigned long long)near.solidCount());
        const uint32_t starts[9] = {13, 12, 1, 2, 10, 10, 7, 4, 2};
        std::vector<uint32_t> paths, lengths;
        field.tracePaths(starts, 3, 32, paths, lengths, 77u);
        std::printf("lengths=%u,%u,%u\nroute=", lengths[0], lengths[1], lengths[2]);
        for (uint32_t k = 0; k <= lengths[0] && k < 32u; ++k) std::printf("%u,%u,%u;", paths[3 * k], paths[3 * k + 1], paths[3 * k + 2]);
        unsigned untouched = 0;
        for (uint32_t k = 0; k < 32u * 3u; ++k) untouched += paths[32u * 3u + k] == 77u;
        std::printf("\nuntouched=%u\n", untouched);
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 1;
    }
    return 0;
}
