// Exercises the rigid-piece mirrors of the C++ host adapter (cpuvoxelraycaster_amd/host/hip_raycaster.hpp) at 16^3: three loose
// pieces; their moments and mass properties are printed, every piece is turned a quarter turn about z about its own centre of
// mass and moved by (1, -2, 0) into an empty volume, then taken out again with a keep mask; the pytest wrapper compares the
// numbers with the numpy model's.
#include <cstdio>
#include <vector>

#include "../../cpuvoxelraycaster_amd/host/hip_raycaster.hpp"

int main()
{
    try {
        vrc_host::HipVoxelVolume debris(4), world(4);
        debris.fillBox(1, 9, 1, 7, 11, 6, true);
        debris.fillBox(9, 5, 9, 12, 8, 15, true);
        debris.fillBox(10, 8, 9, 11, 12, 10, true);          // an arm on the second box
        debris.setCell(vrc_host::Cell::Solid, vrc_host::Cell::Grass, 3, 13, 3);   // a speck, still in the queue
        vrc_host::HipVoxelLabels labels = debris.labelComponents(6);
        std::printf("count=%llu\n", (unsigned long long)labels.count());
        const std::vector<vrc_piece_moments> mo = labels.moments();
        for (const vrc_piece_moments& m : mo)
            std::printf("moments=%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu\n", (unsigned long long)m.voxels, (unsigned long long)m.s1[0],
                        (unsigned long long)m.s1[1], (unsigned long long)m.s1[2], (unsigned long long)m.s2[0], (unsigned long long)m.s2[1],
                        (unsigned long long)m.s2[2], (unsigned long long)m.s2[3], (unsigned long long)m.s2[4], (unsigned long long)m.s2[5]);
        std::printf("window=%zu\n", labels.moments(1, 5).size());
        const std::vector<vrc_host::HipMassProperties> mp = labels.massProperties();
        std::vector<float> target;
        for (const vrc_host::HipMassProperties& p : mp) {
            std::printf("mass=%.17g centre=%.17g,%.17g,%.17g ixx=%.17g ixy=%.17g\n", p.mass, p.centre[0], p.centre[1], p.centre[2], p.inertia[0], p.inertia[1]);
            target.push_back((float)p.centre[0] + 1.0f);
            target.push_back((float)p.centre[1] - 2.0f);
            target.push_back((float)p.centre[2]);
        }
        const float quarter[9] = {0, 1, 0, -1, 0, 0, 0, 0, 1};   // +90 degrees about z, vrc_make_rotation's layout (columns)
        std::vector<uint32_t> boxes;
        const std::vector<vrc_affine> maps = labels.poses(quarter, target, world.depth(), boxes);
        for (size_t i = 0; i < maps.size(); ++i)
            std::printf("map=%d,%d,%d,%d,%d,%d,%d,%d,%d t=%lld,%lld,%lld box=%u,%u,%u,%u,%u,%u\n", maps[i].m[0], maps[i].m[1], maps[i].m[2], maps[i].m[3], maps[i].m[4],
                        maps[i].m[5], maps[i].m[6], maps[i].m[7], maps[i].m[8], (long long)maps[i].t[0], (long long)maps[i].t[1], (long long)maps[i].t[2],
                        boxes[6 * i], boxes[6 * i + 1], boxes[6 * i + 2], boxes[6 * i + 3], boxes[6 * i + 4], boxes[6 * i + 5]);
        labels.placeAffine(maps, world, VRC_COPY_OR, &boxes);
        std::printf("placed=%llu\n", (unsigned long long)world.solidCount());
        std::vector<uint8_t> keep(labels.count(), 0);
        keep[0] = 1;
        labels.placeAffine(maps, world, VRC_COPY_ANDNOT, nullptr, &keep);
        std::printf("without_first=%llu\n", (unsigned long long)world.solidCount());
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 1;
    }
    return 0;
}
