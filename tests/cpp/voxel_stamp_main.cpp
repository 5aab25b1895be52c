// Exercises the affine stamp of the C++ host adapter (cpuvoxelraycaster_amd/host/hip_raycaster.hpp) at 64^3 on the scene of
// voxel_distance_main.cpp (two boxes, a voxel at the corner of one, a speck): a quarter turn into a second volume and its
// inverse back into a third, then the scene placed with a 30-degree turn about two axes at scale 1.5 in a 128^3 world.  The
// solid counts, a few probe voxels and the placement's map are printed, and the pytest wrapper compares them with the numpy
// model's.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../cpuvoxelraycaster_amd/host/hip_raycaster.hpp"

static void print_probes(const char* name, vrc_host::HipVoxelVolume& v, const std::vector<uint32_t>& xyz)
{
    const std::vector<uint8_t> solid = v.getVoxels(xyz);
    std::printf("%s=", name);
    for (uint8_t s : solid) std::printf("%u", (unsigned)s);
    std::printf("\n");
}

int main()
{
    try {
        vrc_host::HipVoxelVolume vol(6);
        vol.fillBox(3, 4, 5, 13, 10, 9, true);           // 10 x 6 x 4
        vol.fillBox(30, 30, 30, 35, 33, 34, true);       // 5 x 3 x 4
        vol.fillBox(35, 33, 34, 36, 34, 35, true);       // one voxel at its corner
        vol.setCell(vrc_host::Cell::Solid, vrc_host::Cell::Grass, 60, 1, 62);   // a speck, still in the queue when the stamp starts
        const std::vector<uint32_t> probes = {54, 12, 8, 58, 10, 6, 30, 35, 34, 62, 60, 62, 33, 28, 34, 1, 3, 62, 60, 1, 62, 0, 0, 0, 63, 63, 63, 32, 29, 33};

        // q = (p_y, S-1-p_x, p_z), the header's quarter turn, and its inverse q = (S-1-p_y, p_x, p_z)
        const vrc_affine turn = {{0, 65536, 0, -65536, 0, 0, 0, 0, 65536}, 0, {0, (int64_t)64 << 17, 0}};
        const vrc_affine back = {{0, -65536, 0, 65536, 0, 0, 0, 0, 65536}, 0, {(int64_t)64 << 17, 0, 0}};
        vrc_host::HipVoxelVolume turned(6), restored(6);
        turned.fillBox(0, 0, 0, 64, 64, 64, true);       // REPLACE overwrites all of it
        turned.stampAffine(vol, turn);
        restored.stampAffine(turned, back);
        std::printf("solid=%llu turned=%llu restored=%llu\n", (unsigned long long)vol.solidCount(), (unsigned long long)turned.solidCount(),
                    (unsigned long long)restored.solidCount());
        print_probes("turned_at", turned, probes);
        print_probes("restored_at", restored, probes);
        const uint32_t zero[3] = {0, 0, 0}, all[3] = {64, 64, 64};
        const int32_t at[3] = {0, 0, 0};
        restored.copyRegion(vol, zero, all, at, VRC_COPY_ANDNOT);
        std::printf("difference=%llu\n", (unsigned long long)restored.solidCount());

        float rx[9], ry[9], rot[9];
        vrc_make_rotation(0.5235988f, 0.0f, rx);
        vrc_make_rotation(0.0f, 0.5235988f, ry);
        for (int c = 0; c < 3; ++c)
            for (int r = 0; r < 3; ++r) rot[3 * c + r] = (ry[r] * rx[3 * c] + ry[3 + r] * rx[3 * c + 1]) + ry[6 + r] * rx[3 * c + 2];
        vrc_host::HipVoxelVolume world(7);
        world.fillBox(60, 60, 0, 68, 68, 128, true);     // a pillar the paste is ORed onto
        const vrc_affine map = world.stampPlaced(vol, rot, 1.5f);
        std::printf("map=%d,%d,%d,%d,%d,%d,%d,%d,%d reserved=%d t=%lld,%lld,%lld\n", map.m[0], map.m[1], map.m[2], map.m[3], map.m[4], map.m[5], map.m[6],
                    map.m[7], map.m[8], map.reserved, (long long)map.t[0], (long long)map.t[1], (long long)map.t[2]);
        std::printf("rot=%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g\n", rot[0], rot[1], rot[2], rot[3], rot[4], rot[5], rot[6], rot[7], rot[8]);
        std::printf("world=%llu\n", (unsigned long long)world.solidCount());
        const std::vector<uint32_t> far = {64, 64, 64, 60, 60, 0, 49, 5, 36, 64, 66, 62, 51, 7, 40, 100, 64, 64, 64, 20, 64, 64, 64, 110, 40, 40, 40, 127, 127, 127};
        print_probes("world_at", world, far);
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 1;
    }
    return 0;
}
