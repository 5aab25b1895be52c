// Exercises the merged-rectangle extraction of the C++ host adapter (cpuvoxelraycaster_amd/host/hip_raycaster.hpp) at 32^3:
// a sphere, a box and a carved slot; rectCount, surfaceRects, rectTriangles, a window, the triangles voxelised back into a
// new volume with xorMesh, and toObj with merged = true.  Prints one line of figures, then the records and the triangles
// as plain numbers; the pytest wrapper compares them and the OBJ file with the numpy model's.
//   usage: voxel_rects_main <depth> <out.obj>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../cpuvoxelraycaster_amd/host/hip_raycaster.hpp"

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    const uint32_t depth = (uint32_t)atoi(argv[1]);
    try {
        const uint32_t S = 1u << depth;
        vrc_host::HipVoxelVolume world(depth);
        std::vector<vrc_host::HipVoxelVolume::Sphere> balls(1);
        balls[0].x = (int32_t)S / 3; balls[0].y = (int32_t)S / 2; balls[0].z = (int32_t)S / 2; balls[0].radius = (int32_t)S / 4;
        world.fillSpheres(balls, true);
        world.fillBox(S / 2, 2, 0, S - 3, S / 3, S, true);              // touches two walls of the volume
        world.fillBox(S / 4, S / 2 - 1, 0, S / 2, S / 2 + 2, S, false);

        const std::vector<uint64_t> counts = world.rectCount();
        const std::vector<uint64_t> open_counts = world.rectCount(false);
        uint64_t total = 0, open_total = 0;
        for (int d = 0; d < 6; ++d) { total += counts[d]; open_total += open_counts[d]; }
        const std::vector<uint32_t> rects = world.surfaceRects();
        const std::vector<int32_t> tris = world.rectTriangles();
        const std::vector<uint32_t> window = world.surfaceRects(true, 5, 11);
        bool window_ok = window.size() == 44;
        for (size_t i = 0; window_ok && i < window.size(); ++i) window_ok = window[i] == rects[20 + i];

        vrc_host::HipVoxelVolume back(depth);
        back.xorMesh(tris);
        const uint32_t zero[3] = {0, 0, 0}, all[3] = {S, S, S};
        const int32_t at[3] = {0, 0, 0};
        std::unique_ptr<vrc_host::HipVoxelVolume> only_world = world.clone(), only_back = back.clone();
        only_world->copyRegion(back, zero, all, at, VRC_COPY_ANDNOT);
        only_back->copyRegion(world, zero, all, at, VRC_COPY_ANDNOT);
        const std::vector<uint32_t> whole = {0, 0, 0, S, S, S};
        const uint64_t differ = only_world->countBoxes(whole)[0] + only_back->countBoxes(whole)[0];

        const uint64_t written = world.toObj(argv[2], true, true);
        std::printf("solid=%llu back=%llu differ=%llu total=%llu open=%llu faces=%llu rects=%zu triangles=%zu window=%d obj_faces=%llu\n",
                    (unsigned long long)world.solidCount(), (unsigned long long)back.solidCount(), (unsigned long long)differ,
                    (unsigned long long)total, (unsigned long long)open_total, (unsigned long long)(world.surfaceFaces().size() / 4),
                    rects.size() / 4, tris.size() / 9, window_ok ? 1 : 0, (unsigned long long)written);
        std::printf("rects");
        for (size_t i = 0; i < rects.size(); ++i) std::printf(" %u", rects[i]);
        std::printf("\ntris");
        for (size_t i = 0; i < tris.size(); ++i) std::printf(" %d", tris[i]);
        std::printf("\n");
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 1;
    }
    return 0;
}
