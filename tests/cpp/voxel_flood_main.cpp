// Exercises the flood of the C++ host adapter (cpuvoxelraycaster_amd/host/hip_raycaster.hpp) the way an editor's "dig, then
// let the loose pieces fall" would: rays are cast on the terrain, a sphere is dug at every hit, keepConnected() anchored on
// the terrain's bottom slab splits the volume into what still holds on to it and the debris, commit() builds the scene of
// what is left and HipRayCaster::setScene shows it.  Also floods the air from the slab opposite.  Prints counts and a hash of
// the frame; the pytest wrapper compares them with the same sequence through VoxelVolume and with the numpy model.
//   usage: voxel_flood_main <depth> <rays.bin: n x {org xyz, dir xyz} float32> <W> <H> <dig radius> <connectivity>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "../../cpuvoxelraycaster_amd/host/hip_raycaster.hpp"

int main(int argc, char** argv)
{
    if (argc != 7) return 2;
    const uint32_t depth = (uint32_t)atoi(argv[1]);
    std::ifstream f(argv[2], std::ios::binary);
    const std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const float* rays = (const float*)raw.data();
    const size_t n_rays = raw.size() / 24;
    const uint32_t W = (uint32_t)atoi(argv[3]), H = (uint32_t)atoi(argv[4]);
    const int32_t dig = atoi(argv[5]);
    const int connectivity = atoi(argv[6]);
    try {
        std::unique_ptr<vrc_host::HipLSVO> before = vrc_host::HipLSVO::fromFastNoiseTerrain(1337, depth);
        std::vector<vrc_host::Vec3> org(n_rays), dir(n_rays);
        for (size_t i = 0; i < n_rays; ++i) {
            org[i] = {rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]};
            dir[i] = {rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]};
        }
        const std::vector<vrc_hit> hits = before->castRaysRecords(org, dir);
        std::unique_ptr<vrc_host::HipVoxelVolume> vol = vrc_host::HipVoxelVolume::fromScene(*before);
        vol->fillSpheresAtHits(hits, dig, false);
        const uint32_t S = 1u << depth;
        vol->fillBox(20, S / 2 - 5, 20, 23, S / 2 - 2, 23, true);      // a block in the empty half: debris whatever the digs detach
        const uint64_t solid_dug = vol->solidCount();

        // the air above the dug terrain, from the slab y = S - 1 of the volume (a flood through the EMPTY voxels)
        vrc_host::HipVoxelVolume air(depth);
        air.fillBox(0, S - 1, 0, S, S, S, true);
        const vrc_flood_stats air_stats = air.flood(*vol, connectivity, true);

        // the terrain's columns stand on the plane y = S / 2 + 1 (main.cpp:65-74)
        std::unique_ptr<vrc_host::HipVoxelVolume> debris = vol->keepConnected({0, S / 2 + 1, 0, S, S / 2 + 2, S}, connectivity);
        const uint64_t supported = vol->solidCount(), loose = debris->solidCount();
        std::unique_ptr<vrc_host::HipLSVO> after = vol->commit();

        const float size = (float)S;
        vrc_host::CameraState cam;
        cam.position = {size / 2, size / 2 - 56.0f, size / 2};
        cam.view_angle = {0.0f, -0.5f};
        vrc_host::HipRayCaster rc(*before, W, H);
        rc.setLightPosition({-200.0f / 512.0f + 1.0f, -1000.0f / 512.0f + 1.0f, -300.0f / 512.0f + 1.0f});
        rc.use_gi = true; rc.use_samples = true;
        rc.setScene(*after);
        before.reset();
        rc.renderFrame(cam, -1, 2);
        rc.samples_to_image();
        const std::vector<uint8_t> image = rc.render_image();
        uint64_t hash = 1469598103934665603ull;          // FNV-1a
        for (uint8_t b : image) hash = (hash ^ b) * 1099511628211ull;
        std::printf("rays=%zu solid_dug=%llu air=%llu air_converged=%u supported=%llu debris=%llu nodes_after=%llu image_hash=%016llx\n", n_rays,
                    (unsigned long long)solid_dug, (unsigned long long)air_stats.reached, air_stats.converged, (unsigned long long)supported,
                    (unsigned long long)loose, (unsigned long long)vrc_scene_node_count(after->handle()), (unsigned long long)hash);
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 1;
    }
    return 0;
}
