// Exercises the brushes of the C++ host adapter (cpuvoxelraycaster_amd/host/hip_raycaster.hpp) the way a host with a
// "spray" tool would: a batch of rays is cast on the terrain, a sphere is dug at every hit and a smaller one built in front
// of every hit (HipVoxelVolume::fillSpheresAtHits), commit() builds the new scene, HipRayCaster::setScene shows it.  Prints
// a hash of the frame on the new scene; the pytest wrapper compares it with the same sequence through VoxelVolume.
//   usage: voxel_brushes_main <depth> <rays.bin: n x {org xyz, dir xyz} float32> <top.bmp> <side.bmp> <W> <H> <dig radius> <build radius>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "../../cpuvoxelraycaster_amd/host/hip_raycaster.hpp"

int main(int argc, char** argv)
{
    if (argc != 9) return 2;
    const uint32_t depth = (uint32_t)atoi(argv[1]);
    std::ifstream f(argv[2], std::ios::binary);
    const std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const float* rays = (const float*)raw.data();
    const size_t n_rays = raw.size() / 24;
    const uint32_t W = (uint32_t)atoi(argv[5]), H = (uint32_t)atoi(argv[6]);
    const int32_t dig = atoi(argv[7]), build = atoi(argv[8]);
    try {
        std::unique_ptr<vrc_host::HipLSVO> before = vrc_host::HipLSVO::fromFastNoiseTerrain(1337, depth);
        before->loadTextures(argv[3], argv[4]);
        std::vector<vrc_host::Vec3> org(n_rays), dir(n_rays);
        for (size_t i = 0; i < n_rays; ++i) {
            org[i] = {rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]};
            dir[i] = {rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]};
        }
        const std::vector<vrc_hit> hits = before->castRaysRecords(org, dir);
        size_t unit_hits = 0;
        for (const vrc_hit& h : hits) unit_hits += (h.hit & 0xffu) == 1u;

        std::unique_ptr<vrc_host::HipVoxelVolume> vol = vrc_host::HipVoxelVolume::fromScene(*before);
        const uint64_t solid_before = vol->solidCount();
        vol->fillSpheresAtHits(hits, dig, false);
        const uint64_t solid_dug = vol->solidCount();
        vol->fillSpheresAtHits(hits, build, true);
        std::unique_ptr<vrc_host::HipLSVO> after = vol->commit();

        const float size = (float)(1u << depth);
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
        std::printf("rays=%zu unit_hits=%zu solid_before=%llu solid_dug=%llu solid_after=%llu nodes_after=%llu image_hash=%016llx\n", n_rays, unit_hits,
                    (unsigned long long)solid_before, (unsigned long long)solid_dug, (unsigned long long)vol->solidCount(),
                    (unsigned long long)vrc_scene_node_count(after->handle()), (unsigned long long)hash);
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 1;
    }
    return 0;
}
