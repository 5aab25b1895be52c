// Exercises the write half of the C++ host adapter (cpuvoxelraycaster_amd/host/hip_raycaster.hpp) the way a host with
// an "edit the world" key would: a terrain generated on the device is made editable (HipVoxelVolume::fromScene), a list of
// setCell calls is applied, commit() builds the new scene and HipRayCaster::setScene shows it on the renderer that has
// already rendered the old one.  Writes the second frame's image; the pytest wrapper compares it with the Python path's.
//   usage: voxel_volume_main <depth> <edits.bin: n x {x, y, z, solid} uint32> <top.bmp> <side.bmp> <W> <H> <out.rgba>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "../../cpuvoxelraycaster_amd/host/hip_raycaster.hpp"

int main(int argc, char** argv)
{
    if (argc != 8) return 2;
    const uint32_t depth = (uint32_t)atoi(argv[1]);
    std::ifstream f(argv[2], std::ios::binary);
    const std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const uint32_t* edits = (const uint32_t*)raw.data();
    const size_t n_edits = raw.size() / 16;
    const uint32_t W = (uint32_t)atoi(argv[5]), H = (uint32_t)atoi(argv[6]);
    try {
        std::unique_ptr<vrc_host::HipLSVO> before = vrc_host::HipLSVO::fromFastNoiseTerrain(1337, depth);
        before->loadTextures(argv[3], argv[4]);
        const float size = (float)(1u << depth);
        vrc_host::CameraState cam;
        cam.position = {size / 2, size / 2 - 56.0f, size / 2};
        cam.view_angle = {0.0f, -0.5f};
        vrc_host::HipRayCaster rc(*before, W, H);
        rc.setLightPosition({-200.0f / 512.0f + 1.0f, -1000.0f / 512.0f + 1.0f, -300.0f / 512.0f + 1.0f});
        rc.use_gi = true; rc.use_samples = true;
        rc.renderFrame(cam, -1, 2);
        rc.samples_to_image();
        const std::vector<uint8_t> first = rc.render_image();
        rc.resetSamples();

        std::unique_ptr<vrc_host::HipVoxelVolume> vol = vrc_host::HipVoxelVolume::fromScene(*before);
        const uint64_t solid_before = vol->solidCount();
        for (size_t i = 0; i < n_edits; ++i)
            vol->setCell(edits[4 * i + 3] ? vrc_host::Cell::Solid : vrc_host::Cell::Empty, vrc_host::Cell::Grass,
                         edits[4 * i], edits[4 * i + 1], edits[4 * i + 2]);
        float build_ms = 0.0f;
        std::unique_ptr<vrc_host::HipLSVO> after = vol->commit(&build_ms);
        rc.setScene(*after);
        before.reset();                       // no frame uses the old scene any more
        rc.setFrameIndex(0);
        rc.renderFrame(cam, -1, 2);
        rc.samples_to_image();
        const std::vector<uint8_t> second = rc.render_image();
        std::ofstream out(argv[7], std::ios::binary);
        out.write((const char*)second.data(), (std::streamsize)second.size());
        std::printf("edits=%zu solid_before=%llu solid_after=%llu nodes_after=%llu changed=%d build_ms_positive=%d\n", n_edits,
                    (unsigned long long)solid_before, (unsigned long long)vol->solidCount(),
                    (unsigned long long)vrc_scene_node_count(after->handle()), first != second ? 1 : 0, build_ms > 0.0f ? 1 : 0);
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 1;
    }
    return 0;
}
