// Exercises the sparse tile stream of the C++ host adapter (cpuvoxelraycaster_amd/host/hip_raycaster.hpp) at 64^3: a slab with
// a box on it and a sphere dug out of it is saved to the file named by argv[1] and loaded into a second volume.  FNV-1a hashes
// of both downloads and the info are printed; the pytest wrapper compares them and the file's bytes with Python's pack().
#include <cstdio>
#include <vector>

#include "../../cpuvoxelraycaster_amd/host/hip_raycaster.hpp"

static unsigned long long fnv1a(const void* p, size_t n)
{
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
    return h;
}

static unsigned long long hash_of(vrc_host::HipVoxelVolume& v)
{
    std::vector<uint8_t> solid((size_t)1 << (3u * v.depth()));
    vrc_host::check(vrc_volume_download(v.handle(), solid.data()), "vrc_volume_download");
    return fnv1a(solid.data(), solid.size());
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    try {
        vrc_host::HipVoxelVolume world(6);
        world.fillBox(0, 0, 0, 64, 30, 64, true);
        world.fillBox(20, 30, 20, 41, 37, 45, true);
        world.fillSpheres({{31, 29, 33, 9}}, false);
        const vrc_pack_info info = world.packInfo();
        std::printf("saved=%llu\n", hash_of(world));
        std::printf("info depth=%u tiles=%u mixed=%u full=%u partial=%u bytes=%llu solid=%llu\n", info.depth, info.tiles, info.mixed_tiles, info.full_tiles,
                    info.partial_bricks, (unsigned long long)info.bytes, (unsigned long long)info.solid);
        world.save(argv[1]);
        std::unique_ptr<vrc_host::HipVoxelVolume> other = vrc_host::HipVoxelVolume::load(argv[1]);
        std::printf("loaded=%llu depth=%u count=%llu\n", hash_of(*other), other->depth(), (unsigned long long)other->solidCount());
        const std::vector<uint8_t> again = other->pack();
        std::printf("stream=%llu size=%zu\n", fnv1a(again.data(), again.size()), again.size());
        // a stream that breaks a rule throws and leaves the volume as it was
        std::vector<uint8_t> bad = again;
        bad[32] ^= 1;                                          // the solid count
        try {
            other->unpack(bad);
            std::printf("refused=no\n");
        } catch (const std::exception& e) {
            std::printf("refused=%s\n", e.what());
        }
        std::printf("kept=%llu\n", hash_of(*other));
    } catch (const std::exception& e) {
        std::fprintf(stderr, "volume_pack_main: %s\n", e.what());
        return 1;
    }
    return 0;
}
