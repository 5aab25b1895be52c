// Exercises the deltas of the C++ host adapter (cpuvoxelraycaster_amd/host/hip_raycaster.hpp) at 64^3: a slab with a box on
// it, a sphere dug out of it, the diff of the two, the diff applied onto a clone of the first, and HipVoxelHistory through
// record, undo and redo.  FNV-1a hashes of the downloads and of the records are printed, and the pytest wrapper compares them
// with the numpy model's.
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

int main()
{
    try {
        vrc_host::HipVoxelVolume world(6);
        world.fillBox(0, 0, 0, 64, 30, 64, true);
        world.fillBox(20, 30, 20, 41, 37, 45, true);
        std::unique_ptr<vrc_host::HipVoxelVolume> before = world.clone();
        std::printf("before=%llu\n", hash_of(world));
        world.fillSpheres({{31, 29, 33, 9}}, false);
        std::printf("after=%llu\n", hash_of(world));

        vrc_host::HipVoxelDelta delta = before->diff(world);
        const vrc_delta_stats s = delta.stats();
        std::printf("stats words=%llu voxels=%llu lo=%u,%u,%u hi=%u,%u,%u reserved=%u,%u\n", (unsigned long long)s.words, (unsigned long long)s.voxels, s.lo[0],
                    s.lo[1], s.lo[2], s.hi[0], s.hi[1], s.hi[2], s.reserved[0], s.reserved[1]);
        const std::vector<uint32_t> records = delta.records();
        std::printf("count=%llu depth=%u bytes=%llu records=%llu\n", (unsigned long long)delta.count(), delta.depth(), (unsigned long long)delta.bytes(),
                    fnv1a(records.data(), records.size() * 4u));
        const std::vector<uint32_t> window = delta.records(3, 5);
        std::printf("window=%zu %s\n", window.size() / 2, std::equal(window.begin(), window.end(), records.begin() + 6) ? "same" : "different");

        before->applyDelta(delta);
        std::printf("applied=%llu\n", hash_of(*before));
        before->applyDelta(delta);
        std::printf("again=%llu\n", hash_of(*before));
        vrc_host::HipVoxelDelta copy = vrc_host::HipVoxelDelta::fromRecords(6, records);
        before->applyDelta(copy);
        std::printf("copy=%llu voxels=%llu\n", hash_of(*before), (unsigned long long)copy.stats().voxels);

        vrc_host::HipVoxelHistory history(world);
        std::printf("idle=%d\n", history.record() ? 1 : 0);
        world.fillBox(5, 40, 5, 9, 44, 9, true);
        const vrc_host::HipVoxelDelta* step = history.record();
        std::printf("step=%llu built=%llu\n", (unsigned long long)step->stats().voxels, hash_of(world));
        step = history.undo();
        std::printf("undo=%llu undone=%llu stacks=%zu,%zu\n", (unsigned long long)step->count(), hash_of(world), history.undoCount(), history.redoCount());
        step = history.redo();
        std::printf("redo=%llu redone=%llu stacks=%zu,%zu bytes=%llu\n", (unsigned long long)step->count(), hash_of(world), history.undoCount(), history.redoCount(),
                    (unsigned long long)history.bytes());
        std::printf("nothing=%d\n", history.redo() ? 1 : 0);
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 1;
    }
    return 0;
}
