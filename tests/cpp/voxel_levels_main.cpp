// Exercises the methods between depths of the C++ host adapter (cpuvoxelraycaster_amd/host/hip_raycaster.hpp) on a seeded
// field of 32^3: the counts of every level, the three named reductions, a band with an op over what the destination holds,
// expand into a larger volume and back.  FNV-1a hashes of the downloads and of the counts are printed, and the pytest wrapper
// compares them with the numpy model's.
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
    using Volume = vrc_host::HipVoxelVolume;
    try {
        Volume world(5);
        world.fillRandom(7, 0.5);
        std::printf("filled=%llu\n", hash_of(world));
        for (uint32_t k = 1; k <= 5; ++k) {
            const std::vector<uint32_t> counts = world.cellCounts(k);
            unsigned long long sum = 0;
            for (uint32_t c : counts) sum += c;
            std::printf("cells%u=%zu counts%u=%llu sum%u=%llu\n", k, counts.size(), k, fnv1a(counts.data(), counts.size() * 4u), k, sum);
        }
        std::printf("any4=%llu all4=%llu\n", hash_of(*world.reduced(4)), hash_of(*world.reduced(4, Volume::LevelRule::All)));
        std::printf("half4=%llu half3=%llu half2=%llu\n", hash_of(*world.reduced(4, Volume::LevelRule::Majority)),
                    hash_of(*world.reduced(3, Volume::LevelRule::Majority)), hash_of(*world.reduced(2, Volume::LevelRule::Majority)));

        Volume coarse(3);
        coarse.fillRandom(5, 0.5);
        uint32_t lo = 0, hi = 0;
        Volume::countRange(Volume::LevelRule::Majority, 2, &lo, &hi);
        world.reduceInto(coarse, lo + 2u, hi, VRC_COPY_ANDNOT);
        std::printf("lo=%u hi=%u band=%llu source=%llu\n", lo, hi, hash_of(coarse), hash_of(world));

        std::unique_ptr<Volume> blown = coarse.expanded(6);
        std::printf("expanded=%llu\n", hash_of(*blown));
        coarse.expandInto(world, VRC_COPY_OR);
        std::printf("merged=%llu\n", hash_of(world));
        std::printf("back=%llu\n", hash_of(*blown->reduced(3, Volume::LevelRule::All)));
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 1;
    }
    return 0;
}
