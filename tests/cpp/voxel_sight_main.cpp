// Exercises the sight methods of the C++ host adapter (cpuvoxelraycaster_amd/host/hip_raycaster.hpp) at 16^3: sight over the
// field to the solid, thin and supercover, striding and plain, for a ball of radius 1, and over a band with an upper end;
// visibleFrom whole and within a radius.  FNV-1a hashes of the records and of the downloads are printed with the stats, and
// the pytest wrapper compares them with tests/sight_model.py.
#include <cstdio>
#include <vector>

#include "../../cpuvoxelraycaster_amd/host/hip_raycaster.hpp"

typedef vrc_host::HipVoxelVolume V;

static unsigned long long fnv1a(const void* p, size_t n)
{
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
    return h;
}

template <class T>
static unsigned long long hash_of(const std::vector<T>& v) { return fnv1a(v.data(), v.size() * sizeof(T)); }

int main()
{
    try {
        const int S = 16;
        V world(4);
        world.fillBox(6, 0, 6, 8, 12, 8, true);          // a pillar
        world.fillBox(0, 10, 0, 16, 11, 5, true);        // a ledge
        world.fillBox(12, 3, 12, 13, 4, 13, true);       // a single voxel
        vrc_host::HipVoxelDistance field = world.distanceField();

        const int starts[4][3] = {{1, 1, 1}, {15, 15, 15}, {3, 14, 9}, {7, 5, 7}};
        std::vector<int32_t> segments;
        for (int s = 0; s < 4; ++s)
            for (int x = 0; x < S; ++x)
                for (int y = 0; y < S; ++y)
                    for (int z = 0; z < S; ++z)
                        if ((x + y + z) % 3 == 0) {
                            const int32_t seg[6] = {starts[s][0], starts[s][1], starts[s][2], x, y, z};
                            segments.insert(segments.end(), seg, seg + 6);
                        }
        const int32_t beyond[6] = {1, 1, 1, S, 0, 0};
        segments.insert(segments.end(), beyond, beyond + 6);
        const uint64_t n = segments.size() / 6;
        std::printf("segments=%llu\n", (unsigned long long)n);
        std::printf("thin=%llu\n", hash_of(field.sight(segments.data(), n)));
        std::printf("touch=%llu\n", hash_of(field.sight(segments.data(), n, 1u, VRC_DISTANCE_NONE, VRC_SIGHT_TOUCH)));
        std::printf("plain=%llu\n", hash_of(field.sight(segments.data(), n, 1u, VRC_DISTANCE_NONE, VRC_SIGHT_TOUCH | VRC_SIGHT_PLAIN)));
        std::printf("ball=%llu\n", hash_of(field.sight(segments.data(), n, 2u)));
        std::printf("band=%llu\n", hash_of(field.sight(segments.data(), n, 4u, 40u, VRC_SIGHT_TOUCH)));

        const uint32_t eye[3] = {3, 14, 9};
        vrc_host::HipVoxelDistance seen = field.visibleFrom(eye);
        const vrc_sight_stats& st = seen.sightStats();
        std::printf("seen=%llu visible=%llu max_d2=%u argmax=%u,%u,%u connectivity=%d\n", hash_of(seen.download()), (unsigned long long)st.visible, st.max_d2,
                    st.argmax[0], st.argmax[1], st.argmax[2], seen.connectivity());
        vrc_host::HipVoxelDistance near = field.visibleFrom(eye, 6u, 1u, VRC_DISTANCE_NONE, VRC_SIGHT_TOUCH);
        std::printf("near=%llu near_visible=%llu\n", hash_of(near.download()), (unsigned long long)near.sightStats().visible);
        V picked(4);
        seen.select(0u, VRC_DISTANCE_NONE - 1u, picked);
        std::printf("picked=%llu\n", (unsigned long long)picked.solidCount());
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "voxel_sight_main: %s\n", e.what());
        return 1;
    }
}
