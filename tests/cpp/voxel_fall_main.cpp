// Exercises the falling pieces of the C++ host adapter (cpuvoxelraycaster_amd/host/hip_raycaster.hpp) at 16^3: a slab with a
// ledge, three loose boxes and a speck fall towards -y; the offsets, the stats and the voxel count of the placed volume are
// printed, then dropLoose does the same on the world itself, and the pytest wrapper compares the numbers with the numpy
// model's.
//   usage: voxel_fall_main <connectivity> <drop_limit>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../cpuvoxelraycaster_amd/host/hip_raycaster.hpp"

static void scene(vrc_host::HipVoxelVolume& vol, bool fixed, bool loose)
{
    if (fixed) {
        vol.fillBox(0, 0, 0, 16, 2, 16, true);           // the slab
        vol.fillBox(2, 2, 2, 5, 6, 5, true);             // a ledge on it
    }
    if (loose) {
        vol.fillBox(1, 9, 1, 7, 11, 7, true);            // lands on the ledge
        vol.fillBox(3, 13, 3, 5, 14, 5, true);           // lands on the box below
        vol.fillBox(9, 5, 9, 12, 8, 15, true);           // lands on the slab
        vol.setCell(vrc_host::Cell::Solid, vrc_host::Cell::Grass, 10, 12, 10);   // a speck above it, still in the queue
    }
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    const int connectivity = atoi(argv[1]);
    const uint32_t limit = (uint32_t)atoi(argv[2]);
    try {
        vrc_host::HipVoxelVolume fixed(4), debris(4), world(4);
        scene(fixed, true, false);
        scene(debris, false, true);
        scene(world, true, true);
        vrc_host::HipVoxelLabels labels = debris.labelComponents(connectivity);
        vrc_fall_stats st;
        const std::vector<int32_t> offsets = labels.fall(&fixed, VRC_FACE_YN, limit, &st);
        std::printf("count=%llu\n", (unsigned long long)labels.count());
        for (size_t i = 0; i < offsets.size(); i += 3) std::printf("offset=%d,%d,%d\n", offsets[i], offsets[i + 1], offsets[i + 2]);
        std::printf("stats moved_voxels=%llu pieces=%u moved_pieces=%u max_drop=%u reserved=%u,%u\n", (unsigned long long)st.moved_voxels, st.pieces,
                    st.moved_pieces, st.max_drop, st.reserved[0], st.reserved[1]);
        std::printf("rounds=%u\n", st.rounds);
        labels.place(offsets, fixed, VRC_COPY_OR);
        std::printf("placed=%llu\n", (unsigned long long)fixed.solidCount());
        std::vector<uint8_t> keep(labels.count(), 0);
        keep[0] = 1;
        labels.place(offsets, fixed, VRC_COPY_ANDNOT, &keep);
        std::printf("without_first=%llu\n", (unsigned long long)fixed.solidCount());

        const uint32_t anchor[6] = {0, 0, 0, 16, 1, 16};
        const uint64_t before = world.solidCount();
        const vrc_fall_stats dropped = world.dropLoose(anchor, 1, VRC_FACE_YN, connectivity, limit);
        std::printf("dropped moved_voxels=%llu pieces=%u moved_pieces=%u max_drop=%u before=%llu after=%llu\n", (unsigned long long)dropped.moved_voxels,
                    dropped.pieces, dropped.moved_pieces, dropped.max_drop, (unsigned long long)before, (unsigned long long)world.solidCount());
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 1;
    }
    return 0;
}
