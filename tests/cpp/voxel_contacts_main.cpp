// Exercises HipVoxelLabels::contacts of the C++ host adapter (cpuvoxelraycaster_amd/host/hip_raycaster.hpp) at 16^3: the three
// loose pieces of the rigid test over a slab two voxels thick.  The first box is lowered until it rests on the slab, the second
// one cell into it, the speck (piece 1) stays in the open; then the same with a keep mask that drops the second box.  The pytest wrapper
// compares the printed records with the numpy model's.
#include <cstdio>
#include <vector>

#include "../../cpuvoxelraycaster_amd/host/hip_raycaster.hpp"

static void print(const char* tag, const std::vector<vrc_piece_contact>& records)
{
    for (const vrc_piece_contact& c : records)
        std::printf("%s=%llu,%llu,%llu,%llu,%llu,%lld,%lld,%lld,%llu,%llu,%llu,%llu,%lld,%lld,%lld,%llu\n", tag, (unsigned long long)c.posed,
                    (unsigned long long)c.overlap, (unsigned long long)c.overlap_s1[0], (unsigned long long)c.overlap_s1[1], (unsigned long long)c.overlap_s1[2],
                    (long long)c.overlap_n[0], (long long)c.overlap_n[1], (long long)c.overlap_n[2], (unsigned long long)c.touch, (unsigned long long)c.touch_s1[0],
                    (unsigned long long)c.touch_s1[1], (unsigned long long)c.touch_s1[2], (long long)c.touch_n[0], (long long)c.touch_n[1], (long long)c.touch_n[2],
                    (unsigned long long)c.reserved);
}

int main()
{
    try {
        vrc_host::HipVoxelVolume debris(4), world(4);
        debris.fillBox(1, 9, 1, 7, 11, 6, true);
        debris.fillBox(9, 5, 9, 12, 8, 15, true);
        debris.fillBox(10, 8, 9, 11, 12, 10, true);          // an arm on the second box
        debris.setCell(vrc_host::Cell::Solid, vrc_host::Cell::Grass, 3, 13, 3);   // a speck, still in the queue
        world.fillBox(0, 0, 0, 16, 2, 16, true);             // the slab
        vrc_host::HipVoxelLabels labels = debris.labelComponents(6);
        std::printf("count=%llu\n", (unsigned long long)labels.count());
        const int down[3] = {7, 0, 4};                       // piece i moves by (0, -down[i], 0): q = p + (0, down, 0)
        std::vector<vrc_affine> maps(3);
        for (int i = 0; i < 3; ++i) {
            maps[i] = vrc_affine();
            maps[i].m[0] = maps[i].m[4] = maps[i].m[8] = 65536;
            maps[i].t[1] = (int64_t)down[i] << 17;
        }
        print("contact", labels.contacts(maps, world));
        std::vector<uint8_t> keep(3, 1);
        keep[2] = 0;
        std::vector<uint32_t> boxes(18);
        for (int i = 0; i < 3; ++i)
            for (int a = 0; a < 6; ++a) boxes[6 * i + a] = a < 3 ? 0u : 16u;
        boxes[3] = 4;                                        // the first piece only as far as x < 4
        print("kept", labels.contacts(maps, world, &boxes, &keep));
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 1;
    }
    return 0;
}
