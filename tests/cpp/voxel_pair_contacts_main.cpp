// Exercises HipVoxelLabels::candidatePairs and HipVoxelLabels::pairContacts of the C++ host adapter
// (cpuvoxelraycaster_amd/host/hip_raycaster.hpp) at 16^3: the three loose pieces of the rigid test.  The first box is lowered
// onto the second one until it sinks one cell into it, the speck (piece 1) is moved next to the first box; the boxes are the
// moved record boxes.  The pytest wrapper compares the printed pairs and records with the numpy model's.
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
        vrc_host::HipVoxelVolume debris(4);
        debris.fillBox(1, 9, 1, 7, 11, 6, true);
        debris.fillBox(9, 5, 9, 12, 8, 15, true);
        debris.fillBox(10, 8, 9, 11, 12, 10, true);          // an arm on the second box
        debris.setCell(vrc_host::Cell::Solid, vrc_host::Cell::Grass, 3, 13, 3);   // a speck, still in the queue
        vrc_host::HipVoxelLabels labels = debris.labelComponents(6);
        std::printf("count=%llu\n", (unsigned long long)labels.count());
        // piece i moves by move[i]: q = p - move
        const int move[3][3] = {{6, 2, 7}, {3, -2, 6}, {0, 0, 0}};
        const uint32_t lo_hi[3][6] = {{1, 9, 1, 7, 11, 6}, {3, 13, 3, 4, 14, 4}, {9, 5, 9, 12, 12, 15}};
        std::vector<vrc_affine> maps(3);
        std::vector<uint32_t> boxes(18);
        for (int i = 0; i < 3; ++i) {
            maps[i] = vrc_affine();
            maps[i].m[0] = maps[i].m[4] = maps[i].m[8] = 65536;
            for (int a = 0; a < 3; ++a) {
                maps[i].t[a] = -((int64_t)move[i][a] << 17);
                boxes[6 * i + a] = lo_hi[i][a] + move[i][a];
                boxes[6 * i + 3 + a] = lo_hi[i][3 + a] + move[i][a];
            }
        }
        const std::vector<uint32_t> pairs = labels.candidatePairs(boxes, 4);
        for (size_t k = 0; k < pairs.size(); k += 2) std::printf("pair=%u,%u\n", pairs[k], pairs[k + 1]);
        print("contact", labels.pairContacts(maps, pairs, 4, &boxes));
        std::vector<uint8_t> keep(3, 1);
        keep[1] = 0;
        const std::vector<uint32_t> fewer = labels.candidatePairs(boxes, 4, &keep);
        for (size_t k = 0; k < fewer.size(); k += 2) std::printf("keptpair=%u,%u\n", fewer[k], fewer[k + 1]);
        const std::vector<uint32_t> all = {0, 0, 0, 1, 0, 2, 1, 0, 2, 0};
        print("kept", labels.pairContacts(maps, all, 4, nullptr, &keep));
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 1;
    }
    return 0;
}
