// The piece boxes of the capsule brush (cpuvoxelraycaster_amd/csrc/vrc_stroke.h) held to the rule of include/vrc.h by brute
// force, on the host: built with -fsanitize=address,undefined by tests/test_stroke_host.py and run as a child process.
//   usage: stroke_pieces_main <seeded capsules at 64^3> <seed>
// One line per capsule:  <set> <index> S=<S> item=<8 numbers> covered=<0|1> voxels=<voxels of the rule inside the volume>
//                        pieces=<non-empty piece boxes> piece_items=<sum of their word items> box_items=<word items of the
//                        capsule's clipped bounding box>
// covered: every voxel of the volume that the rule names lies in the box of the piece whose slab holds it.  The rule is
// evaluated here in __int128, for every voxel of the capsule's bounding box grown by one voxel (nothing outside that box is
// within r of the segment); set "sums" only counts.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../cpuvoxelraycaster_amd/csrc/vrc_stroke.h"

typedef __int128 wide;

static bool rule(const int32_t it[8], int64_t x, int64_t y, int64_t z)
{
    const wide r = it[6];
    if (r < 0) return false;
    const wide d[3] = {(wide)it[3] - it[0], (wide)it[4] - it[1], (wide)it[5] - it[2]};
    const wide q[3] = {(wide)x - it[0], (wide)y - it[1], (wide)z - it[2]};
    const wide L2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2], qq = q[0] * q[0] + q[1] * q[1] + q[2] * q[2];
    const wide t = q[0] * d[0] + q[1] * d[1] + q[2] * d[2];
    if (L2 == 0 || t <= 0) return qq <= r * r;
    if (t >= L2) {
        const wide e[3] = {(wide)x - it[3], (wide)y - it[4], (wide)z - it[5]};
        return e[0] * e[0] + e[1] * e[1] + e[2] * e[2] <= r * r;
    }
    return qq * L2 - t * t <= r * r * L2;
}

// vrc_box_words.h: box_word_items, restated (that header needs the HIP runtime)
static uint64_t word_items(const uint32_t lo[3], const uint32_t hi[3])
{
    const uint32_t nbx = ((hi[0] - 1u) >> 1) - (lo[0] >> 1) + 1u, nby = ((hi[1] - 1u) >> 1) - (lo[1] >> 1) + 1u;
    const uint32_t wpr = (((((hi[2] - 1u) >> 1) - (lo[2] >> 1)) + 3u) >> 2) + 1u;
    return (uint64_t)nbx * nby * wpr;
}

struct Box {
    bool any;
    uint32_t lo[3], hi[3];
};

static bool report(const char* set, int index, uint32_t S, const int32_t it[8], bool brute)
{
    bool covered = true;
    uint64_t voxels = 0, piece_items = 0, box_items = 0, pieces = 0;
    if (vrc::stroke_item_kept(it)) {
        const vrc::Capsule c = {{it[0], it[1], it[2]}, {it[3], it[4], it[5]}, it[6]};
        const vrc::StrokePieces ps = vrc::stroke_pieces(c, S);
        std::vector<Box> boxes(ps.count);
        for (uint32_t k = 0; k < ps.count; ++k) {
            boxes[k].any = vrc::stroke_piece_box(c, S, ps, k, boxes[k].lo, boxes[k].hi);
            if (!boxes[k].any) continue;
            ++pieces;
            piece_items += word_items(boxes[k].lo, boxes[k].hi);
            for (int j = 0; j < 3; ++j) covered = covered && boxes[k].lo[j] < boxes[k].hi[j] && boxes[k].hi[j] <= S;
        }
        // the clipped bounding box, grown by one voxel for the brute force
        int64_t lo[3], hi[3];
        uint32_t blo[3], bhi[3];
        bool empty = it[6] < 0;
        for (int j = 0; j < 3; ++j) {
            const int64_t mn = it[j] < it[3 + j] ? it[j] : it[3 + j], mx = it[j] < it[3 + j] ? it[3 + j] : it[j];
            const int64_t l = mn - it[6], h = mx + it[6] + 1;
            lo[j] = l - 1 < 0 ? 0 : l - 1;
            hi[j] = h + 1 > (int64_t)S ? (int64_t)S : h + 1;
            blo[j] = (uint32_t)(l < 0 ? 0 : l);
            bhi[j] = (uint32_t)(h > (int64_t)S ? (int64_t)S : h);
            empty = empty || l >= (int64_t)S || h <= 0;
        }
        if (!empty) box_items = word_items(blo, bhi);
        if (brute && !empty)
            for (int64_t x = lo[0]; x < hi[0]; ++x)
                for (int64_t y = lo[1]; y < hi[1]; ++y)
                    for (int64_t z = lo[2]; z < hi[2]; ++z) {
                        if (!rule(it, x, y, z)) continue;
                        ++voxels;
                        const int64_t p[3] = {x, y, z};
                        const int64_t k = ps.count ? (p[ps.axis] - ps.first) / VRC_STROKE_PIECE : -1;
                        bool in = k >= 0 && k < (int64_t)ps.count && p[ps.axis] >= ps.first && boxes[k].any;
                        for (int j = 0; in && j < 3; ++j) in = p[j] >= (int64_t)boxes[k].lo[j] && p[j] < (int64_t)boxes[k].hi[j];
                        covered = covered && in;
                    }
    }
    std::printf("%s %d S=%u item=%d,%d,%d,%d,%d,%d,%d,%d covered=%d voxels=%llu pieces=%llu piece_items=%llu box_items=%llu\n", set, index, S, it[0],
                it[1], it[2], it[3], it[4], it[5], it[6], it[7], covered ? 1 : 0, (unsigned long long)voxels, (unsigned long long)pieces,
                (unsigned long long)piece_items, (unsigned long long)box_items);
    return covered;
}

static uint64_t state;
static uint32_t rnd(uint32_t n)          // splitmix64
{
    uint64_t z = (state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (uint32_t)((z ^ (z >> 31)) % n);
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    const int count = atoi(argv[1]);
    state = (uint64_t)atoll(argv[2]);
    bool all = true;
    const uint32_t S = 64;
    for (int i = 0; i < count; ++i) {
        int32_t it[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const uint32_t kind = rnd(8);
        for (int j = 0; j < 3; ++j) {
            it[j] = (int32_t)rnd(S + 40) - 20;
            it[3 + j] = kind == 0 ? it[j] : kind == 1 ? it[j] + (int32_t)rnd(7) - 3 : (int32_t)rnd(S + 40) - 20;
        }
        if (kind == 2) it[3 + rnd(3)] = it[rnd(3)];                      // often axis-aligned in one axis
        if (kind == 3) { it[3] = it[0] + 30; it[4] = it[1] - 30; it[5] = it[2] + 30; }   // a tie of the major axis
        if (kind == 4) { it[rnd(3)] = -(int32_t)rnd(8193); it[3 + rnd(3)] = (int32_t)rnd(8193); }      // ends far outside
        it[6] = kind == 5 ? (int32_t)rnd(40) : (int32_t)rnd(7) - 1;
        all = report("seeded", i, S, it, true) && all;
    }
    const int32_t L = VRC_STROKE_LIMIT;
    const int32_t limits[][8] = {
        {-L, -L, -L, L, L, L, 0, 0}, {-L, -L, -L, L, L, L, 1, 0}, {L, -L, L, -L, L, -L, 3, 0}, {-L, 10, 20, L, 40, 30, 2, 0},
        {30, 30, 30, 30, 30, 30, L, 0}, {-L, -L, -L, -L, -L, -L, L, 0}, {-L, L, -L, L, -L, L, L, 0}, {0, 0, 0, 63, 63, 63, L, 0},
        {L, L, L, L, L, L, L, 0}, {-L, 0, 0, L, 63, 0, 0, 0}, {L + 1, 0, 0, 0, 0, 0, 1, 0}, {0, 0, 0, 9, 9, 9, L + 1, 0}, {0, 0, 0, 9, 9, 9, 1, 1},
    };
    for (size_t i = 0; i < sizeof limits / sizeof limits[0]; ++i) all = report("limits", (int)i, S, limits[i], true) && all;
    const int32_t thin[][6] = {{-40, -40, -40, 295, 295, 295}, {0, 0, 0, 255, 1, 0}, {0, 3, 250, 255, 254, 253},
                               {5, 0, 7, 9, 255, 100}, {250, 7, 0, 3, 60, 255}, {255, 255, 255, 0, 0, 0}};
    const int32_t radii[] = {0, 1, 3};
    int index = 0;
    for (size_t i = 0; i < sizeof thin / sizeof thin[0]; ++i)
        for (int r = 0; r < 3; ++r) {
            const int32_t it[8] = {thin[i][0], thin[i][1], thin[i][2], thin[i][3], thin[i][4], thin[i][5], radii[r], 0};
            all = report("thin", index++, 256, it, true) && all;
        }
    const int32_t diagonal[8] = {0, 0, 0, 511, 511, 511, 3, 0}, fat[8] = {128, 256, 256, 384, 256, 256, 64, 0};
    report("sums", 0, 512, diagonal, false);
    report("sums", 1, 512, fat, false);
    std::printf("all_covered=%d\n", all ? 1 : 0);
    return 0;
}
