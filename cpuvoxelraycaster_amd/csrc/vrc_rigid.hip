// vrc_rigid.hip -- the pieces of a labelling as rigid bodies with a pose (include/vrc.h: vrc_rigid_moments,
// vrc_rigid_place_affine, vrc_rigid_contacts, vrc_rigid_clearance): the raw moments a physics engine derives mass, centre of mass and inertia
// tensor from, the write-back of every piece through its own inverse affine map, and the contact record of every piece
// under such a map against a world.  The labels are vrc_components.hip's: one uint32 id per KEY
// (vrc_box_words.h: voxel_key / key_voxel), VRC_NO_COMPONENT outside M.  Exact in integers.
//
// Moments.  A lane owns a key, a workgroup GROUP x ROUNDS consecutive keys (256 occupancy words), as the labelling's passes
// do; within it every wave walks its own 64 x ROUNDS consecutive keys, a quarter of them, 8 bricks = 16 voxels along z a round.  With c = 2p + 1 a voxel adds ten terms to its piece: 1, c_x, c_y, c_z and the six products.  One 64-bit atomic per
// voxel and term would queue every voxel of a large piece on ten words, so the terms are summed on chip first; pieces are
// spatially coherent, so most waves see ONE id:
//   uniform   every voxel of the wave's 64 keys carries one id: the lanes add their terms to ten 32-bit registers (a term is
//             below 2^22, a lane adds at most ROUNDS of them) and carry them from round to round while the id stays.  When it
//             changes, and at the end, the wave sums the registers in 64 bits; at the end the four waves meet in LDS and the
//             waves that hold the same id issue their ten atomics once -- a workgroup wholly inside one piece costs ten;
//   few       a wave with several ids takes a leader's id, sums the matching lanes with shuffles (32 bits: 64 terms), lets
//             the leader issue the ten atomics and masks the lanes off, FEW times at the most;
//   many      whatever lanes are left then (a checkerboard: every lane its own id) issue their own ten atomics.
// An id outside the window or VRC_NO_COMPONENT costs no atomic.  Every sum is below 2^53 (vrc.h), every atomic a 64-bit vector
// atomic add at agent scope in plain HIP C++; integer adds commute, so the bytes do not depend on the schedule.
//
// Placement.  vrc_stamp.hip's gather with the id array for a source: one thread per (piece, destination occupancy word), the
// 64-bit map evaluated once per word and the other 31 voxels following in 32-bit running sums.  The source bit of q is
// "q lies in the piece's record box and id(q) == piece": the record box stands in for the volume in the stamp's miss / inside
// test, so a word whose source bounding box misses the piece loads nothing.  The grid is 2-D and needs neither scratch nor
// a look at the boxes from the host: blockIdx.y strides over the pieces, blockIdx.x over the words of that piece's box.
// Pieces may overlap in dst, so a word is written with a 32-bit vector atomic OR / AND, and not at all where its 32 bits are
// 0.  Within a wave every lane has a word of its own -- except in a destination of 4^3, where two brick rows share a word:
// there the lanes that hit one word join their bits first.
//
// Measured on an MI355X at 512^3 on the fall benchmark's scene (tools/bench_edit.py --rigid, profiles/edit/bench_rigid.json; 404
// loose blocks of 1.9 M voxels; device time by events, median of 5): the moments of all pieces 0.44 ms next to 0.20 ms of
// vrc_labels_select in the same run -- the waves there are uniform, and since a wave walks consecutive keys (16 voxels along
// z a round) and a block is 30 voxels long, a run of one id lasts about two rounds, after which the 64-bit wave sums and the
// ten atomics come.  With the rounds of a wave GROUP keys = 64 voxels apart the id changed every round: 0.66 ms.  The
// placement with pure-translation maps (0.16 M box words) 0.075 ms next to 0.19 ms of vrc_fall_place, with a 30-degree turn
// about two axes (0.74 M box words) 0.078 ms: the same time for 4.5 times the words, so the fixed grid and the per-piece
// set-up seem to set it at this size; not measured apart.
//
// Contacts.  The placement's grid, per-piece set-up (pose_piece) and per-word gather (posed_word), one copy for both kernels;
// where the placement stores the gathered word, k_contacts reduces it.  A word with no gathered bit -- almost all of a
// generous box -- ends there.  Another loads the world word and at most six neighbour words, builds W*(p - e_a) and
// W*(p + e_a) for its 32 voxels by shifts under constant masks (a neighbour beyond the volume is all ones; a 4^3 world, whose
// rows share words, is brought to the same form by world_word), and adds popcounts: the counts, the normals as differences,
// the sums of c = 2p + 1 from the x and y parity planes and the three bit planes of the layer number.  32 bits in a lane, 64
// from the wave sums on; the four waves meet in LDS and lanes 0..14 issue the non-zero ones of the 15 sums as 64-bit vector
// atomic adds in plain HIP C++.  A workgroup that gathered nothing for a piece issues none.
// Measured on the same scene (tools/bench_edit.py --contacts, profiles/edit/bench_contacts.json; the zeroing of the records
// included): translation maps against the supported part 0.111 ms next to 0.081 ms of the placement with the same maps and
// boxes in the same run (1.37 times), the 30-degree turn 0.118 ms next to 0.080 ms (1.48 times); against the whole medium,
// where most gathered words meet solid, 0.110 and 0.116 ms.  The passes have not been timed apart.
//
// Pair contacts (vrc_rigid_pair_contacts).  k_contacts with a second posed piece for a world: blockIdx.y strides over the listed
// pairs, the workgroup poses both pieces, and where k_contacts loads the world word and its six neighbours, k_pair_contacts
// gathers them from piece b (piece_word) under a mask of the bits the sums will read -- up to 32 ids for the centre word, 16
// for an x or y face, 4 for a z face -- with zeros for walls.  contact_sums, add_set and contact_flush are one copy for both.
// The broad phase (vrc_rigid_box_pair_count / vrc_rigid_box_pairs) is k_box_pairs: a thread per a over all b, count, scan
// (vrc_group.h), emit.
// Measured on the same scene with the 30-degree turn (tools/bench_edit.py --pair-contacts, profiles/edit/bench_pair_contacts.json):
// 3688 candidate pairs of the 404 pieces counted and listed in 0.33 ms (two synchronous calls, their scratch allocation
// included), all their records in 0.81 ms (652 pairs overlap, 798 touch), next to 0.098 ms PER PAIR of clearing a scratch
// volume, placing b and calling vrc_rigid_contacts for a (64 sampled pairs; 360 ms scaled to all, 445 times).  The passes have
// not been timed apart.
//
// Clearance (vrc_rigid_clearance).  k_contacts with a dense uint32 field (a vrc_distance snapshot) for a world: a lane with
// gathered bits walks them and loads the field at each -- up to 32 values in four runs of eight along z -- into a count, a
// count of VRC_DISTANCE_NONE, a 64-bit sum, and a packed minimum (value << 32 | index) and maximum (value << 32 | ~index)
// that carry the voxel of smallest dense index with them.  clearance_flush is contact_flush for these five: shuffles, LDS,
// at most three atomic adds, one atomicMin and one atomicMax per workgroup and piece.  The record itself holds the two
// packed words while the kernel runs; a kernel of one thread per record before it writes the identities and one after it
// decodes them in place, so the call keeps no scratch.
// Measured on the same scene over the Euclidean field of the supported part (tools/bench_edit.py --clearance,
// profiles/edit/bench_clearance.json; A B A B with vrc_rigid_contacts against the supported part, same maps and boxes, same
// run): translation maps 0.121 ms next to 0.109 ms of the contact call (1.11 times), the 30-degree turn 0.122 ms next to
// 0.117 ms (1.05 times).  The three kernels and their passes have not been timed apart.
#include "vrc_rigid.h"

#include <stddef.h>

#include "vrc_box_words.h"
#include "vrc_group.h"

namespace {

constexpr uint32_t NONE = VRC_NO_COMPONENT;
constexpr uint32_t GROUP = 256;               // lanes per workgroup
constexpr uint32_t WAVES = GROUP / 64u;
constexpr uint32_t ROUNDS = 32;               // a workgroup of the moments pass takes ROUNDS x GROUP consecutive keys
constexpr uint32_t GROUP_KEYS = GROUP * ROUNDS;
constexpr uint32_t WAVE_KEYS = 64u * ROUNDS;       // the consecutive keys one wave of the moments pass walks
constexpr uint32_t SUMS = 10;                 // vrc_piece_moments as ten uint64: voxels, s1[3], s2[6]
constexpr uint32_t FEW = 4;                   // ids a mixed wave reduces with shuffles before its lanes go alone

constexpr uint32_t CONTACT_SUMS = 15;         // vrc_piece_contact: posed, overlap (count, s1[3], n[3]), touch (the same); then `reserved`
constexpr uint32_t CONTACT_WORDS = 16;

static_assert(sizeof(vrc_piece_moments) == SUMS * 8u, "vrc_piece_moments is ten 64-bit sums");
static_assert(sizeof(vrc_piece_contact) == CONTACT_WORDS * 8u, "vrc_piece_contact is 15 64-bit sums and a reserved word");
static_assert(sizeof(vrc_affine) == 64, "vrc_affine is 64 bytes");

// the registers of a uniform run, summed over the wave and added to record `slot` by lane 0; called by whole waves
__device__ __forceinline__ void flush_run(const uint32_t acc[SUMS], uint32_t slot, unsigned long long* out)
{
    for (uint32_t k = 0; k < SUMS; ++k) {
        const unsigned long long s = wave_sum((unsigned long long)acc[k]);
        if ((threadIdx.x & 63u) == 0u) atomicAdd(out + (size_t)SUMS * slot + k, s);
    }
}

__global__ __launch_bounds__(GROUP) void k_moments(uint32_t lg, uint32_t n_keys, const uint32_t* __restrict__ L, uint32_t first, uint32_t want,
                                                   unsigned long long* out)
{
    __shared__ unsigned long long part[WAVES][SUMS];
    __shared__ uint32_t part_slot[WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t acc[SUMS];
    for (uint32_t k = 0; k < SUMS; ++k) acc[k] = 0u;
    uint32_t run = NONE;                                                // wave-uniform: the record the registers belong to
    for (uint32_t r = 0; r < ROUNDS; ++r) {
        // a wave walks its own WAVE_KEYS CONSECUTIVE keys, 16 voxels further along z every round, so that a run lasts as long as the
        // piece does along z; whole waves pass or fail the bound
        const uint32_t key = blockIdx.x * GROUP_KEYS + wave * WAVE_KEYS + r * 64u + lane;
        if (key >= n_keys) break;
        const uint32_t id = L[key];
        const uint32_t slot = id - first;
        const bool in = id != NONE && id >= first && slot < want;
        unsigned long long todo = __ballot(in);
        if (!todo) continue;                                            // wave-uniform
        uint32_t c[3], t[SUMS];
        key_voxel(lg, key, c);
        for (int a = 0; a < 3; ++a) c[a] = in ? 2u * c[a] + 1u : 0u;
        t[0] = in ? 1u : 0u;
        t[1] = c[0]; t[2] = c[1]; t[3] = c[2];
        t[4] = c[0] * c[0]; t[5] = c[1] * c[1]; t[6] = c[2] * c[2];
        t[7] = c[0] * c[1]; t[8] = c[0] * c[2]; t[9] = c[1] * c[2];
        const uint32_t lslot = __shfl(slot, __ffsll((long long)todo) - 1);
        if (__ballot(in && slot != lslot) == 0ull) {                    // uniform: carried in registers
            if (run != lslot) {
                if (run != NONE) flush_run(acc, run, out);
                for (uint32_t k = 0; k < SUMS; ++k) acc[k] = 0u;
                run = lslot;
            }
            for (uint32_t k = 0; k < SUMS; ++k) acc[k] += t[k];
            continue;
        }
        for (uint32_t pass = 0; todo && pass < FEW; ++pass) {           // few: wave-uniform
            const int leader = __ffsll((long long)todo) - 1;
            const uint32_t ls = __shfl(slot, leader);
            const bool mine = in && slot == ls;
            const unsigned long long same = __ballot(mine);
            todo &= ~same;
            if (same & (same - 1ull)) {
                for (uint32_t k = 0; k < SUMS; ++k) {
                    const uint32_t s = wave_sum(mine ? t[k] : 0u);
                    if ((int)lane == leader) atomicAdd(out + (size_t)SUMS * ls + k, (unsigned long long)s);
                }
            } else if ((int)lane == leader) {
                for (uint32_t k = 0; k < SUMS; ++k) atomicAdd(out + (size_t)SUMS * ls + k, (unsigned long long)t[k]);
            }
        }
        if ((todo >> lane) & 1ull)                                      // many: the lanes that are left
            for (uint32_t k = 0; k < SUMS; ++k) atomicAdd(out + (size_t)SUMS * slot + k, (unsigned long long)t[k]);
    }
    // the end of the runs: the waves of the workgroup that hold the same record add once
    unsigned long long total[SUMS];
    for (uint32_t k = 0; k < SUMS; ++k) total[k] = run != NONE ? wave_sum((unsigned long long)acc[k]) : 0ull;
    if (lane == 0u) {
        part_slot[wave] = run;
        for (uint32_t k = 0; k < SUMS; ++k) part[wave][k] = total[k];
    }
    __syncthreads();
    if (threadIdx.x >= SUMS) return;
    const uint32_t k = threadIdx.x;
    for (uint32_t w = 0; w < WAVES; ++w) {
        const uint32_t slot = part_slot[w];
        if (slot == NONE) continue;
        bool earlier = false;
        for (uint32_t v = 0; v < w; ++v) earlier = earlier || part_slot[v] == slot;
        if (earlier) continue;
        unsigned long long s = 0ull;
        for (uint32_t v = w; v < WAVES; ++v) s += part_slot[v] == slot ? part[v][k] : 0ull;
        atomicAdd(out + (size_t)SUMS * slot + k, s);
    }
}

// The 32 source bits of one destination word, under `mask`: bit = 1 iff the voxel's source q lies in [rlo, rhi) and carries
// `piece`.  q / frac / step as in vrc_stamp.hip's gather_word; ext = rhi - rlo.  INSIDE: every q of the word lies in the box.
template <bool INSIDE>
__device__ __forceinline__ uint32_t gather_piece(const uint32_t* __restrict__ L, uint32_t lg, uint32_t piece, const uint32_t rlo[3], const uint32_t ext[3],
                                                 const int32_t q[3], const int32_t frac[3], const int32_t step[3][3], uint32_t mask)
{
    uint32_t bits = 0u;
#pragma unroll
    for (uint32_t col = 0; col < 4u; ++col) {          // col = y * 2 + x, as in a brick's bit index
        int32_t d[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) d[a] = frac[a] + ((col & 1u) ? step[a][0] : 0) + ((col & 2u) ? step[a][1] : 0);
#pragma unroll
        for (uint32_t k = 0; k < 8u; ++k) {
            const uint32_t bit = (k >> 1) * 8u + (k & 1u) * 4u + col;
            if ((mask >> bit) & 1u) {
                const uint32_t x = (uint32_t)(q[0] + (d[0] >> 17)), y = (uint32_t)(q[1] + (d[1] >> 17)), z = (uint32_t)(q[2] + (d[2] >> 17));
                // unsigned: a coordinate below rlo, a negative one included, is a large one
                if (INSIDE || (x - rlo[0] < ext[0] && y - rlo[1] < ext[1] && z - rlo[2] < ext[2]))
                    bits |= (L[voxel_key(lg, x, y, z)] == piece ? 1u : 0u) << bit;
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) d[a] += step[a][2];
        }
    }
    return bits;
}

// What a workgroup knows of a piece before it walks the words of the piece's box: the per-piece set-up of the two kernels
// that gather posed pieces (k_place_affine stores the gathered bits, k_contacts reduces them).
struct Posed {
    vrc_affine map;
    BoxWords b;                          // the piece's box of the destination, clipped
    uint32_t rlo[3], ext[3];             // the piece's record box in the labels' volume: what bounds the loads of ids
    int32_t rmin[3], rmax[3];
    int32_t step[3][3], dmin[3], dmax[3];        // per source axis: s per destination voxel step (|.| <= 2^21), and the extremes of delta over a word's 2 x 2 x 8 voxels
};

// false: the piece is skipped whole -- keep[piece] == 0, a map beyond the limits, an empty or inverted box, an empty record.
// Uniform for the workgroup.  Sd / Ss: the voxels per axis of the destination / of the labels' volume.
__device__ __forceinline__ bool pose_piece(const vrc_component* __restrict__ records, uint32_t piece, const uint8_t* __restrict__ keep,
                                           const vrc_affine* __restrict__ maps, const uint32_t* __restrict__ boxes, uint32_t Sd, uint32_t Ss, Posed& s)
{
    if (keep && keep[piece] == 0) return false;
    s.map = maps[piece];
    bool legal = s.map.reserved == 0;
    for (int i = 0; i < 9; ++i) legal = legal && s.map.m[i] <= vrc::AFFINE_M_LIMIT && s.map.m[i] >= -vrc::AFFINE_M_LIMIT;
    for (int a = 0; a < 3; ++a) legal = legal && s.map.t[a] <= vrc::AFFINE_T_LIMIT && s.map.t[a] >= -vrc::AFFINE_T_LIMIT;
    if (!legal) return false;
    uint32_t given[6], lo[3], hi[3];
    for (uint32_t a = 0; a < 6u; ++a) given[a] = boxes ? boxes[6u * piece + a] : (a < 3u ? 0u : Sd);
    if (!clip_box(given, Sd, lo, hi)) return false;
    bool none = false;
    for (int a = 0; a < 3; ++a) {
        s.rlo[a] = records[piece].lo[a];
        const uint32_t rhi = min(records[piece].hi[a], Ss);
        none = none || s.rlo[a] >= rhi;
        s.ext[a] = rhi - s.rlo[a];
        s.rmin[a] = (int32_t)s.rlo[a]; s.rmax[a] = (int32_t)rhi - 1;
    }
    if (none) return false;
    s.b = box_words(lo, hi);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int c = 0; c < 3; ++c) s.step[a][c] = 2 * s.map.m[3 * a + c];
        s.dmin[a] = min(s.step[a][0], 0) + min(s.step[a][1], 0) + 7 * min(s.step[a][2], 0);
        s.dmax[a] = max(s.step[a][0], 0) + max(s.step[a][1], 0) + 7 * max(s.step[a][2], 0);
    }
    return true;
}

// the gathered bits of the piece in destination word r under `want`, a mask of the word's bits the caller needs (the box's
// own mask is ANDed to it): the map evaluated once in 64 bits, then gather_piece.  r is an item of s.b or any other word of
// the destination made by piece_word below; a word outside the box has the mask 0 and costs no load.
__device__ __forceinline__ uint32_t posed_word(const uint32_t* __restrict__ L, uint32_t lg, uint32_t piece, const Posed& s, const RowWord& r, uint32_t want)
{
    const uint32_t mask = box_mask(s.b, r) & want;
    if (!mask) return 0u;
    // z of the word's first voxel, relative to the row (negative where the word starts in the row before: n = 2;
    // those voxels are outside the mask)
    const int64_t z0 = 2 * ((int64_t)(4u * r.w) - (int64_t)r.base);
    const int64_t c[3] = {4 * (int64_t)r.cx + 1, 4 * (int64_t)r.cy + 1, 2 * z0 + 1};   // 2p + 1: the centre in half voxels
    int32_t q[3], frac[3];
    bool miss = false, inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int64_t v = (int64_t)s.map.m[3 * a] * c[0] + (int64_t)s.map.m[3 * a + 1] * c[1] + (int64_t)s.map.m[3 * a + 2] * c[2] + s.map.t[a];
        q[a] = (int32_t)(v >> 17);                 // |v| < 2^41
        frac[a] = (int32_t)(v & 0x1ffff);
        const int32_t qmin = q[a] + ((frac[a] + s.dmin[a]) >> 17), qmax = q[a] + ((frac[a] + s.dmax[a]) >> 17);
        miss = miss || qmax < s.rmin[a] || qmin > s.rmax[a];
        inside = inside && qmin >= s.rmin[a] && qmax <= s.rmax[a];
    }
    if (miss) return 0u;
    return inside ? gather_piece<true>(L, lg, piece, s.rlo, s.ext, q, frac, s.step, mask) : gather_piece<false>(L, lg, piece, s.rlo, s.ext, q, frac, s.step, mask);
}

__global__ __launch_bounds__(GROUP) void k_place_affine(const uint32_t* __restrict__ L, uint32_t lg, const vrc_component* __restrict__ records, uint32_t C,
                                                        const uint8_t* __restrict__ keep, const vrc_affine* __restrict__ maps, const uint32_t* __restrict__ boxes,
                                                        uint32_t* dst, uint32_t Sd, int op)
{
    const uint32_t n = Sd >> 1, Ss = 2u << lg;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t piece = blockIdx.y; piece < C; piece += gridDim.y) {  // uniform for the workgroup, and so is all that skips a piece
        Posed s;
        if (!pose_piece(records, piece, keep, maps, boxes, Sd, Ss, s)) continue;
        for (uint64_t base = (uint64_t)blockIdx.x * GROUP; base < s.b.items; base += (uint64_t)gridDim.x * GROUP) {      // uniform trip count
            const uint64_t it = base + threadIdx.x;
            uint32_t bits = 0u;
            RowWord r;
            r.w = 0u;
            if (it < s.b.items && row_word(s.b, n, it, r)) bits = posed_word(L, lg, piece, s, r, ~0u);
            if (n >= 4u) {                                              // a lane, a word
                if (bits) {
                    if (op == VRC_COPY_OR) atomicOr(&dst[r.w], bits);
                    else atomicAnd(&dst[r.w], ~bits);
                }
                continue;
            }
            // 4^3: two words in all, shared by the rows
            const uint32_t word = (uint32_t)r.w;
            unsigned long long todo = __ballot(bits != 0u);
            while (todo) {                                              // wave-uniform
                const int leader = __ffsll((long long)todo) - 1;
                const uint32_t lword = __shfl(word, leader);
                const bool mine = bits != 0u && word == lword;
                todo &= ~__ballot(mine);
                uint32_t joined = mine ? bits : 0u;
                for (int o = 32; o; o >>= 1) joined |= __shfl_xor(joined, o);
                if ((int)lane == leader) {
                    if (op == VRC_COPY_OR) atomicOr(&dst[lword], joined);
                    else atomicAnd(&dst[lword], ~joined);
                }
            }
        }
    }
}

// ---- contacts ------------------------------------------------------------------------------------------------------

// A world word as the contact step sees it: word k of brick row (cx, cy), bit 4 zl + 2 y + x for the voxel (x, y) of the 2 x 2
// column in z layer zl of the word's eight.  From 8^3 on (n >= 4) a row is n / 4 whole words and this is a load.  In a world of
// 4^3 (n = 2) a row is two bytes and two rows share a word: there the row's 16 bits are moved down to layers 0..3 and layers
// 4..7, which lie beyond the volume, read as ones -- a wall, as every neighbour beyond the volume does -- so that the shifts
// below hold for it unchanged; the gathered bits are moved down by the same amount (contact_word).
__device__ __forceinline__ uint32_t world_word(const uint32_t* __restrict__ W, uint32_t n, uint32_t cx, uint32_t cy, uint32_t k)
{
    if (n >= 4u) return W[((((uint64_t)cx * n + cy) * n) >> 2) + k];
    const uint32_t b = (cx * 2u + cy) * 2u;                             // the row's first byte, 0 .. 6
    return 0xffff0000u | ((W[b >> 2] >> (8u * (b & 3u))) & 0xffffu);
}

// one set M of voxels of a word added to its count, its sums of c = 2p + 1 and its sums of normals: popcounts only.  c0 = c of
// the word's voxel 0; the x and y parity planes and the three bit planes of the layer number give what the other voxels add.
__device__ __forceinline__ void add_set(uint32_t M, const uint32_t c0[3], const uint32_t lower[3], const uint32_t upper[3], uint32_t acc[7])
{
    const uint32_t k = __popc(M);
    acc[0] += k;
    acc[1] += k * c0[0] + 2u * __popc(M & 0xaaaaaaaau);
    acc[2] += k * c0[1] + 2u * __popc(M & 0xccccccccu);
    acc[3] += k * c0[2] + 2u * (__popc(M & 0xf0f0f0f0u) + 2u * __popc(M & 0xff00ff00u) + 4u * __popc(M & 0xffff0000u));
#pragma unroll
    for (int a = 0; a < 3; ++a) acc[4 + a] += (uint32_t)(__popc(M & lower[a]) - __popc(M & upper[a]));        // two's complement
}

// The contact step of one word with gathered bits != 0, the seven words given as values: w = the world's word under the bits
// and the words across its six faces, each already in the form "1 = solid, or what the caller lets a voxel beyond the
// volume read".  The six neighbour masks are whole-word operations; then the 15 sums.  c0 = c of the word's voxel 0.
// acc: posed, then overlap (count, s1 x 3, n x 3), then touch.  Of w only the bits under `bits` and their neighbours inside
// the word are read, of xm / xp the odd / even x plane, of ym / yp the upper / lower y plane, of zm / zp the last / first layer.
__device__ __forceinline__ void contact_sums(uint32_t bits, uint32_t w, uint32_t xm, uint32_t xp, uint32_t ym, uint32_t yp, uint32_t zm, uint32_t zp,
                                             const uint32_t c0[3], uint32_t acc[15])
{
    // W*(p - e_a) and W*(p + e_a) for the 32 voxels p of the word
    const uint32_t lower[3] = {((w & 0x55555555u) << 1) | ((xm & 0xaaaaaaaau) >> 1), ((w & 0x33333333u) << 2) | ((ym & 0xccccccccu) >> 2), (w << 4) | (zm >> 28)};
    const uint32_t upper[3] = {((w & 0xaaaaaaaau) >> 1) | ((xp & 0x55555555u) << 1), ((w & 0xccccccccu) >> 2) | ((yp & 0x33333333u) << 2), (w >> 4) | (zp << 28)};
    acc[0] += __popc(bits);
    add_set(bits & w, c0, lower, upper, acc + 1);
    add_set(bits & ~w & (lower[0] | lower[1] | lower[2] | upper[0] | upper[1] | upper[2]), c0, lower, upper, acc + 8);
}

// vrc_rigid_contacts' step: the world word and at most six neighbour words are loads, a neighbour beyond the volume is a wall
__device__ __forceinline__ void contact_word(const uint32_t* __restrict__ W, uint32_t n, const RowWord& r, uint32_t bits, uint32_t acc[15])
{
    const uint32_t rows = n >= 4u ? n >> 2 : 1u;                        // words per row
    const uint32_t k = n >= 4u ? (uint32_t)(r.w - (r.base >> 2)) : 0u;
    if (n < 4u) bits >>= 8u * ((uint32_t)r.base & 3u);                  // 4^3: the row's two bytes down to layers 0..3 (world_word)
    const uint32_t cx = r.cx, cy = r.cy;
    const uint32_t w = world_word(W, n, cx, cy, k);
    // across the word's faces: the rows cx -+ 1 and cy -+ 1 and the words k -+ 1 of the same row; beyond the volume all ones
    const uint32_t xm = cx ? world_word(W, n, cx - 1u, cy, k) : ~0u, xp = cx + 1u < n ? world_word(W, n, cx + 1u, cy, k) : ~0u;
    const uint32_t ym = cy ? world_word(W, n, cx, cy - 1u, k) : ~0u, yp = cy + 1u < n ? world_word(W, n, cx, cy + 1u, k) : ~0u;
    const uint32_t zm = k ? world_word(W, n, cx, cy, k - 1u) : ~0u, zp = k + 1u < rows ? world_word(W, n, cx, cy, k + 1u) : ~0u;
    const uint32_t c0[3] = {4u * cx + 1u, 4u * cy + 1u, 16u * k + 1u};
    contact_sums(bits, w, xm, xp, ym, yp, zm, zp, c0, acc);
}

// The end of a workgroup's walk over one record's words: the lanes' 32-bit sums become 64-bit wave sums, the four waves meet
// in LDS and lanes 0..14 add the non-zero ones of the 15 sums to `record` with 64-bit vector atomic adds.  Called by the whole
// workgroup; one that gathered nothing (acc[0] is `posed`) issues nothing.  The first barrier also keeps the LDS of the record
// before until its readers are done.
__device__ __forceinline__ void contact_flush(const uint32_t acc[CONTACT_SUMS], unsigned long long (*part)[CONTACT_SUMS], unsigned long long* record)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (!__syncthreads_or(acc[0] != 0u)) return;
    const bool some = __ballot(acc[0] != 0u) != 0ull;                   // wave-uniform
    for (uint32_t k = 0; k < CONTACT_SUMS; ++k) {
        // the normals (k = 5..7, 12..14) are signed
        const bool is_signed = (k >= 5u && k <= 7u) || k >= 12u;
        const unsigned long long mine = is_signed ? (unsigned long long)(long long)(int32_t)acc[k] : (unsigned long long)acc[k];
        const unsigned long long total = some ? wave_sum(mine) : 0ull;
        if (lane == 0u) part[wave][k] = total;
    }
    __syncthreads();
    if (threadIdx.x < CONTACT_SUMS) {                                   // the non-zero sums of the workgroup: at most 15 atomics
        unsigned long long v = 0ull;
        for (uint32_t wv = 0; wv < WAVES; ++wv) v += part[wv][threadIdx.x];
        if (v) atomicAdd(record + threadIdx.x, v);
    }
}

// k_place_affine's grid and gather, ending in a reduction: the contact record of every piece against the world W (Sd^3).
// Width of the sums.  One word adds at most 32 to a count or a normal and less than 32 * 2048 = 2^16 to a sum of c.  A lane
// takes the words of a box by grid stride: at most 512 * 512 * 129 < 2^25.02 words (all of 1024^3) over at least 4
// workgroups = 1024 lanes (contacts_run), so fewer than 2^15.02 words and sums below 2^31.02: the lanes add in 32 bits
// (normals in two's complement).  Sixty-four lanes no longer fit: the wave sums, the LDS and the atomics are 64 bits wide.
__global__ __launch_bounds__(GROUP) void k_contacts(const uint32_t* __restrict__ L, uint32_t lg, const vrc_component* __restrict__ records, uint32_t C,
                                                    const uint8_t* __restrict__ keep, const vrc_affine* __restrict__ maps, const uint32_t* __restrict__ boxes,
                                                    const uint32_t* __restrict__ W, uint32_t Sd, unsigned long long* out)
{
    __shared__ unsigned long long part[WAVES][CONTACT_SUMS];
    const uint32_t n = Sd >> 1, Ss = 2u << lg;
    for (uint32_t piece = blockIdx.y; piece < C; piece += gridDim.y) {  // uniform for the workgroup, and so is all that skips a piece
        Posed s;
        if (!pose_piece(records, piece, keep, maps, boxes, Sd, Ss, s)) continue;
        uint32_t acc[CONTACT_SUMS];
        for (uint32_t k = 0; k < CONTACT_SUMS; ++k) acc[k] = 0u;
        for (uint64_t base = (uint64_t)blockIdx.x * GROUP; base < s.b.items; base += (uint64_t)gridDim.x * GROUP) {      // uniform trip count
            const uint64_t it = base + threadIdx.x;
            RowWord r;
            if (it < s.b.items && row_word(s.b, n, it, r)) {
                const uint32_t bits = posed_word(L, lg, piece, s, r, ~0u);
                if (bits) contact_word(W, n, r, bits, acc);             // almost no word of a generous box gets here
            }
        }
        contact_flush(acc, part, out + (size_t)CONTACT_WORDS * piece);
    }
}

// ---- contacts between posed pieces, pair by pair ---------------------------------------------------------------

// Word k of brick row (cx, cy) of the posed volume as piece `piece` under s fills it, under `want`: the "world word" of the
// pair kernel, a gather of ids where world_word loads.  The word need not be an item of s.b: outside the piece's box the box
// mask is 0, and so the result without a load -- a voxel beyond box b is not in A_b.  From 8^3 on this is posed_word of the
// word.  In a posed volume of 4^3 (n = 2) two rows share a word and the row's 16 bits lie in its lower or upper half: `want`
// comes in, and the bits go out, moved DOWN to layers 0..3 -- the form contact_word brings a's bits to -- and layers 4..7,
// which lie beyond the volume, read 0 here: there are no walls between pieces.
__device__ __forceinline__ uint32_t piece_word(const uint32_t* __restrict__ L, uint32_t lg, uint32_t piece, const Posed& s, uint32_t n, uint32_t cx, uint32_t cy,
                                               uint32_t k, uint32_t want)
{
    if (!want) return 0u;
    RowWord r;
    r.cx = cx; r.cy = cy;
    r.base = ((uint64_t)cx * n + cy) * n;
    r.first = r.base + s.b.cz0; r.last = r.base + s.b.cz1;
    if (n >= 4u) {
        r.w = (r.base >> 2) + k;
        return posed_word(L, lg, piece, s, r, want);
    }
    const uint32_t up = 8u * ((uint32_t)r.base & 3u);
    r.w = r.base >> 2;
    return (posed_word(L, lg, piece, s, r, (want & 0xffffu) << up) >> up) & 0xffffu;
}

// The contact step of one word of A_a with bits != 0 against A_b: contact_word with gathers for loads and zeros for walls.
// A gather is asked only for the bits the sums will read: under the word itself a's bits and their neighbours inside the word
// (at most 32 ids), across an x or y face the one plane that faces a's bits there (at most 16), across a z face one layer
// (at most 4); a face with none of a's bits on it, a word beyond the volume, one outside box b and one whose source box
// misses b's record box cost nothing.
// 4^3: a's bits are moved down to layers 0..3 as in contact_word, and piece_word hands b's rows over in the same form, each
// from its own half of its own word: row (cx, cy) lies in half (2 cx + cy) & 1 of word cx, so the x neighbours come from the
// other word and the y neighbour from the other half of the same one.  The row is the whole of z, so no word lies before or
// after it, and with layers 4..7 reading 0 the shift (w >> 4) gives layer 3 an empty upper neighbour, as the rule wants.
__device__ __forceinline__ void pair_word(const uint32_t* __restrict__ L, uint32_t lg, uint32_t b, const Posed& sb, uint32_t n, const RowWord& r, uint32_t bits,
                                          uint32_t acc[15])
{
    const uint32_t rows = n >= 4u ? n >> 2 : 1u;                        // words per row
    const uint32_t k = n >= 4u ? (uint32_t)(r.w - (r.base >> 2)) : 0u;
    if (n < 4u) bits >>= 8u * ((uint32_t)r.base & 3u);
    const uint32_t cx = r.cx, cy = r.cy;
    const uint32_t near = bits | ((bits & 0xaaaaaaaau) >> 1) | ((bits & 0x55555555u) << 1) | ((bits & 0xccccccccu) >> 2) | ((bits & 0x33333333u) << 2) |
                          (bits << 4) | (bits >> 4);
    const uint32_t w = piece_word(L, lg, b, sb, n, cx, cy, k, near);
    const uint32_t xm = cx ? piece_word(L, lg, b, sb, n, cx - 1u, cy, k, (bits & 0x55555555u) << 1) : 0u;
    const uint32_t xp = cx + 1u < n ? piece_word(L, lg, b, sb, n, cx + 1u, cy, k, (bits & 0xaaaaaaaau) >> 1) : 0u;
    const uint32_t ym = cy ? piece_word(L, lg, b, sb, n, cx, cy - 1u, k, (bits & 0x33333333u) << 2) : 0u;
    const uint32_t yp = cy + 1u < n ? piece_word(L, lg, b, sb, n, cx, cy + 1u, k, (bits & 0xccccccccu) >> 2) : 0u;
    const uint32_t zm = k ? piece_word(L, lg, b, sb, n, cx, cy, k - 1u, bits << 28) : 0u;
    const uint32_t zp = k + 1u < rows ? piece_word(L, lg, b, sb, n, cx, cy, k + 1u, bits >> 28) : 0u;
    const uint32_t c0[3] = {4u * cx + 1u, 4u * cy + 1u, 16u * k + 1u};
    contact_sums(bits, w, xm, xp, ym, yp, zm, zp, c0, acc);
}

// k_contacts with a second posed piece for a world: out[pair] = the contact record of A_a against A_b without walls, for
// every listed pair (a, b).  blockIdx.y strides over the PAIRS, blockIdx.x over the words of box a; the workgroup poses both
// pieces.  A pair with an index >= C, or whose a is skipped, keeps its zero record; with b skipped only `posed` is counted.
// Width of the sums.  As in k_contacts a word adds at most 32 to a count or a normal and less than 2^16 to a sum of c, and the
// grid is posed_grid's with the pairs for the pieces: blockIdx.y takes at most 4096 rows, so a pair's box a -- at most all of
// 1024^3, 512 * 512 * 129 < 2^25.02 words -- is shared by at least 16384 / 4096 = 4 workgroups = 1024 lanes (or every lane
// has at most one word, where the volume has fewer).  A lane starts from zero for every pair it takes and so adds fewer than
// 2^15.02 words and stays below 2^31.02 in 32 bits, whatever the number of pairs; wave sums, LDS and atomics are 64 bits wide.
__global__ __launch_bounds__(GROUP) void k_pair_contacts(const uint32_t* __restrict__ L, uint32_t lg, const vrc_component* __restrict__ records, uint32_t C,
                                                         const uint8_t* __restrict__ keep, const vrc_affine* __restrict__ maps, const uint32_t* __restrict__ boxes,
                                                         const uint32_t* __restrict__ pairs, uint32_t n_pairs, uint32_t Sd, unsigned long long* out)
{
    __shared__ unsigned long long part[WAVES][CONTACT_SUMS];
    const uint32_t n = Sd >> 1, Ss = 2u << lg;
    for (uint32_t pair = blockIdx.y; pair < n_pairs; pair += gridDim.y) {       // uniform for the workgroup, and so is all that skips a pair
        const uint32_t a = pairs[2u * (size_t)pair], b = pairs[2u * (size_t)pair + 1u];
        if (a >= C || b >= C) continue;
        Posed sa, sb;
        if (!pose_piece(records, a, keep, maps, boxes, Sd, Ss, sa)) continue;
        const bool other = pose_piece(records, b, keep, maps, boxes, Sd, Ss, sb);
        uint32_t acc[CONTACT_SUMS];
        for (uint32_t k = 0; k < CONTACT_SUMS; ++k) acc[k] = 0u;
        for (uint64_t base = (uint64_t)blockIdx.x * GROUP; base < sa.b.items; base += (uint64_t)gridDim.x * GROUP) {     // uniform trip count
            const uint64_t it = base + threadIdx.x;
            RowWord r;
            if (it < sa.b.items && row_word(sa.b, n, it, r)) {
                const uint32_t bits = posed_word(L, lg, a, sa, r, ~0u);
                if (bits) {                                             // almost no word of a generous box gets here
                    if (other) pair_word(L, lg, b, sb, n, r, bits, acc);
                    else acc[0] += __popc(bits);
                }
            }
        }
        contact_flush(acc, part, out + (size_t)CONTACT_WORDS * pair);
    }
}

// ---- clearance: a field read at the voxels of every posed piece ------------------------------------------------

// While k_clearance runs, a record holds the packed minimum at byte 24 (min_value, min_at[0]) and the packed maximum at byte
// 40 (max_value, max_at[0]); k_clearance_begin puts the identities there, k_clearance_end decodes them in place.
constexpr uint32_t CLEAR_POSED = 0, CLEAR_NONE = 1, CLEAR_SUM = 2, CLEAR_MIN = 3, CLEAR_MAX = 5;     // 64-bit words of the record
constexpr uint32_t CLEAR_PARTS = 5, CLEAR_WORDS = 8;
constexpr unsigned long long NO_MIN = ~0ull, NO_MAX = 0ull;          // no finite value: a packed word of a real voxel is neither

static_assert(sizeof(vrc_piece_clearance) == CLEAR_WORDS * 8u, "vrc_piece_clearance is eight 64-bit words");
static_assert(offsetof(vrc_piece_clearance, min_value) == CLEAR_MIN * 8u && offsetof(vrc_piece_clearance, max_value) == CLEAR_MAX * 8u,
              "the packed minimum and maximum lie where min_value and max_value do");

// What a lane knows of the field over the voxels it gathered for one piece.  lo = (value << 32) | index: the least value, and
// among equals the smallest dense index; hi = (value << 32) | ~index: the greatest value, and among equals the smallest
// dense index again (decode_argmax of vrc_snapshots.hip reads the same form).  VRC_DISTANCE_NONE enters neither.
struct Clearance {
    uint32_t posed, none;
    unsigned long long sum, lo, hi;
};

// the gathered bits of word r, one load of the field each.  Bit 4 zl + 2 y + x is voxel (2 cx + x, 2 cy + y, z0 + zl), z0 the
// z of the word's first layer: in a field of 4^3 (n = 2), where two brick rows share a word, z0 is -4 for the row in the
// word's upper half -- the set bits lie in the row's own half, so z0 + zl is 0..3 there too (posed_word takes the same z0).
__device__ __forceinline__ void clearance_word(const uint32_t* __restrict__ field, uint32_t Sd, const RowWord& r, uint32_t bits, Clearance& c)
{
    const int32_t z0 = 2 * (int32_t)((int64_t)(4u * r.w) - (int64_t)r.base);
    const uint32_t corner = (2u * r.cx * Sd + 2u * r.cy) * Sd + (uint32_t)z0;          // modulo 2^32: whole again with zl added
    c.posed += __popc(bits);
    while (bits) {
        const uint32_t bit = (uint32_t)__ffs((int)bits) - 1u;
        bits &= bits - 1u;
        const uint32_t index = corner + ((bit & 1u) ? Sd * Sd : 0u) + ((bit & 2u) ? Sd : 0u) + (bit >> 2);
        const uint32_t v = field[index];
        if (v == VRC_DISTANCE_NONE) { ++c.none; continue; }
        c.sum += v;
        const unsigned long long lo = ((unsigned long long)v << 32) | index, hi = ((unsigned long long)v << 32) | (uint32_t)~index;
        c.lo = lo < c.lo ? lo : c.lo;
        c.hi = hi > c.hi ? hi : c.hi;
    }
}

// the 64-bit minimum / maximum of a wave by shuffles of the two 32-bit halves
template <bool MAX>
__device__ __forceinline__ unsigned long long wave_extreme(unsigned long long v)
{
    for (int o = 32; o; o >>= 1) {
        const uint32_t up = __shfl_xor((uint32_t)(v >> 32), o), down = __shfl_xor((uint32_t)v, o);
        const unsigned long long other = ((unsigned long long)up << 32) | down;
        v = (MAX ? other > v : other < v) ? other : v;
    }
    return v;
}

// contact_flush for a Clearance: wave reductions, the four waves meet in LDS, and lanes 0..4 issue what is not an identity --
// three 64-bit vector atomic adds, one atomicMin, one atomicMax, at most.  Called by the whole workgroup; one that gathered
// nothing for the piece issues nothing.  The first barrier also keeps the LDS of the record before until its readers are done.
__device__ __forceinline__ void clearance_flush(const Clearance& c, unsigned long long (*part)[CLEAR_PARTS], unsigned long long* record)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (!__syncthreads_or(c.posed != 0u)) return;
    const bool some = __ballot(c.posed != 0u) != 0ull;                  // wave-uniform
    const unsigned long long posed = some ? wave_sum((unsigned long long)c.posed) : 0ull, none = some ? wave_sum((unsigned long long)c.none) : 0ull;
    const unsigned long long sum = some ? wave_sum(c.sum) : 0ull;
    const unsigned long long lo = some ? wave_extreme<false>(c.lo) : NO_MIN, hi = some ? wave_extreme<true>(c.hi) : NO_MAX;
    if (lane == 0u) {
        part[wave][0] = posed; part[wave][1] = none; part[wave][2] = sum; part[wave][3] = lo; part[wave][4] = hi;
    }
    __syncthreads();
    if (threadIdx.x >= CLEAR_PARTS) return;
    const uint32_t k = threadIdx.x;
    unsigned long long v = part[0][k];
    for (uint32_t wv = 1; wv < WAVES; ++wv) {
        const unsigned long long o = part[wv][k];
        v = k < 3u ? v + o : k == 3u ? (o < v ? o : v) : (o > v ? o : v);
    }
    if (k == 0u) { if (v) atomicAdd(record + CLEAR_POSED, v); }
    else if (k == 1u) { if (v) atomicAdd(record + CLEAR_NONE, v); }
    else if (k == 2u) { if (v) atomicAdd(record + CLEAR_SUM, v); }
    else if (k == 3u) { if (v != NO_MIN) atomicMin(record + CLEAR_MIN, v); }
    else if (v != NO_MAX) atomicMax(record + CLEAR_MAX, v);
}

// one thread per record: the identities of the five reductions, every other byte 0
__global__ __launch_bounds__(GROUP) void k_clearance_begin(unsigned long long* out, uint32_t C)
{
    const uint32_t i = blockIdx.x * GROUP + threadIdx.x;
    if (i >= C) return;
    for (uint32_t k = 0; k < CLEAR_WORDS; ++k) out[(size_t)CLEAR_WORDS * i + k] = k == CLEAR_MIN ? NO_MIN : 0ull;
}

// one thread per record: the two packed words become min_value / min_at and max_value / max_at in place.  No finite value:
// VRC_DISTANCE_NONE at 0,0,0 and 0 at 0,0,0.  depth: of the field.
__global__ __launch_bounds__(GROUP) void k_clearance_end(unsigned long long* out, uint32_t C, uint32_t depth)
{
    const uint32_t i = blockIdx.x * GROUP + threadIdx.x;
    if (i >= C) return;
    unsigned long long* words = out + (size_t)CLEAR_WORDS * i;
    const unsigned long long lo = words[CLEAR_MIN], hi = words[CLEAR_MAX];
    const uint32_t mask = (1u << depth) - 1u;
    const uint32_t at_lo = lo == NO_MIN ? 0u : (uint32_t)lo, at_hi = hi == NO_MAX ? 0u : ~(uint32_t)hi;
    // value, x in one word and y, z in the next, low half first; NO_MIN gives VRC_DISTANCE_NONE, NO_MAX gives 0
    words[CLEAR_MIN] = (lo >> 32) | ((unsigned long long)(at_lo >> (2u * depth)) << 32);
    words[CLEAR_MIN + 1u] = ((at_lo >> depth) & mask) | ((unsigned long long)(at_lo & mask) << 32);
    words[CLEAR_MAX] = (hi >> 32) | ((unsigned long long)(at_hi >> (2u * depth)) << 32);
    words[CLEAR_MAX + 1u] = ((at_hi >> depth) & mask) | ((unsigned long long)(at_hi & mask) << 32);
}

// k_contacts with a field for a world: where that kernel calls contact_word, this one reads the field at the gathered bits.
// Width of the sums.  A lane takes fewer than 2^15.02 words of a piece (k_contacts), so at most 2^20.02 voxels: the two counts
// fit 32 bits; a finite value is below 2^30 (a travel field; below 2^22 for a Euclidean one), so the sum is 64 bits wide from
// the lane on.  Minimum and maximum do not depend on the order they are taken in, sums of integers neither.
__global__ __launch_bounds__(GROUP) void k_clearance(const uint32_t* __restrict__ L, uint32_t lg, const vrc_component* __restrict__ records, uint32_t C,
                                                     const uint8_t* __restrict__ keep, const vrc_affine* __restrict__ maps, const uint32_t* __restrict__ boxes,
                                                     const uint32_t* __restrict__ field, uint32_t Sd, unsigned long long* out)
{
    __shared__ unsigned long long part[WAVES][CLEAR_PARTS];
    const uint32_t n = Sd >> 1, Ss = 2u << lg;
    for (uint32_t piece = blockIdx.y; piece < C; piece += gridDim.y) {  // uniform for the workgroup, and so is all that skips a piece
        Posed s;
        if (!pose_piece(records, piece, keep, maps, boxes, Sd, Ss, s)) continue;
        Clearance c = {0u, 0u, 0ull, NO_MIN, NO_MAX};
        for (uint64_t base = (uint64_t)blockIdx.x * GROUP; base < s.b.items; base += (uint64_t)gridDim.x * GROUP) {      // uniform trip count
            const uint64_t it = base + threadIdx.x;
            RowWord r;
            if (it < s.b.items && row_word(s.b, n, it, r)) {
                const uint32_t bits = posed_word(L, lg, piece, s, r, ~0u);
                if (bits) clearance_word(field, Sd, r, bits, c);        // almost no word of a generous box gets here
            }
        }
        clearance_flush(c, part, out + (size_t)CLEAR_WORDS * piece);
    }
}

// ---- the broad phase: which boxes come near each other -----------------------------------------------------------

// box i of the table clipped to the posed volume; false: the piece has no pairs (keep[i] == 0, an empty or inverted box)
__device__ __forceinline__ bool pair_box(const uint8_t* __restrict__ keep, const uint32_t* __restrict__ boxes, uint32_t i, uint32_t Sd, uint32_t lo[3], uint32_t hi[3])
{
    if (keep && keep[i] == 0) return false;
    return clip_box(boxes + 6u * (size_t)i, Sd, lo, hi);
}

// One thread per a walks all b: C^2 box tests.  b is uniform for the wave, so box b and keep[b] come through wave-uniform
// loads and every lane compares them with a box of its own in registers.  The count pass (EMIT false) stores how many b are
// candidates of a in slots[a]; k_scan_slots turns the counts into offsets with the total in slots[C]; the emit pass runs
// the same loop and writes entry slots[a] + j of the canonical list -- (a, b) ascending -- where it falls into
// [first, first + want).  first + want <= the total.
template <bool EMIT>
__global__ __launch_bounds__(GROUP) void k_box_pairs(const uint8_t* __restrict__ keep, const uint32_t* __restrict__ boxes, uint32_t C, uint32_t Sd,
                                                     unsigned long long* __restrict__ slots, unsigned long long first, unsigned long long want,
                                                     uint32_t* __restrict__ pairs)
{
    const uint32_t a = blockIdx.x * GROUP + threadIdx.x;
    uint32_t alo[3] = {0u, 0u, 0u}, ahi[3] = {0u, 0u, 0u};
    bool live = a < C && pair_box(keep, boxes, a, Sd, alo, ahi);
    unsigned long long at = 0ull;
    if (EMIT && live) {
        at = slots[a];
        live = at < first + want && slots[a + 1u] > first;             // a's run meets the window
    }
    if (EMIT && !__syncthreads_or(live)) return;
    uint32_t found = 0u;
    for (uint32_t b = 0; b < C; ++b) {                                  // uniform
        uint32_t blo[3], bhi[3];
        if (!pair_box(keep, boxes, b, Sd, blo, bhi)) continue;
        bool near = live && a != b;
        for (int x = 0; x < 3; ++x) near = near && alo[x] <= bhi[x] && blo[x] <= ahi[x];        // hi exclusive: box a meets box b grown by one voxel
        if (!near) continue;
        if (EMIT) {
            const unsigned long long e = at + found;
            if (e >= first && e - first < want) {
                pairs[2u * (e - first)] = a;
                pairs[2u * (e - first) + 1u] = b;
            }
        }
        ++found;
    }
    if (!EMIT && a < C) slots[a] = found;
}

}  // namespace

namespace vrc {

hipError_t moments_run(const uint32_t* labels, uint32_t depth, uint64_t first, uint64_t want, vrc_piece_moments* out, hipStream_t st)
{
    const hipError_t e = hipMemsetAsync(out, 0, (size_t)want * sizeof(vrc_piece_moments), st);
    if (e != hipSuccess) return e;
    const uint32_t n_keys = 1u << (3u * depth);
    hipLaunchKernelGGL(k_moments, dim3((n_keys + GROUP_KEYS - 1u) / GROUP_KEYS), dim3(GROUP), 0, st, depth - 1u, n_keys, labels, (uint32_t)first, (uint32_t)want,
                       (unsigned long long*)out);
    return hipGetLastError();
}

// the grid of the two kernels that gather posed pieces: about 16384 workgroups in all: the more pieces, the fewer workgroups
// share a piece's box; the rest is the strides.  A piece has at least 4 workgroups unless the destination has fewer words.
static dim3 posed_grid(uint64_t pieces, uint32_t Sd)
{
    const uint32_t zero[3] = {0u, 0u, 0u}, all[3] = {Sd, Sd, Sd};
    const uint32_t gy = pieces > 4096u ? 4096u : (uint32_t)pieces;
    const uint64_t whole = (box_word_items(zero, all) + GROUP - 1u) / GROUP;
    const uint32_t share = 16384u / gy;
    return dim3(whole < share ? (uint32_t)whole : share, gy);
}

void place_affine_run(const uint32_t* labels, const vrc_component* records, uint64_t pieces, uint32_t depth, const uint8_t* keep, const vrc_affine* maps,
                      const uint32_t* boxes, uint32_t* dst, uint32_t dst_depth, int op, hipStream_t st)
{
    const uint32_t Sd = 1u << dst_depth;
    hipLaunchKernelGGL(k_place_affine, posed_grid(pieces, Sd), dim3(GROUP), 0, st, labels, depth - 1u, records, (uint32_t)pieces, keep, maps, boxes, dst, Sd, op);
}

hipError_t contacts_run(const uint32_t* labels, const vrc_component* records, uint64_t pieces, uint32_t depth, const uint8_t* keep, const vrc_affine* maps,
                        const uint32_t* boxes, const uint32_t* world, uint32_t world_depth, vrc_piece_contact* out, hipStream_t st)
{
    const hipError_t e = hipMemsetAsync(out, 0, (size_t)pieces * sizeof(vrc_piece_contact), st);
    if (e != hipSuccess) return e;
    const uint32_t Sd = 1u << world_depth;
    hipLaunchKernelGGL(k_contacts, posed_grid(pieces, Sd), dim3(GROUP), 0, st, labels, depth - 1u, records, (uint32_t)pieces, keep, maps, boxes, world, Sd,
                       (unsigned long long*)out);
    return hipGetLastError();
}

hipError_t pair_contacts_run(const uint32_t* labels, const vrc_component* records, uint64_t pieces, uint32_t depth, const uint8_t* keep, const vrc_affine* maps,
                             const uint32_t* boxes, uint32_t posed_depth, uint64_t n_pairs, const uint32_t* pairs, vrc_piece_contact* out, hipStream_t st)
{
    const hipError_t e = hipMemsetAsync(out, 0, (size_t)n_pairs * sizeof(vrc_piece_contact), st);
    if (e != hipSuccess) return e;
    const uint32_t Sd = 1u << posed_depth;
    hipLaunchKernelGGL(k_pair_contacts, posed_grid(n_pairs, Sd), dim3(GROUP), 0, st, labels, depth - 1u, records, (uint32_t)pieces, keep, maps, boxes, pairs,
                       (uint32_t)n_pairs, Sd, (unsigned long long*)out);
    return hipGetLastError();
}

hipError_t clearance_run(const uint32_t* labels, const vrc_component* records, uint64_t pieces, uint32_t depth, const uint8_t* keep, const vrc_affine* maps,
                         const uint32_t* boxes, const uint32_t* field, uint32_t field_depth, vrc_piece_clearance* out, hipStream_t st)
{
    const uint32_t Sd = 1u << field_depth, C = (uint32_t)pieces;
    const dim3 per_record((C + GROUP - 1u) / GROUP);
    hipLaunchKernelGGL(k_clearance_begin, per_record, dim3(GROUP), 0, st, (unsigned long long*)out, C);
    hipLaunchKernelGGL(k_clearance, posed_grid(pieces, Sd), dim3(GROUP), 0, st, labels, depth - 1u, records, C, keep, maps, boxes, field, Sd,
                       (unsigned long long*)out);
    hipLaunchKernelGGL(k_clearance_end, per_record, dim3(GROUP), 0, st, (unsigned long long*)out, C, field_depth);
    return hipGetLastError();
}

size_t box_pair_scratch_bytes(uint64_t pieces) { return (size_t)(pieces + 1u) * 8u; }

void box_pair_count_run(const uint8_t* keep, const uint32_t* boxes, uint64_t pieces, uint32_t posed_depth, unsigned long long* slots, hipStream_t st)
{
    const uint32_t C = (uint32_t)pieces;
    hipLaunchKernelGGL(k_box_pairs<false>, dim3((C + GROUP - 1u) / GROUP), dim3(GROUP), 0, st, keep, boxes, C, 1u << posed_depth, slots, 0ull, 0ull, (uint32_t*)nullptr);
    // a slot is below C <= BOX_PAIR_PIECES = 2^20 and the 1024 slots of a step sum to less than 2^30, as scan_slots wants them
    hipLaunchKernelGGL(k_scan_slots<unsigned long long>, dim3(1), dim3(SCAN_GROUP), 0, st, slots, C, (unsigned long long*)nullptr);
}

void box_pairs_run(const uint8_t* keep, const uint32_t* boxes, uint64_t pieces, uint32_t posed_depth, unsigned long long* slots, uint64_t first, uint64_t want,
                   uint32_t* pairs, hipStream_t st)
{
    const uint32_t C = (uint32_t)pieces;
    hipLaunchKernelGGL(k_box_pairs<true>, dim3((C + GROUP - 1u) / GROUP), dim3(GROUP), 0, st, keep, boxes, C, 1u << posed_depth, slots, (unsigned long long)first,
                       (unsigned long long)want, pairs);
}

}  // namespace vrc
