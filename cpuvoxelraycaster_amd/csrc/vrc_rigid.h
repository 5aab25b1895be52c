// vrc_rigid.h -- what a physics engine needs of the pieces of a labelling, and what it hands back (vrc_rigid.hip), as
// vrc_snapshots.hip calls them: the raw moments of every piece, the gather that writes every piece through its own
// inverse affine map, the same gather ending in the contact record of every posed piece against a world or, pair by pair,
// against another posed piece, and the broad phase that lists the pairs worth asking about.  Like vrc_fall.h it knows arrays only; volumes, their ordering, the staging of host memory and the
// argument checks stay with the entry points.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vrc.h"

namespace vrc {

// the limits of a map (vrc.h: vrc_volume_stamp_affine): the entry points refuse what the host can read, the kernel drops the
// piece whose map it finds beyond them
constexpr int32_t AFFINE_M_LIMIT = 1 << 20;
constexpr int64_t AFFINE_T_LIMIT = 1ll << 40;

// out[k] = the moments of piece first + k, k < want, of `labels` (8^depth ids by key); first + want <= the number of pieces.
// Zeroes out[0 .. want) and accumulates into it in ONE pass over the ids; no scratch.  out is DEVICE memory.  Enqueues on `st`.
hipError_t moments_run(const uint32_t* labels, uint32_t depth, uint64_t first, uint64_t want, vrc_piece_moments* out, hipStream_t st);

// for every piece i < pieces with keep[i] != 0 (keep == nullptr: all) and every voxel p of dst in box i (boxes: pieces x 6,
// lo then hi, clipped to dst; nullptr: all of dst): with q = (maps[i] (2p + 1)) >> 17, dst(p) is set (VRC_COPY_OR) or cleared
// (VRC_COPY_ANDNOT) iff labels(q) == i.  `records` are the labels' own: a piece's box bounds what is loaded.  A piece whose
// map lies beyond the limits is dropped whole.  keep, maps and boxes are DEVICE memory.  One kernel, no scratch: a 2-D grid,
// blockIdx.y striding over the pieces and blockIdx.x over the words of a piece's box.  Enqueues on `st`.  pieces >= 1.
void place_affine_run(const uint32_t* labels, const vrc_component* records, uint64_t pieces, uint32_t depth, const uint8_t* keep,
                      const vrc_affine* maps, const uint32_t* boxes, uint32_t* dst, uint32_t dst_depth, int op, hipStream_t st);

// out[i] = the contact record (vrc.h: vrc_rigid_contacts) of piece i < pieces against `world` (8^world_depth voxels as
// occupancy words, only read): the voxels place_affine_run would set with the same keep, maps and boxes -- one copy of the
// gather serves both -- counted, and those inside a solid voxel of the world (overlap) or face to face with one or with the
// volume's faces (touch) summed with their centres and normals.  Zeroes out[0 .. pieces) and adds into it in ONE kernel of
// place_affine_run's grid; a skipped piece keeps its zero record.  keep, maps, boxes and out are DEVICE memory; no scratch.
// Enqueues on `st`.  pieces >= 1.
hipError_t contacts_run(const uint32_t* labels, const vrc_component* records, uint64_t pieces, uint32_t depth, const uint8_t* keep,
                        const vrc_affine* maps, const uint32_t* boxes, const uint32_t* world, uint32_t world_depth, vrc_piece_contact* out, hipStream_t st);

// out[k] = the contact record (vrc.h: vrc_rigid_pair_contacts) of posed piece pairs[2k] against posed piece pairs[2k + 1],
// k < n_pairs < 2^32: A_a as contacts_run gathers it, against A_b gathered the same way in place of a world and with no
// walls -- a neighbour beyond the posed volume (8^posed_depth voxels) or beyond box b reads 0.  Zeroes out[0 .. n_pairs) and
// adds into it in ONE kernel of contacts_run's shape with the pairs for the pieces; a pair with an index >= pieces, or whose
// a is skipped, keeps its zero record.  keep, maps, boxes, pairs and out are DEVICE memory; no scratch.  Enqueues on `st`.
// pieces >= 1, n_pairs >= 1.
hipError_t pair_contacts_run(const uint32_t* labels, const vrc_component* records, uint64_t pieces, uint32_t depth, const uint8_t* keep,
                             const vrc_affine* maps, const uint32_t* boxes, uint32_t posed_depth, uint64_t n_pairs, const uint32_t* pairs,
                             vrc_piece_contact* out, hipStream_t st);

// out[i] = the clearance record (vrc.h: vrc_rigid_clearance) of piece i < pieces over `field` (8^field_depth uint32 values as
// [(x*S + y)*S + z], only read): the voxels contacts_run would count as `posed` with the same keep, maps and boxes -- the one
// gather again -- counted, and the field's values there summed, with their least and greatest finite value and the voxels of
// smallest dense index that hold them.  Three kernels on `st`: one thread per record writes the reductions' identities, the
// gather kernel of contacts_run's grid reduces into the records with 64-bit vector atomics (add, min, max), one thread per
// record decodes the packed minimum and maximum in place.  A skipped piece gets the record of the empty set.  keep, maps,
// boxes and out are DEVICE memory; no scratch.  pieces >= 1, field_depth in 2..10.
hipError_t clearance_run(const uint32_t* labels, const vrc_component* records, uint64_t pieces, uint32_t depth, const uint8_t* keep,
                         const vrc_affine* maps, const uint32_t* boxes, const uint32_t* field, uint32_t field_depth, vrc_piece_clearance* out, hipStream_t st);

// The broad phase (vrc.h: vrc_rigid_box_pair_count / vrc_rigid_box_pairs): the ordered pairs (a, b), a != b, of kept pieces
// whose boxes (pieces x 6, clipped to the posed volume; required) meet when one is grown by a voxel, ascending.  A thread per
// a walks all b -- pieces^2 box tests, hence the limit on the pieces.  `slots` is the scratch of both calls,
// box_pair_scratch_bytes(pieces) = (pieces + 1) x 8 bytes.  box_pair_count_run fills it: the count of every a, scanned into
// offsets, and the total in slots[pieces].  box_pairs_run, behind it on the same stream, writes the entries
// [first, first + want) of the list to pairs[0 .. 2 want); first + want <= the total.  keep, boxes and pairs are DEVICE
// memory.  Both enqueue on `st`.  1 <= pieces <= BOX_PAIR_PIECES.
constexpr uint64_t BOX_PAIR_PIECES = 1ull << 20;
size_t box_pair_scratch_bytes(uint64_t pieces);
void box_pair_count_run(const uint8_t* keep, const uint32_t* boxes, uint64_t pieces, uint32_t posed_depth, unsigned long long* slots, hipStream_t st);
void box_pairs_run(const uint8_t* keep, const uint32_t* boxes, uint64_t pieces, uint32_t posed_depth, unsigned long long* slots, uint64_t first, uint64_t want,
                   uint32_t* pairs, hipStream_t st);

}  // namespace vrc
