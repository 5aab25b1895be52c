// vrc_delta.h -- the difference of two brick-word fields as a list of changed words (vrc_delta.hip), as vrc_snapshots.hip
// calls it.  The kernels know word arrays and record lists only; volumes, their ordering and the delta object stay with
// vrc_snapshots.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vrc {

// What the passes reduce, at the front of the scratch block.  delta_totals_reset puts lo and first_bad to ~0 and the rest to
// 0; lo / hi are the box of the changed voxels (hi exclusive), meaningless while voxels == 0.
struct DeltaTotals {
    uint32_t lo[3];
    uint32_t first_bad;               // delta_check_run: the least index of a record that breaks the rule, ~0 = none
    uint32_t hi[3];
    uint32_t words;                   // delta_offsets_run: the number of records
    unsigned long long voxels;        // the sum of popcount(bits)
    unsigned long long pad;
};
static_assert(sizeof(DeltaTotals) == 48, "the slots behind it start on a multiple of 16 bytes");

// the words of a field at `depth`: 8^depth / 32
inline uint32_t delta_words(uint32_t depth) { return 1u << (3u * depth - 5u); }
// Bytes of the scratch block of a diff at `depth`: the totals, then one 32-bit slot per workgroup of 256 words and one for
// the total behind them -- 1/256 of the occupancy + 52 bytes from depth 4 up (512 KiB at depth 10, 64 KiB at depth 9).
// delta_check_run needs the totals alone.
size_t delta_scratch_bytes(uint32_t depth);
void delta_totals_reset(DeltaTotals* totals, hipStream_t st);
// passes 1 and 2 over before ^ after: the totals (reset here first), every workgroup's exclusive record offset into its slot
// and the number of records into totals->words.  Two kernels on `st`.
void delta_offsets_run(const uint32_t* before, const uint32_t* after, uint32_t depth, void* scratch, hipStream_t st);
// pass 3, after delta_offsets_run on the same stream: the records {word, bits} in ascending word order to records[0 .. words)
void delta_emit_run(const uint32_t* before, const uint32_t* after, uint32_t depth, const void* scratch, uint2* records, hipStream_t st);
// n <= 2^25 + 1 caller records held to the rule (word strictly ascending and below the words of `depth`, bits != 0):
// totals->first_bad, and the voxels and the box of the list (reset here first).  One kernel on `st`.
void delta_check_run(const uint2* records, uint32_t n, uint32_t depth, DeltaTotals* totals, hipStream_t st);
// words[record.word] ^= record.bits for n records with distinct words below the field's size.  One kernel on `st`.
void delta_apply_run(const uint2* records, uint32_t n, uint32_t* words, hipStream_t st);

}  // namespace vrc
