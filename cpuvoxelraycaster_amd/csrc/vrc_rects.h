// vrc_rects.h -- the exposed faces of a brick-word field merged into rectangles (vrc_rects.hip), as vrc_volume.hip calls
// it.  Like the surface extractor it knows word arrays only; volumes, their ordering, staging and scratch memory stay with
// vrc_volume.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vrc {

// Bytes of the block at `depth`, with S = 2^depth, w = max(1, S / 32) the 32-bit words of a row and L = 6 S^2 w the lanes
// (one per direction, plane, row and word):  8 * (ceil(L / 256) + 7)  for the offsets -- one 64-bit slot per workgroup of
// 256 lanes, one for the total behind them, six for the per-direction totals --  plus  2 * 4 * S^2 * w  for the two row
// bit fields: 32 MiB + 768 KiB + 56 bytes at depth 9, 256 MiB + 6 MiB + 56 at depth 10.
size_t rect_scratch_bytes(uint32_t depth);
// where in the block the total and the six per-direction totals lie
unsigned long long* rect_total_slot(unsigned long long* scratch, uint32_t depth);
unsigned long long* rect_direction_slots(unsigned long long* scratch, uint32_t depth);
// the brick words as the two row bit fields of the block.  One kernel on `st`; every later pass reads the fields only.
void rect_rows_run(const uint32_t* words, uint32_t depth, unsigned long long* scratch, hipStream_t st);
// after rect_rows_run: the six per-direction totals into rect_direction_slots (zeroed here first).  One kernel on `st`.
void rect_count_run(uint32_t depth, int closed, unsigned long long* scratch, hipStream_t st);
// after rect_rows_run: every workgroup's exclusive rectangle offset into its slot, the total into rect_total_slot and,
// where it is not NULL, into the device word d_total.  Two kernels on `st`.
void rect_offsets_run(uint32_t depth, int closed, unsigned long long* scratch, unsigned long long* d_total, hipStream_t st);
// after rect_offsets_run with the same `closed`: rectangles [first, first + capacity) of the canonical order to out[0 ..]
// in `format` (include/vrc.h: VRC_SURFACE_*).  One kernel on `st`.
void rect_emit_run(uint32_t depth, int closed, int format, uint64_t first, uint64_t capacity, void* out, const unsigned long long* scratch,
                   hipStream_t st);

}  // namespace vrc
