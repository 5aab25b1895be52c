// vrc_surface.h -- the exposed faces of a brick-word field as a face / triangle list (vrc_surface.hip), as vrc_volume.hip
// calls it.  The extractor knows word arrays only; volumes, their ordering, staging and scratch memory stay with
// vrc_volume.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vrc {

// Bytes of the offsets block at `depth`: one 64-bit slot per workgroup of 256 words, one for the total T behind them and
// six for the per-direction totals of surface_count -- 8 * (ceil(words / 256) + 7): 1/128 of the occupancy + 56 bytes
// from depth 5 up (1 MiB + 56 bytes at depth 10, 128 KiB + 56 at depth 9), 64 bytes below.
size_t surface_scratch_bytes(uint32_t depth);
// where in the block the total and the six per-direction totals lie
unsigned long long* surface_total_slot(unsigned long long* scratch, uint32_t depth);
unsigned long long* surface_direction_slots(unsigned long long* scratch, uint32_t depth);
// the six per-direction totals into surface_direction_slots (zeroed here first).  One kernel on `st`.
void surface_count_run(const uint32_t* words, uint32_t depth, int closed, unsigned long long* scratch, hipStream_t st);
// passes 1 and 2: every workgroup's exclusive face offset into its slot, T into surface_total_slot and, where it is not
// NULL, into the device word d_total.  Two kernels on `st`.
void surface_offsets_run(const uint32_t* words, uint32_t depth, int closed, unsigned long long* scratch, unsigned long long* d_total,
                         hipStream_t st);
// pass 3, after surface_offsets_run on the same stream: faces [first, first + capacity) of the canonical order to
// out[0 ..] in `format` (include/vrc.h: VRC_SURFACE_*).  One kernel on `st`.
void surface_emit_run(const uint32_t* words, uint32_t depth, int closed, int format, uint64_t first, uint64_t capacity, void* out,
                      const unsigned long long* scratch, hipStream_t st);

}  // namespace vrc
