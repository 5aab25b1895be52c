// vrc_components.h -- connected-component labelling of a brick-word field (vrc_components.hip), as vrc_volume.hip calls it.
// Like the flood it knows word arrays only; volumes, their ordering and every allocation stay with vrc_volume.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vrc.h"

namespace vrc {

// bytes of device scratch a labelling at `depth` needs: the per-workgroup root counts / offsets and their total
size_t components_scratch_bytes(uint32_t depth);
// where the scan leaves C, the number of components (one uint32)
uint32_t* components_total_slot(uint32_t* scratch, uint32_t depth);
// First half: labels[key] = the key of the component's representative for the voxels of M, VRC_NO_COMPONENT elsewhere
// (M = medium for through == 0, its complement inside the volume otherwise); scratch = the exclusive prefix of the
// representatives per workgroup and their total.  labels: 8^depth uint32.  cells, optional (nullptr: none): a dense field
// [(x*S + y)*S + z] of one uint32 per voxel; two neighbours are then joined only if they carry the same value, so the
// components are those of M cut along the cells' borders (vrc_fracture.hip).  Enqueues on `st`.
void components_roots_run(const uint32_t* medium, uint32_t depth, int connectivity, int through, const uint32_t* cells, uint32_t* labels, uint32_t* scratch,
                          hipStream_t st);
// Second half, once the host has read the total and made room for the records: labels[key] = the component's id, and
// records[id] complete.  Enqueues on `st`.
void components_ids_run(uint32_t depth, uint32_t* labels, const uint32_t* scratch, vrc_component* records, hipStream_t st);
// ids[i] = labels at voxel xyz[3i..3i+2], VRC_NO_COMPONENT outside the volume
void components_at_run(const uint32_t* labels, uint32_t depth, uint64_t n, const uint32_t* xyz, uint32_t* ids, hipStream_t st);
// dst (op)= { v : keep[labels[v]] != 0 }, whole words
void components_select_run(const uint32_t* labels, uint32_t depth, const uint8_t* keep, uint32_t* dst, int op, hipStream_t st);

}  // namespace vrc
