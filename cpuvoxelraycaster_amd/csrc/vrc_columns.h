// vrc_columns.h -- the occupancy looked at and written along an axis (vrc_columns.hip): the profile of every column of a
// rectangle of a face, the fill of every column's span from two height maps, and the selection by the count of solid voxels
// met before a voxel, as vrc_volume_ops.hip calls them.  Like vrc_fall.h it knows arrays only; volumes, their ordering and
// the staging of the caller's lists stay with the entry points.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vrc.h"

namespace vrc {

// rect = (u_lo, v_lo, u_hi, v_hi) of the face across `axis`, non-empty and inside [0, S]^2, (u, v) the other two axes in
// x < y < z order; the maps of a rect are dense (u_hi - u_lo) x (v_hi - v_lo) arrays.  direction = 2 * axis + side as in
// vrc_fall.h.

// out[(u - u_lo) * (v_hi - v_lo) + (v - v_lo)] = the record of column (u, v) of the word field `words` (include/vrc.h:
// vrc_columns_profile).  Every record of the rect is written once, by plain stores.  One kernel on `st`.
void columns_profile_run(const uint32_t* words, uint32_t depth, int direction, const uint32_t rect[4], vrc_column* out, hipStream_t st);
// every column of the rect takes (op) its span [lo, hi) along `axis`: lo from lo_map (nullptr: lo_const), hi from hi_map
// (nullptr: hi_const), both clamped to [0, S]; under VRC_COPY_REPLACE the rest of the column is cleared.  One kernel on `st`.
void columns_fill_run(uint32_t* words, uint32_t depth, int axis, const uint32_t rect[4], const int32_t* lo_map, int32_t lo_const,
                      const int32_t* hi_map, int32_t hi_const, int op, hipStream_t st);
// dst takes (op) the voxels p of src with lo <= P(p) < hi that are solid (of & VRC_COLUMNS_SOLID) or empty (of &
// VRC_COLUMNS_EMPTY), P(p) the solid voxels before p along the direction; lo <= hi <= S + 1; the two fields do not overlap.
// Every word of dst has one owner.  One kernel on `st`.
void columns_select_run(uint32_t* dst, const uint32_t* src, uint32_t depth, int direction, uint32_t lo, uint32_t hi, int of, int op,
                        hipStream_t st);

}  // namespace vrc
