// vrc_build_grids.h -- the per-level grids of the device builder (vrc_build_sweeps.h) as a type of its own: the editable
// volume keeps one between commits (vrc_volume_state.h), and not every file that handles a volume takes in the builder.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vrc.h"

// The per-level count / rank / index grids of one build.  Levels 0 .. N-2 share one allocation; the bottom level (7/8
// of all cells: 1.6 GB at depth 10) gets three of its own -- one multi-GB hipMalloc costs ~100 ms where the same bytes
// in a few pieces cost 2 ms.  A one-shot build allocates and frees them; an editable volume keeps them between commits.
struct BuildGrids {
    uint32_t depth = 0;
    uint32_t* arena = nullptr;
    uint32_t *cnt[VRC_MAX_DEPTH] = {}, *rank[VRC_MAX_DEPTH] = {}, *index[VRC_MAX_DEPTH] = {};

    hipError_t alloc(uint32_t N)
    {
        depth = N;
        uint64_t total_cells = 0;
        for (uint32_t L = 0; L + 1 < N; ++L) total_cells += 1ull << (3 * L);
        hipError_t e = hipMalloc((void**)&arena, (total_cells ? total_cells : 1) * 12);
        if (e != hipSuccess) return e;
        uint64_t off = 0;
        for (uint32_t L = 0; L + 1 < N; ++L) {
            const uint64_t cells = 1ull << (3 * L);
            cnt[L] = arena + off; rank[L] = arena + total_cells + off; index[L] = arena + 2 * total_cells + off;
            off += cells;
        }
        const uint64_t bottom = 1ull << (3 * (N - 1));
        if ((e = hipMalloc((void**)&cnt[N - 1], bottom * 4)) != hipSuccess) return e;
        if ((e = hipMalloc((void**)&rank[N - 1], bottom * 4)) != hipSuccess) return e;
        return hipMalloc((void**)&index[N - 1], bottom * 4);
    }
    void release()
    {
        if (arena) (void)hipFree(arena);
        if (depth) { (void)hipFree(cnt[depth - 1]); (void)hipFree(rank[depth - 1]); (void)hipFree(index[depth - 1]); }
        *this = BuildGrids();
    }
    bool allocated() const { return depth != 0 && index[depth - 1] != nullptr; }
};
