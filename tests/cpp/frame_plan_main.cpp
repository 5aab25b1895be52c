// The frame launch planner (csrc/vrc_plan.h) over cases from stdin, against the kernel table of the built libvrc_hip.so.
// No HIP call: runs without a device.  One case per line, 21 integers (tools/frame_plan_cases.py names them); one line out:
//   rc kernel grid lds n_items sample_chunk sample_chunk_tail tail_tiles checker_wide spp row_block shard_index shard_count
// ("0 - 0 ..." when there is nothing to launch, "rc error: <vrc_last_error>" when the planner refuses).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../cpuvoxelraycaster_amd/csrc/vrc_plan.h"

int main()
{
    char line[512];
    while (fgets(line, sizeof(line), stdin)) {
        long long v[21];
        int n = 0;
        for (char* q = line; n < 21; ++n) {
            char* e;
            v[n] = strtoll(q, &e, 10);
            if (e == q) break;
            q = e;
        }
        if (n == 0) continue;
        if (n != 21) { fprintf(stderr, "bad case line: %s", line); return 2; }
        vrc::PlanInput in;
        memset(&in.cam, 0, sizeof(in.cam));
        memset(&in.p, 0, sizeof(in.p));
        in.cam.rot[0] = in.cam.rot[4] = in.cam.rot[8] = 1.0f; in.cam.fov = 1.0f;
        in.cam.aperture = v[0] ? 0.0f : 0.5f; in.cam.focal_length = v[0] ? 1.0f : 60.0f;
        in.p.gi_bounces = (uint32_t)v[1]; in.p.use_samples = (uint32_t)v[2]; in.p.spp = (uint32_t)v[3]; in.p.checker_parity = (int32_t)v[4];
        in.fused = v[5] != 0; in.capture = v[6] != 0;
        in.width = (uint32_t)v[7]; in.height = (uint32_t)v[8]; in.depth = (uint32_t)v[9];
        in.p.row_block = (uint32_t)v[10]; in.p.shard_index = (uint32_t)v[11]; in.p.shard_count = (uint32_t)v[12];
        in.tuning.blocks_per_cu = (uint32_t)v[13]; in.tuning.blocks_per_cu_set = v[13] != 0; in.tuning.sample_chunk = (uint32_t)v[14];
        in.tuning.tail_units_per_wave = (uint32_t)v[15]; in.tuning.lane_samples = (uint32_t)v[16]; in.tuning.quad_walks = v[17] != 0;
        in.tuning.reuse_invariant = v[18] != 0; in.tuning.walk_from_root = v[19] != 0;
        in.cu_count = (int)v[20];
        vrc::FramePlan f;
        const int rc = vrc::plan_frame(in, f);
        if (rc) printf("%d error: %s\n", rc, vrc_last_error());
        else if (!f.kernel) printf("0 - 0 0 0 0 0 0 0 %u %u %u %u\n", f.p.spp, f.p.row_block, f.p.shard_index, f.p.shard_count);
        else printf("0 %s %u %u %u %u %u %u %u %u %u %u %u\n", f.kernel->name, f.grid, f.lds, f.n_items, f.sample_chunk, f.sample_chunk_tail,
                    f.tail_tiles, f.checker_wide, f.p.spp, f.p.row_block, f.p.shard_index, f.p.shard_count);
    }
    return 0;
}
