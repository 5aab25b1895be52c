// Exercises the surface voxelisation of the C++ host adapter (cpuvoxelraycaster_amd/host/hip_raycaster.hpp) the way a tool that
// paints a model's skin into a world would: the triangles' touched voxels are set in an empty volume
// (HipVoxelVolume::rasterMesh), their thin shell is cleared out of a full one, and an indexed mesh's thin shell is set through
// shellMesh.  Prints the solid count and a hash of the volume's sparse tile stream after each step; the pytest wrapper compares
// them with the numpy model's.
//   usage: voxel_raster_main <depth> <tris.bin: n x 9 int32> <verts.bin: k x 3 float64> <faces.bin: m x 3 uint32> <scale> <offset>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "../../cpuvoxelraycaster_amd/host/hip_raycaster.hpp"

static std::vector<char> slurp(const char* path)
{
    std::ifstream f(path, std::ios::binary);
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static unsigned long long digest(vrc_host::HipVoxelVolume& vol)
{
    unsigned long long hash = 1469598103934665603ull;          // FNV-1a
    for (uint8_t b : vol.pack()) hash = (hash ^ b) * 1099511628211ull;
    return hash;
}

int main(int argc, char** argv)
{
    if (argc != 7) return 2;
    const uint32_t depth = (uint32_t)atoi(argv[1]), S = 1u << depth;
    const std::vector<char> raw_tris = slurp(argv[2]), raw_verts = slurp(argv[3]), raw_faces = slurp(argv[4]);
    const std::vector<int32_t> tris((const int32_t*)raw_tris.data(), (const int32_t*)raw_tris.data() + raw_tris.size() / 36 * 9);
    const std::vector<double> verts((const double*)raw_verts.data(), (const double*)raw_verts.data() + raw_verts.size() / 24 * 3);
    const std::vector<uint32_t> faces((const uint32_t*)raw_faces.data(), (const uint32_t*)raw_faces.data() + raw_faces.size() / 12 * 3);
    const double scale = atof(argv[5]), offset = atof(argv[6]);
    try {
        vrc_host::HipVoxelVolume touched(depth);
        touched.rasterMesh(tris);
        std::printf("triangles=%zu touched=%llu:%016llx", tris.size() / 9, (unsigned long long)touched.solidCount(), digest(touched));
        vrc_host::HipVoxelVolume carved(depth);
        carved.fillBox(0, 0, 0, S, S, S, true);
        carved.rasterMesh(tris, VRC_RASTER_THIN, false);
        std::printf(" carved=%llu:%016llx", (unsigned long long)carved.solidCount(), digest(carved));
        vrc_host::HipVoxelVolume skin(depth);
        skin.shellMesh(verts, faces, true, true, scale, offset, offset, offset);
        skin.shellMesh(verts, faces, false, false, scale, offset + 3.0, offset, offset);
        std::printf(" skin=%llu:%016llx\n", (unsigned long long)skin.solidCount(), digest(skin));
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 1;
    }
    return 0;
}
