// Exercises the mesh voxelisation of the C++ host adapter (cpuvoxelraycaster_amd/host/hip_raycaster.hpp): xorMesh of
// ready-made fixed-point triangles, voxelizeMesh of an indexed float mesh, and stampMesh -- paste with OR, then carve a
// shifted copy with ANDNOT -- into a volume that already holds a slab.  Writes the three dense occupancies; the pytest
// wrapper compares them bit for bit with the numpy model.
//   usage: voxel_mesh_main <depth> <verts.bin: n x 3 float64> <faces.bin: m x 3 uint32> <tris.bin: k x 9 int32>
//                          <scale> <ox> <oy> <oz> <output prefix>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "../../cpuvoxelraycaster_amd/host/hip_raycaster.hpp"

template <class T>
static std::vector<T> read_all(const char* path)
{
    std::ifstream f(path, std::ios::binary);
    const std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const T* p = (const T*)raw.data();
    return std::vector<T>(p, p + raw.size() / sizeof(T));
}

static void dump(vrc_host::HipVoxelVolume& vol, const std::string& path)
{
    const uint64_t S = 1ull << vol.depth();
    std::vector<uint8_t> dense(S * S * S);
    vrc_host::check(vrc_volume_download(vol.handle(), dense.data()), "vrc_volume_download");
    std::ofstream(path, std::ios::binary).write((const char*)dense.data(), (std::streamsize)dense.size());
}

int main(int argc, char** argv)
{
    if (argc != 10) return 2;
    const uint32_t depth = (uint32_t)atoi(argv[1]);
    const std::vector<double> verts = read_all<double>(argv[2]);
    const std::vector<uint32_t> faces = read_all<uint32_t>(argv[3]);
    const std::vector<int32_t> tris = read_all<int32_t>(argv[4]);
    const double scale = atof(argv[5]), ox = atof(argv[6]), oy = atof(argv[7]), oz = atof(argv[8]);
    const std::string prefix = argv[9];
    try {
        const uint32_t S = 1u << depth;
        vrc_host::HipVoxelVolume a(depth);
        a.setCell(vrc_host::Cell::Solid, vrc_host::Cell::Grass, 1, 2, 3);       // still queued when xorMesh is called
        a.xorMesh(tris);
        dump(a, prefix + "_xor.bin");

        vrc_host::HipVoxelVolume b(depth);
        b.voxelizeMesh(verts, faces, scale, ox, oy, oz);
        dump(b, prefix + "_vox.bin");

        vrc_host::HipVoxelVolume c(depth);
        c.fillBox(0, 0, 0, S, S / 4, S, true);
        c.stampMesh(verts, faces, VRC_COPY_OR, scale, ox, oy, oz);
        c.stampMesh(verts, faces, VRC_COPY_ANDNOT, scale, ox + 7.0, oy - 3.0, oz + 4.5);
        dump(c, prefix + "_stamp.bin");
        std::printf("triangles=%zu faces=%zu solid=%llu %llu %llu\n", tris.size() / 9, faces.size() / 3, (unsigned long long)a.solidCount(),
                    (unsigned long long)b.solidCount(), (unsigned long long)c.solidCount());
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 1;
    }
    return 0;
}
