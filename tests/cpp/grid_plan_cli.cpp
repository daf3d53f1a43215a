// grid_plan_cli.cpp — grid_plan of physics_amd/csrc/setup.hpp for a body set in a file, so that a Python test can ask which
// bucket table a scene gets instead of restating the split (tests/test_pair_ref_cpu.py). Built by a host compiler alone.
//   grid_plan_cli <file> <contact margin>     file: uint64 n, n x 3 float32 positions, n x 3 float32 half extents
//   prints: table_size cells_x cells_y cells_z
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../physics_amd/csrc/setup.hpp"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    unsigned long long n = 0;
    if (std::fread(&n, 8, 1, f) != 1) return 2;
    std::vector<float> pos(3 * n), he(3 * n);
    if (std::fread(pos.data(), 4, 3 * n, f) != 3 * n || std::fread(he.data(), 4, 3 * n, f) != 3 * n) return 2;
    std::fclose(f);
    const phys::GridPlan p = phys::grid_plan(n, n, pos.data(), he.data(), (float)std::atof(argv[2]));
    std::printf("%u %u %u %u\n", p.table_size, p.shape.mx + 1u, p.shape.my + 1u, p.shape.mz + 1u);
    return 0;
}
