// static_set_cli.cpp — build_static_set of physics_amd/csrc/setup.hpp for a static set in a file, so that a Python test can
// take the float32 fattened boxes the world uploads and ask which grid a scene gets, instead of restating the build
// (tests/static_ref.py, tests/test_static_ref_cpu.py, tests/test_gpu_static_independent.py). It serves scene facts and boxes
// and is never a reference for the visit. Built by a host compiler alone.
//   static_set_cli <file> <contact margin> <box file>
//   file: uint64 n, n x 3 float32 positions, n x 4 float32 rotations, n uint32 shapes, n x 3 float32 half extents
//   box file (written): n x 6 float32 {lo xyz, hi xyz}
//   prints: n_large  dim_x dim_y dim_z  cell_edge  longest_cell_list  span_x span_y span_z  first_x first_y first_z  multi_cell  org_x org_y org_z  most_cells
//           (span: the largest cell span of a small static per axis; first: the largest packed first cell per axis;
//            multi_cell: small statics in more than one cell; most_cells: the most cells ONE small static lies in)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../physics_amd/csrc/setup.hpp"

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    unsigned long long n = 0;
    if (std::fread(&n, 8, 1, f) != 1 || n == 0) { std::fclose(f); return 2; }
    std::vector<float> pos(3 * n), rot(4 * n), he(3 * n);
    std::vector<uint32_t> shape(n);
    if (std::fread(pos.data(), 4, 3 * n, f) != 3 * n || std::fread(rot.data(), 4, 4 * n, f) != 4 * n ||
        std::fread(shape.data(), 4, n, f) != n || std::fread(he.data(), 4, 3 * n, f) != 3 * n)
        return 2;
    std::fclose(f);
    const phys::StaticSet s = phys::build_static_set(n, pos.data(), rot.data(), shape.data(), he.data(), (float)std::atof(argv[2]), 0.5f);

    std::vector<float> box(6 * n);
    for (unsigned long long k = 0; k < n; ++k)
        for (int a = 0; a < 3; ++a) { box[6 * k + a] = s.box[8 * k + a]; box[6 * k + 3 + a] = s.box[8 * k + 4 + a]; }
    std::FILE* o = std::fopen(argv[3], "wb");
    if (!o || std::fwrite(box.data(), 4, 6 * n, o) != 6 * n) return 2;
    std::fclose(o);

    std::vector<uint8_t> is_large(n, 0);
    for (uint32_t j = 0; j < s.n_large; ++j) is_large[s.large[j]] = 1;
    uint32_t longest = 0, span[3] = {0, 0, 0}, first[3] = {0, 0, 0};
    unsigned long long multi = 0, most = 0;
    if (s.dim[0]) {
        const unsigned long long cells = (unsigned long long)s.dim[0] * s.dim[1] * s.dim[2];
        for (unsigned long long c = 0; c < cells; ++c) longest = std::max(longest, s.cell_start[c + 1] - s.cell_start[c]);
        for (unsigned long long k = 0; k < n; ++k) {
            if (is_large[k]) continue;
            uint32_t p;
            std::memcpy(&p, &s.box[8 * k + 3], 4);
            const uint32_t lo[3] = {p & 1023u, (p >> 10) & 1023u, p >> 20};
            bool many = false;
            unsigned long long in = 1;
            for (int a = 0; a < 3; ++a) {
                const uint32_t hi = phys::st_cell(s.box[8 * k + 4 + a], s.org[a], s.inv_cell, s.dim[a]);
                span[a] = std::max(span[a], hi - lo[a] + 1u);
                first[a] = std::max(first[a], lo[a]);
                many = many || hi > lo[a];
                in *= hi - lo[a] + 1u;
            }
            multi += many;
            most = std::max(most, in);
        }
    }
    std::printf("%u %u %u %u %.9g %u %u %u %u %u %u %u %llu %.9g %.9g %.9g %llu\n", s.n_large, s.dim[0], s.dim[1], s.dim[2],
                s.dim[0] ? 1.0 / (double)s.inv_cell : 0.0, longest, span[0], span[1], span[2], first[0], first[1], first[2], multi,
                (double)s.org[0], (double)s.org[1], (double)s.org[2], most);
    return 0;
}
