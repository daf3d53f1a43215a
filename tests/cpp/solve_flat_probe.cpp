// solve_flat_probe.cpp — the cluster solver's flat row driver (solve_manifold_flat, include/spec/contact_solve.h) beside the
// driver it restates (solve_manifold_geo), with a host compiler alone: no HIP, no library. tests/test_solve_flat_cpu.py builds
// and runs it, once under the address and undefined-behaviour sanitizers, and compares the two halves of every answer bit for bit.
//
//   solve_flat_probe <file>    one answer line per input line; every number a 32-bit word in hex (floats by their bits)
//
// Input line (74 words): count has_b warm sweeps | n[3] pt[4][3] bias[4] | xA[3] invMA IA[9] | xB[3] invMB IB[9] |
//                        vA[3] wA[3] vB[3] wB[3] | friction | pn[4] pt0[4] pt1[4]
//   warm == 0: a cold solve - the impulses start from zero (the line's are ignored), the first sweep makes the row masses and
//              relaxes; warm != 0: the first sweep makes the masses and applies the line's impulses; `sweeps` regular sweeps follow.
// solve_manifold_geo gets the line as it stands, body B's numbers included when has_b == 0 (it must ignore them);
// solve_manifold_flat gets what its contract asks of the caller: zeros for xB, invMB, IB, vB, wB when has_b == 0.
// Answer: geo's record, then flat's, each 12 + (1 + sweeps) * 24 words: the row masses after the first sweep [point][t1, t2, n],
//         then after every sweep vA[3] wA[3] vB[3] wB[3] pn[4] pt0[4] pt1[4].
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/spec/contact_solve.h"

static FILE* g_in;
static bool word(uint32_t* out) {
    unsigned v = 0;
    if (std::fscanf(g_in, "%x", &v) != 1) return false;
    *out = (uint32_t)v;
    return true;
}
static uint32_t need() {
    uint32_t v;
    if (!word(&v)) { std::fprintf(stderr, "solve_flat_probe: short or malformed line\n"); std::exit(2); }
    return v;
}
static float real() {
    const uint32_t u = need();
    float x;
    std::memcpy(&x, &u, 4);
    return x;
}
static v3 real3() { v3 r; r.x = real(); r.y = real(); r.z = real(); return r; }
static void put(float x) { uint32_t u; std::memcpy(&u, &x, 4); std::printf("%08x ", u); }
static void put3(v3 a) { put(a.x); put(a.y); put(a.z); }

struct Body { v3 x; float inv_mass; m33 I; };
static Body read_body() {
    Body b;
    b.x = real3(); b.inv_mass = real();
    for (int k = 0; k < 9; ++k) b.I.m[k] = real();
    return b;
}
static void put_state(const geo_manifold_t& g, const v3 v[4]) {
    for (int k = 0; k < 4; ++k) put3(v[k]);
    for (int k = 0; k < 4; ++k) put(g.pn[k]);
    for (int k = 0; k < 4; ++k) put(g.pt0[k]);
    for (int k = 0; k < 4; ++k) put(g.pt1[k]);
}
static void put_masses(const geo_manifold_t& g) {
    for (int k = 0; k < 4; ++k) for (int t = 0; t < 3; ++t) put(g.mass[k][t]);
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: solve_flat_probe <file>\n"); return 2; }
    g_in = std::fopen(argv[1], "r");
    if (!g_in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint32_t first;
    while (word(&first)) {
        geo_manifold_t g;
        g.count = (int)first;
        g.has_b = (int)need();
        const int warm = (int)need();
        const int sweeps = (int)need();
        if (g.count < 1 || g.count > 4 || sweeps < 0 || sweeps > 64) { std::fprintf(stderr, "solve_flat_probe: bad count or sweeps\n"); return 2; }
        g.n = real3();
        tangent_basis(g.n, &g.t1, &g.t2);
        for (int k = 0; k < 4; ++k) g.pt[k] = real3();
        for (int k = 0; k < 4; ++k) g.bias[k] = real();
        const Body A = read_body(), B = read_body();
        v3 v[4];
        for (int k = 0; k < 4; ++k) v[k] = real3();
        const float friction = real();
        for (int k = 0; k < 4; ++k) g.pn[k] = real();
        for (int k = 0; k < 4; ++k) g.pt0[k] = real();
        for (int k = 0; k < 4; ++k) g.pt1[k] = real();
        if (!warm) for (int k = 0; k < 4; ++k) { g.pn[k] = 0.0f; g.pt0[k] = 0.0f; g.pt1[k] = 0.0f; }
        for (int k = 0; k < 4; ++k) for (int t = 0; t < 3; ++t) g.mass[k][t] = 0.0f;

        {   // the spec's driver, body B as the line has it
            geo_manifold_t c = g;
            v3 u[4] = {v[0], v[1], v[2], v[3]};
            solve_manifold_geo(&c, 1, warm ? 1 : 0, friction, A.x, A.inv_mass, &A.I, B.x, B.inv_mass, &B.I, &u[0], &u[1], &u[2], &u[3]);
            put_masses(c);
            put_state(c, u);
            for (int s = 0; s < sweeps; ++s) {
                solve_manifold_geo(&c, 0, 0, friction, A.x, A.inv_mass, &A.I, B.x, B.inv_mass, &B.I, &u[0], &u[1], &u[2], &u[3]);
                put_state(c, u);
            }
        }
        {   // the flat driver, body B zero-filled by the caller where there is none
            geo_manifold_t c = g;
            v3 u[4] = {v[0], v[1], v[2], v[3]};
            Body Bz = B;
            if (!g.has_b) {
                std::memset(&Bz, 0, sizeof Bz);
                u[2] = v3_make(0.0f, 0.0f, 0.0f); u[3] = u[2];
            }
            if (warm) solve_manifold_flat<true, true>(&c, friction, A.x, A.inv_mass, &A.I, Bz.x, Bz.inv_mass, &Bz.I, &u[0], &u[1], &u[2], &u[3]);
            else solve_manifold_flat<true, false>(&c, friction, A.x, A.inv_mass, &A.I, Bz.x, Bz.inv_mass, &Bz.I, &u[0], &u[1], &u[2], &u[3]);
            put_masses(c);
            put_state(c, u);
            for (int s = 0; s < sweeps; ++s) {
                solve_manifold_flat<false, false>(&c, friction, A.x, A.inv_mass, &A.I, Bz.x, Bz.inv_mass, &Bz.I, &u[0], &u[1], &u[2], &u[3]);
                put_state(c, u);
            }
        }
        std::printf("\n");
    }
    std::fclose(g_in);
    return 0;
}
