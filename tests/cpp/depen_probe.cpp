// depen_probe.cpp — depenetration's own statement of its rule (include/spec/depenetrate.h) with a host compiler alone: no HIP, no
// library (tests/test_depen_cpu.py builds and runs it, once under the address and undefined-behaviour sanitizers, and holds it
// to the float64 statement of tests/depen_ref.py; tests/test_gpu_depen.py runs a host loop of phys_penetration calls with
// dp_step between them and holds the kernel to it bit for bit).
//
//   depen_probe <file>    one answer line per input line; every number a 32-bit word in hex (floats by their bits)
//
// A query is 10 words: pos[3] has_rot rot[4] R h. A target list is: ground_flag ground_y count, then per target 12 words:
// id type centre[3] rot[4] half_extent[3]. An answer of the probe is 5 words: id depth n[3]. Input lines, by their first word:
//   0 query                                    ->  valid                        dp_valid
//   1 p[3] status k max_iters skin answer      ->  p[3] status go               dp_step
//   2 query gap targets                        ->  answer                       dp_deepest: the probe's own loop over the list
//   3 query skin max_iters targets             ->  p[3] status, max_iters slots (id n[3] depth)   the whole loop
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/spec/depenetrate.h"

static FILE* g_in;
static bool word(uint32_t* out) {
    unsigned v = 0;
    if (std::fscanf(g_in, "%x", &v) != 1) return false;
    *out = (uint32_t)v;
    return true;
}
static uint32_t need() {
    uint32_t v;
    if (!word(&v)) { std::fprintf(stderr, "depen_probe: short or malformed line\n"); std::exit(2); }
    return v;
}
static float real() {
    const uint32_t u = need();
    float x;
    std::memcpy(&x, &u, 4);
    return x;
}
static v3 real3() { v3 r; r.x = real(); r.y = real(); r.z = real(); return r; }
static quat real4() { quat q; q.i = real(); q.j = real(); q.k = real(); q.w = real(); return q; }
static uint32_t bits(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }
static void put(float x) { std::printf("%08x ", bits(x)); }
static void put3(v3 a) { put(a.x); put(a.y); put(a.z); }

struct Query { v3 pos; int has_rot; quat rot; float R, h; };
struct Target { uint32_t id; geom_t g; };
struct Targets { int ground; float ground_y; std::vector<Target> list; };

static Query read_query() {
    Query q;
    q.pos = real3(); q.has_rot = (int)need(); q.rot = real4(); q.R = real(); q.h = real();
    return q;
}
static Targets read_targets() {
    Targets t;
    t.ground = (int)need(); t.ground_y = real();
    const uint32_t count = need();
    for (uint32_t k = 0; k < count; ++k) {
        Target x;
        x.id = need();
        const uint32_t type = need();
        const v3 c = real3();
        const quat q = real4();
        const v3 h = real3();
        x.g = geom_make(c, q, h, type);
        t.list.push_back(x);
    }
    return t;
}
static v3 axis_of(const Query& q) { return q.has_rot ? dp_axis(q.rot) : v3_make(0.0f, 1.0f, 0.0f); }

// the probe at p: every target of the list in the order given, then the ground
static dp_best dp_deepest(const Query& q, v3 p, float gap, const Targets& t) {
    const geom_t Q = dp_capsule(p, axis_of(q), q.R, q.h);
    dp_best best = dp_none();
    for (const Target& x : t.list) dp_target(&Q, &x.g, x.id, gap, &best);
    if (t.ground) dp_ground(&Q, t.ground_y, gap, &best);
    return best;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: depen_probe <file>\n"); return 2; }
    g_in = std::fopen(argv[1], "r");
    if (!g_in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint32_t op;
    while (word(&op)) {
        if (op == 0) {
            const Query q = read_query();
            std::printf("%08x", (unsigned)dp_valid(q.pos, q.has_rot, q.rot, q.R, q.h));
        } else if (op == 1) {
            dp_state s;
            s.p = real3(); s.status = need();
            const uint32_t k = need(), max_iters = need();
            const float skin = real();
            dp_best b;
            b.id = need(); b.depth = real(); b.n = real3();
            const int go = dp_step(&s, k, max_iters, skin, &b);
            put3(s.p);
            std::printf("%08x %08x", (unsigned)s.status, (unsigned)go);
        } else if (op == 2) {
            const Query q = read_query();
            const float gap = real();
            const Targets t = read_targets();
            const dp_best b = dp_valid(q.pos, q.has_rot, q.rot, q.R, q.h) ? dp_deepest(q, q.pos, gap, t) : dp_none();
            std::printf("%08x ", (unsigned)b.id); put(b.depth); put3(b.n);
        } else if (op == 3) {
            const Query q = read_query();
            const float skin = real();
            const uint32_t max_iters = need();
            const Targets t = read_targets();
            if (max_iters < 1u || max_iters > DP_MAX_ITERS) { std::fprintf(stderr, "depen_probe: max_iters out of range\n"); return 2; }
            dp_state s;
            dp_begin(&s, q.pos);
            dp_best slots[DP_MAX_ITERS];
            uint32_t k = 0;
            if (!dp_valid(q.pos, q.has_rot, q.rot, q.R, q.h)) {
                s.status = DP_INVALID;
            } else {
                for (;; ++k) {
                    const dp_best b = dp_deepest(q, s.p, skin, t);
                    if (!dp_step(&s, k, max_iters, skin, &b)) break;
                    slots[k] = b;
                }
            }
            put3(s.p);
            std::printf("%08x ", (unsigned)s.status);
            for (uint32_t e = 0; e < max_iters; ++e) {
                dp_best b = dp_none();
                b.depth = 0.0f;
                if (e < k) b = slots[e];
                std::printf("%08x ", (unsigned)b.id); put3(b.n); put(b.depth);
            }
        } else {
            std::fprintf(stderr, "depen_probe: unknown line kind %u\n", (unsigned)op);
            return 2;
        }
        std::printf("\n");
    }
    std::fclose(g_in);
    return 0;
}
