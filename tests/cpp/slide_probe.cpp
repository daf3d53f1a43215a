// slide_probe.cpp — move-and-slide's own statement of its rule (include/spec/slide.h) with a host compiler alone: no HIP, no
// library (tests/test_slide_cpu.py builds and runs it, once under the address and undefined-behaviour sanitizers, and holds it
// to the float64 statement of tests/slide_ref.py; tests/test_gpu_slide.py runs a host loop of capsule casts with these steps
// between them and holds the kernel to it bit for bit).
//
//   slide_probe <file>    one answer line per input line; every number a 32-bit word in hex (floats by their bits)
//
// A state is 14 words: p[3] m[3] m0[3] n_prev[3] have_prev status. Input lines, by their first word:
//   0 pos[3] motion[3] has_rot rot[4] R h      ->  valid                        sl_valid
//   1 state skin                               ->  L max_t go                   before a cast: sl_length, sl_max_t; go = L > 0
//   2 state skin id t n[3]                     ->  state go                     after a cast: sl_miss (id == PHYS_RAY_MISS) or sl_hit
//   3 state                                    ->  state                        the casts ran out: sl_ran_out
//   4 pos[3] motion[3]                         ->  state                        sl_begin
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/spec/slide.h"

static const uint32_t kMiss = 0xFFFFFFFEu;  // PHYS_RAY_MISS (physics_hip.h; this probe reads the spec header alone)

static FILE* g_in;
static bool word(uint32_t* out) {
    unsigned v = 0;
    if (std::fscanf(g_in, "%x", &v) != 1) return false;
    *out = (uint32_t)v;
    return true;
}
static uint32_t need() {
    uint32_t v;
    if (!word(&v)) { std::fprintf(stderr, "slide_probe: short or malformed line\n"); std::exit(2); }
    return v;
}
static float real() {
    const uint32_t u = need();
    float x;
    std::memcpy(&x, &u, 4);
    return x;
}
static v3 real3() { v3 r; r.x = real(); r.y = real(); r.z = real(); return r; }
static uint32_t bits(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }
static void put(float x) { std::printf("%08x ", bits(x)); }
static void put3(v3 a) { put(a.x); put(a.y); put(a.z); }

static sl_state read_state() {
    sl_state s;
    s.p = real3(); s.m = real3(); s.m0 = real3(); s.n_prev = real3();
    s.have_prev = (int)need();
    s.status = need();
    return s;
}
static void put_state(const sl_state& s) {
    put3(s.p); put3(s.m); put3(s.m0); put3(s.n_prev);
    std::printf("%08x %08x ", (unsigned)s.have_prev, (unsigned)s.status);
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: slide_probe <file>\n"); return 2; }
    g_in = std::fopen(argv[1], "r");
    if (!g_in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint32_t op;
    while (word(&op)) {
        if (op == 0) {
            const v3 pos = real3(), motion = real3();
            const int has_rot = (int)need();
            quat q; q.i = real(); q.j = real(); q.k = real(); q.w = real();
            const float R = real(), h = real();
            std::printf("%08x", (unsigned)sl_valid(pos, motion, has_rot, q, R, h));
        } else if (op == 1) {
            const sl_state s = read_state();
            const float skin = real();
            const float L = sl_length(s.m);
            put(L); put(sl_max_t(L, skin));
            std::printf("%08x", (unsigned)(L > 0.0f));
        } else if (op == 2) {
            sl_state s = read_state();
            const float skin = real();
            const uint32_t id = need();
            const float t = real();
            const v3 n = real3();
            int go = 0;
            if (id == kMiss) sl_miss(&s);
            else go = sl_hit(&s, sl_length(s.m), skin, t, n);
            put_state(s);
            std::printf("%08x", (unsigned)go);
        } else if (op == 3) {
            sl_state s = read_state();
            sl_ran_out(&s);
            put_state(s);
        } else if (op == 4) {
            sl_state s;
            const v3 pos = real3(), motion = real3();
            sl_begin(&s, pos, motion);
            put_state(s);
        } else {
            std::fprintf(stderr, "slide_probe: unknown line kind %u\n", (unsigned)op);
            return 2;
        }
        std::printf("\n");
    }
    std::fclose(g_in);
    return 0;
}
