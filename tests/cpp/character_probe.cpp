// character_probe.cpp — character walking's own statement of its rule (include/spec/character.h) with a host compiler alone: no
// HIP, no library (tests/test_character_cpu.py builds and runs it, once under the address and undefined-behaviour sanitizers,
// and holds it to the float64 statement of tests/character_ref.py; tests/test_gpu_character.py drives ch_next / ch_answer with
// World.capsulecast as the cast and holds the kernel to that loop bit for bit).
//
//   character_probe <file>    one answer line per input line; every number a 32-bit word in hex (floats by their bits)
//
// A state is 36 words: sl (p[3] m[3] m0[3] n_prev[3] have_prev status) pos[3] p_move[3] m_move[3] lift L skin step_height
// snap_distance min_floor_ny max_slides k phase walking ended floor_found status. Input lines, by their first word:
//   0 pos[3] motion[3] has_rot rot[4] R h                                                ->  valid          ch_valid
//   1 pos[3] motion[3] grounded skin max_slides step_height snap_distance min_floor_ny   ->  state          ch_begin
//   2 state                       ->  state go origin[3] dir[3] len max_t slot                              ch_next
//   3 state id t n[3] point[3]    ->  state floor_found                                                     ch_answer
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/spec/character.h"

static FILE* g_in;
static bool word(uint32_t* out) {
    unsigned v = 0;
    if (std::fscanf(g_in, "%x", &v) != 1) return false;
    *out = (uint32_t)v;
    return true;
}
static uint32_t need() {
    uint32_t v;
    if (!word(&v)) { std::fprintf(stderr, "character_probe: short or malformed line\n"); std::exit(2); }
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
static void putw(uint32_t u) { std::printf("%08x ", (unsigned)u); }

static ch_state read_state() {
    ch_state s;
    s.sl.p = real3(); s.sl.m = real3(); s.sl.m0 = real3(); s.sl.n_prev = real3();
    s.sl.have_prev = (int)need();
    s.sl.status = need();
    s.pos = real3(); s.p_move = real3(); s.m_move = real3();
    s.lift = real(); s.L = real(); s.skin = real(); s.step_height = real(); s.snap_distance = real(); s.min_floor_ny = real();
    s.max_slides = need(); s.k = need(); s.phase = need(); s.walking = need(); s.ended = need(); s.floor_found = need();
    s.status = need();
    return s;
}
static void put_state(const ch_state& s) {
    put3(s.sl.p); put3(s.sl.m); put3(s.sl.m0); put3(s.sl.n_prev);
    putw((uint32_t)s.sl.have_prev); putw(s.sl.status);
    put3(s.pos); put3(s.p_move); put3(s.m_move);
    put(s.lift); put(s.L); put(s.skin); put(s.step_height); put(s.snap_distance); put(s.min_floor_ny);
    putw(s.max_slides); putw(s.k); putw(s.phase); putw(s.walking); putw(s.ended); putw(s.floor_found);
    putw(s.status);
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: character_probe <file>\n"); return 2; }
    g_in = std::fopen(argv[1], "r");
    if (!g_in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint32_t op;
    while (word(&op)) {
        if (op == 0) {
            const v3 pos = real3(), motion = real3();
            const int has_rot = (int)need();
            quat q; q.i = real(); q.j = real(); q.k = real(); q.w = real();
            const float R = real(), h = real();
            putw((uint32_t)ch_valid(pos, motion, has_rot, q, R, h));
        } else if (op == 1) {
            ch_state s;
            const v3 pos = real3(), motion = real3();
            const uint32_t grounded = need();
            const float skin = real();
            const uint32_t max_slides = need();
            const float step_height = real(), snap_distance = real(), min_floor_ny = real();
            ch_begin(&s, pos, motion, grounded, skin, max_slides, step_height, snap_distance, min_floor_ny);
            put_state(s);
        } else if (op == 2) {
            ch_state s = read_state();
            ch_request r;
            r.origin = v3_make(0.0f, 0.0f, 0.0f); r.dir = r.origin; r.len = 0.0f; r.max_t = 0.0f; r.slot = CH_SLOT_NONE;
            const int go = ch_next(&s, &r);
            put_state(s);
            putw((uint32_t)go); put3(r.origin); put3(r.dir); put(r.len); put(r.max_t); putw((uint32_t)r.slot);
        } else if (op == 3) {
            ch_state s = read_state();
            const uint32_t id = need();
            const float t = real();
            const v3 n = real3(), point = real3();
            ch_answer(&s, id, t, n, point);
            put_state(s);
            putw((uint32_t)ch_floor_found(&s));
        } else {
            std::fprintf(stderr, "character_probe: unknown line kind %u\n", (unsigned)op);
            return 2;
        }
        std::printf("\n");
    }
    std::fclose(g_in);
    return 0;
}
