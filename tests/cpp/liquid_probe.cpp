// liquid_probe.cpp — the liquids' arithmetic (include/spec/liquid.h) and the checks and staging of a liquid set
// (physics_amd/csrc/setup.hpp) with a host compiler alone: no HIP, no library (tests/test_liquid_cpu.py builds and runs it, once
// under the address and undefined-behaviour sanitizers; tests/test_gpu_liquid.py holds the kernels to its output bit for bit).
//
//   liquid_probe --messages      the validation messages of phys_set_liquids / _params / _poses, each written out here
//   liquid_probe <scene file>    evaluates a scene as the library does - check, stage, build the records, accumulate per body in
//                                ascending liquid index - and prints, per body, `acted`, the bits of force and torque, and the
//                                submersion read-out: the bits of frac and the liquid's index
//
// Scene file, every number a 32-bit word in hex (floats by their bits):
//   n_bodies n_liquids has_rot has_mask
//   per body:   shape pos[3] rot[4] half_extent[3] vel[3] ang[3] category force[3] torque[3]
//   per liquid: pos[3] rot[4] half_extent[3] mask density gravity[3] flow[3] drag[2]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../physics_amd/csrc/setup.hpp"

using namespace phys;

static int g_checks = 0;
#define CHECK_STR(what, got, want)                                                                                      \
    do {                                                                                                                \
        ++g_checks;                                                                                                     \
        const char* p_ = (got);                                                                                         \
        const std::string g_ = p_ ? p_ : "(none)", w_ = (want);                                                         \
        if (g_ != w_) {                                                                                                 \
            std::printf("MISMATCH %s:%d  %s:\n  got      \"%s\"\n  expected \"%s\"\n", __FILE__, __LINE__, what, g_.c_str(), w_.c_str()); \
            std::exit(1);                                                                                               \
        }                                                                                                               \
    } while (0)
#define CHECK(what, cond)                                                              \
    do {                                                                               \
        ++g_checks;                                                                    \
        if (!(cond)) { std::printf("MISMATCH %s:%d  %s\n", __FILE__, __LINE__, what); std::exit(1); } \
    } while (0)

static int messages() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    // three liquids, all fine
    float pos[9] = {0, 0, 0, 1, 2, 3, -1, -2, -3};
    float rot[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
    float he[9] = {1, 1, 1, 2, 0, 3, 0.5f, 1, 0};
    float density[3] = {1000, 0, 2.5f};
    float gravity[9] = {0, -9.81f, 0, 0, 0, 0, 1, 2, 3};
    float flow[9] = {0, 0, 0, 1, 0, 0, 0, 0, -2};
    float drag[6] = {0, 0, 0.5f, 0.25f, 3, 0};
    std::string msg;
#define LQ_ERR() liquid_set_error(3, pos, rot, he, density, gravity, flow, drag, msg)
    CHECK_STR("all fine", LQ_ERR(), "(none)");
    CHECK_STR("rot is optional", liquid_set_error(3, pos, nullptr, he, density, gravity, flow, drag, msg), "(none)");
    const char* nf = "liquid 2: non-finite number";
    pos[7] = nan;      CHECK_STR("pos", LQ_ERR(), nf);  pos[7] = -2;
    rot[9] = inf;      CHECK_STR("rot", LQ_ERR(), nf);
    CHECK_STR("rot null: not looked at", liquid_set_error(3, pos, nullptr, he, density, gravity, flow, drag, msg), "(none)");
    rot[9] = 0;
    he[6] = -inf;      CHECK_STR("half extent, non-finite before negative", LQ_ERR(), nf);  he[6] = 0.5f;
    density[2] = nan;  CHECK_STR("density", LQ_ERR(), nf);  density[2] = 2.5f;
    gravity[8] = inf;  CHECK_STR("gravity", LQ_ERR(), nf);  gravity[8] = 3;
    flow[6] = nan;     CHECK_STR("flow", LQ_ERR(), nf);  flow[6] = 0;
    drag[5] = nan;     CHECK_STR("drag", LQ_ERR(), nf);  drag[5] = 0;
    he[2] = -1; density[0] = -inf;
    CHECK_STR("non-finite before negative half extent", LQ_ERR(), "liquid 0: non-finite number");
    density[0] = -1;
    CHECK_STR("negative half extent before negative density", LQ_ERR(), "liquid 0: negative half extent");
    drag[2] = -0.5f;  // several offend: the first index
    CHECK_STR("first index", LQ_ERR(), "liquid 0: negative half extent");
    he[2] = 1; drag[0] = -1;
    CHECK_STR("negative density before negative drag", LQ_ERR(), "liquid 0: negative density");
    density[0] = 1000; drag[0] = 0;
    CHECK_STR("negative linear drag", LQ_ERR(), "liquid 1: negative drag coefficient");
    drag[2] = 0.5f; drag[3] = -0.25f;
    CHECK_STR("negative angular drag", LQ_ERR(), "liquid 1: negative drag coefficient");
    drag[3] = 0.25f;
    CHECK_STR("all fine again", LQ_ERR(), "(none)");

    // the staged set and its two updates
    const uint16_t mask[3] = {1, 2, 0xFFFF};
    LiquidStaging st = stage_liquids(3, pos, nullptr, he, mask, density, gravity, flow, drag);
    CHECK("stage_liquids", st.masked && st.drag && st.staged.size() == 3 && lq_f2u(st.staged[1].s[0].x) == 2u && st.staged[0].s[0].w == 1000.0f &&
                               st.staged[1].s[2].w == 1.0f && st.staged[1].s[2].x == 0.0f && st.staged[2].s[1].y == -2.0f &&
                               st.staged[1].s[3].z == 3.0f && st.staged[1].s[4].w == 0.5f && st.staged[1].s[5].w == 0.25f &&
                               st.staged[0].s[5].y == -9.81f && st.staged[2].s[4].z == -2.0f);
    const LiquidStaging plain = stage_liquids(1, pos, rot, he, nullptr, density, gravity, flow, drag);
    CHECK("stage_liquids defaults", !plain.masked && !plain.drag && lq_f2u(plain.staged[0].s[0].x) == 0xFFFFu);
    const lq_record rec = lq_record_make(&st.staged[0]);
    CHECK("record", sizeof(lq_record) == 128 && rec.vol.r[5].w == 1000.0f && vol_mask(rec.vol.r[1]) == 1u && rec.grav.y == -9.81f &&
                        rec.vol.r[0].x == -1.0f && rec.vol.r[1].y == 1.0f && vol_word(rec.vol.r[0]) == PHYS_SHAPE_BOX);
    float density2[3] = {1, 2, 3}, gravity2[9] = {0, -1, 0, 0, -2, 0, 0, -3, 0}, flow2[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, drag2[6] = {0, 0, 0, 0, 0, 0};
    CHECK_STR("params: fine", restage_liquid_params(st.staged, density2, gravity2, flow2, drag2, msg), "(none)");
    CHECK("restage params", st.staged[1].s[0].w == 2.0f && st.staged[2].s[5].y == -3.0f && st.staged[1].s[4].w == 0.0f && !liquids_have_drag(st.staged) &&
                                lq_f2u(st.staged[1].s[0].x) == 2u);
    density2[1] = -2;
    CHECK_STR("params: density", restage_liquid_params(st.staged, density2, gravity2, flow2, drag2, msg), "liquid 1: negative density");
    density2[1] = 2; drag2[5] = -1;
    CHECK_STR("params: drag", restage_liquid_params(st.staged, density2, gravity2, flow2, drag2, msg), "liquid 2: negative drag coefficient");
    drag2[5] = 0; gravity2[1] = inf; density2[0] = 7;
    CHECK_STR("params: non-finite", restage_liquid_params(st.staged, density2, gravity2, flow2, drag2, msg), "liquid 0: non-finite number");
    CHECK("a refused params call changed nothing", st.staged[0].s[0].w == 1.0f);
    float pos2[9] = {5, 5, 5, 6, 6, 6, 7, 7, 7};
    CHECK("restage poses", restage_liquid_poses(st.staged, pos2, nullptr) && st.staged[2].s[1].x == 7.0f && st.staged[2].s[2].w == 1.0f);
    pos2[4] = nan;
    CHECK("non-finite poses", !restage_liquid_poses(st.staged, pos2, nullptr) && st.staged[1].s[1].x == 6.0f);
    std::printf("%d checks passed\n", g_checks);
    return 0;
}

static uint32_t word(FILE* f) {
    unsigned v = 0;
    if (std::fscanf(f, "%x", &v) != 1) { std::fprintf(stderr, "scene file: short or malformed\n"); std::exit(2); }
    return (uint32_t)v;
}
static float real(FILE* f) { return lq_u2f(word(f)); }
static v3 real3(FILE* f) { v3 r; r.x = real(f); r.y = real(f); r.z = real(f); return r; }

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: liquid_probe --messages | <scene file>\n"); return 2; }
    if (std::strcmp(argv[1], "--messages") == 0) return messages();
    FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    const uint32_t nb = word(f), nl = word(f), has_rot = word(f), has_mask = word(f);
    if (nb > (1u << 20) || nl > PHYS_MAX_LIQUIDS) { std::fprintf(stderr, "scene file: counts out of range\n"); return 2; }
    std::vector<lq_body> body(nb);
    std::vector<v3> force(nb), torque(nb);
    for (uint32_t i = 0; i < nb; ++i) {
        const uint32_t shape = word(f);
        const v3 x = real3(f);
        quat q;
        q.i = real(f); q.j = real(f); q.k = real(f); q.w = real(f);
        const v3 h = real3(f), v = real3(f), w = real3(f);
        const uint32_t category = word(f);
        body[i] = lq_body_make(shape, x, q, h, v, w, category);
        force[i] = real3(f);
        torque[i] = real3(f);
    }
    std::vector<uint16_t> mask(nl);
    std::vector<float> pos(3 * nl), rot(4 * nl), he(3 * nl), density(nl), gravity(3 * nl), flow(3 * nl), drag(2 * nl);
    for (uint32_t k = 0; k < nl; ++k) {
        for (int a = 0; a < 3; ++a) pos[3 * k + a] = real(f);
        for (int a = 0; a < 4; ++a) rot[4 * k + a] = real(f);
        for (int a = 0; a < 3; ++a) he[3 * k + a] = real(f);
        mask[k] = (uint16_t)word(f);
        density[k] = real(f);
        for (int a = 0; a < 3; ++a) gravity[3 * k + a] = real(f);
        for (int a = 0; a < 3; ++a) flow[3 * k + a] = real(f);
        for (int a = 0; a < 2; ++a) drag[2 * k + a] = real(f);
    }
    std::fclose(f);
    std::string msg;
    const float* rotp = has_rot ? rot.data() : nullptr;
    if (const char* bad = liquid_set_error(nl, pos.data(), rotp, he.data(), density.data(), gravity.data(), flow.data(), drag.data(), msg)) {
        std::printf("refused: %s\n", bad);
        return 3;
    }
    const LiquidStaging st = stage_liquids(nl, pos.data(), rotp, he.data(), has_mask ? mask.data() : nullptr, density.data(), gravity.data(),
                                           flow.data(), drag.data());
    const std::vector<lq_record> rec = liquid_records(st.staged);
    const int masked = st.masked ? 1 : 0, dragged = st.drag ? 1 : 0;
    for (uint32_t i = 0; i < nb; ++i) {
        lq_sum whole;
        whole.F = whole.T = v3_make(0.0f, 0.0f, 0.0f);
        whole.acted = 0;
        lq_accumulate(rec.data(), nl, &body[i], masked, dragged, &force[i], &torque[i], &whole);
        // the kernel walks the records in tiles of 32 with the same sums: the same bits
        lq_sum tiled = whole;
        tiled.acted = 0;
        float frac = 0.0f;
        uint32_t liquid = LQ_NONE;
        for (uint32_t t0 = 0; t0 < nl; t0 += 32) {
            const uint32_t tn = nl - t0 < 32 ? nl - t0 : 32;
            lq_accumulate(rec.data() + t0, tn, &body[i], masked, dragged, &force[i], &torque[i], &tiled);
            lq_submersion(rec.data() + t0, tn, t0, &body[i], masked, &frac, &liquid);
        }
        const v3 F = whole.acted ? whole.F : force[i], T = whole.acted ? whole.T : torque[i];
        if (tiled.acted != whole.acted || (whole.acted && std::memcmp(&tiled, &whole, sizeof(v3) * 2) != 0)) {
            std::printf("MISMATCH body %u: a tiled walk differs from one walk\n", i);
            return 1;
        }
        if ((liquid != LQ_NONE) != (whole.acted != 0)) {
            std::printf("MISMATCH body %u: the read-out and the accumulation disagree on whether a liquid acts\n", i);
            return 1;
        }
        std::printf("%d %08x %08x %08x %08x %08x %08x %08x %08x\n", whole.acted, lq_f2u(F.x), lq_f2u(F.y), lq_f2u(F.z), lq_f2u(T.x), lq_f2u(T.y),
                    lq_f2u(T.z), lq_f2u(frac), liquid);
    }
    return 0;
}
