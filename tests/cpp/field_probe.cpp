// field_probe.cpp — the force fields' arithmetic (include/spec/force_field.h) and the checks and staging of a field set
// (physics_amd/csrc/setup.hpp) with a host compiler alone: no HIP, no library (tests/test_field_cpu.py builds and runs it, once
// under the address and undefined-behaviour sanitizers; tests/test_gpu_fields.py holds the kernel to its output bit for bit).
//
//   field_probe --messages      the validation messages of phys_set_force_fields / _params / _poses, each written out here
//   field_probe <scene file>    evaluates a scene as the library does - check, stage, build the records, accumulate per body in
//                               ascending field index - and prints, per body, `acted` and the bits of force and torque
//
// Scene file, every number a 32-bit word in hex (floats by their bits):
//   n_bodies n_fields has_rot has_mask has_exponent
//   per body:  pos[3] vel[3] ang[3] mass category force[3] torque[3]
//   per field: kind shape pos[3] rot[4] half_extent[3] mask vec[3] coef[2] exponent
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

static int messages() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    // three fields, all fine: an ACCEL box, a DRAG sphere, a RADIAL capsule
    uint32_t kind[3] = {PHYS_FIELD_ACCEL, PHYS_FIELD_DRAG, PHYS_FIELD_RADIAL};
    uint32_t shape[3] = {PHYS_SHAPE_BOX, PHYS_SHAPE_SPHERE, PHYS_SHAPE_CAPSULE};
    float pos[9] = {0, 0, 0, 1, 2, 3, -1, -2, -3};
    float rot[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
    float he[9] = {1, 1, 1, 2, 0, 0, 0.5f, 1, 0};
    float vec[9] = {0, 9.81f, 0, 1, 0, 0, 0, 0, 0};
    float coef[6] = {0, 0, 0.5f, 0.25f, -3, 1.5f};
    uint32_t ex[3] = {0, 0, 2};
    std::string msg;
    CHECK_STR("all fine", field_set_error(3, kind, shape, pos, rot, he, vec, coef, ex, msg), "(none)");
    CHECK_STR("rot and exponent are optional", field_set_error(3, kind, shape, pos, nullptr, he, vec, coef, nullptr, msg), "(none)");
    CHECK_STR("a negative strength attracts", field_set_error(3, kind, shape, pos, rot, he, vec, coef, ex, msg), "(none)");
    kind[1] = 3;
    CHECK_STR("kind", field_set_error(3, kind, shape, pos, rot, he, vec, coef, ex, msg), "force field 1: kind is neither ACCEL nor DRAG nor RADIAL");
    shape[1] = 0;  // the kind is said first
    CHECK_STR("kind first", field_set_error(3, kind, shape, pos, rot, he, vec, coef, ex, msg), "force field 1: kind is neither ACCEL nor DRAG nor RADIAL");
    kind[1] = PHYS_FIELD_DRAG;
    CHECK_STR("shape", field_set_error(3, kind, shape, pos, rot, he, vec, coef, ex, msg), "force field 1: shape is neither SPHERE nor BOX nor CAPSULE");
    shape[1] = PHYS_SHAPE_SPHERE;
    const char* nf = "force field 2: non-finite number";
    pos[7] = nan;  CHECK_STR("pos", field_set_error(3, kind, shape, pos, rot, he, vec, coef, ex, msg), nf);  pos[7] = -2;
    rot[9] = inf;  CHECK_STR("rot", field_set_error(3, kind, shape, pos, rot, he, vec, coef, ex, msg), nf);
    CHECK_STR("rot null: not looked at", field_set_error(3, kind, shape, pos, nullptr, he, vec, coef, ex, msg), "(none)");
    rot[9] = 0;
    he[6] = -inf;  CHECK_STR("half extent, non-finite before negative", field_set_error(3, kind, shape, pos, rot, he, vec, coef, ex, msg), nf);  he[6] = 0.5f;
    vec[8] = nan;  CHECK_STR("vec", field_set_error(3, kind, shape, pos, rot, he, vec, coef, ex, msg), nf);  vec[8] = 0;
    coef[4] = nan; CHECK_STR("coef", field_set_error(3, kind, shape, pos, rot, he, vec, coef, ex, msg), nf);  coef[4] = -3;
    he[2] = -1;
    CHECK_STR("negative half extent", field_set_error(3, kind, shape, pos, rot, he, vec, coef, ex, msg), "force field 0: negative half extent");
    coef[2] = -0.5f;  // several offend: the first index
    CHECK_STR("first index", field_set_error(3, kind, shape, pos, rot, he, vec, coef, ex, msg), "force field 0: negative half extent");
    he[2] = 1;
    CHECK_STR("negative linear drag", field_set_error(3, kind, shape, pos, rot, he, vec, coef, ex, msg), "force field 1: negative drag coefficient");
    coef[2] = 0.5f; coef[3] = -0.25f;
    CHECK_STR("negative angular drag", field_set_error(3, kind, shape, pos, rot, he, vec, coef, ex, msg), "force field 1: negative drag coefficient");
    coef[3] = 0.25f; coef[5] = 0;
    CHECK_STR("r0 == 0", field_set_error(3, kind, shape, pos, rot, he, vec, coef, ex, msg), "force field 2: r0 (coef[1]) must be above 0");
    coef[5] = -1;
    CHECK_STR("r0 < 0", field_set_error(3, kind, shape, pos, rot, he, vec, coef, ex, msg), "force field 2: r0 (coef[1]) must be above 0");
    coef[5] = 1.5f; ex[2] = 3;
    CHECK_STR("exponent", field_set_error(3, kind, shape, pos, rot, he, vec, coef, ex, msg), "force field 2: exponent above 2");
    CHECK_STR("exponent null: 0", field_set_error(3, kind, shape, pos, rot, he, vec, coef, nullptr, msg), "(none)");
    ex[2] = 2;
    coef[0] = -7; coef[1] = -7;  // an ACCEL field reads no coefficient
    CHECK_STR("ACCEL coefficients are free", field_set_error(3, kind, shape, pos, rot, he, vec, coef, ex, msg), "(none)");

    // the staged set and its two updates
    const uint16_t mask[3] = {1, 2, 0xFFFF};
    FieldStaging st = stage_fields(3, kind, shape, pos, nullptr, he, mask, vec, coef, ex);
    ++g_checks;
    if (!(st.masked && st.drag && st.accel && st.staged.size() == 3 && ff_f2u(st.staged[2].s[0].x) == PHYS_FIELD_RADIAL &&
          ff_f2u(st.staged[2].s[0].y) == PHYS_SHAPE_CAPSULE && ff_f2u(st.staged[1].s[0].z) == 2u && ff_f2u(st.staged[2].s[0].w) == 2u &&
          st.staged[1].s[2].w == 1.0f && st.staged[1].s[2].x == 0.0f && st.staged[2].s[1].y == -2.0f && st.staged[1].s[3].w == 0.5f &&
          st.staged[1].s[4].w == 0.25f && st.staged[0].s[4].y == 9.81f)) {
        std::printf("MISMATCH stage_fields\n");
        return 1;
    }
    const FieldStaging plain = stage_fields(1, kind + 2, shape + 2, pos + 6, rot + 8, he + 6, nullptr, vec + 6, coef + 4, nullptr);
    ++g_checks;
    if (plain.masked || plain.drag || plain.accel || ff_f2u(plain.staged[0].s[0].z) != 0xFFFFu || ff_f2u(plain.staged[0].s[0].w) != 0u) {
        std::printf("MISMATCH stage_fields defaults\n");
        return 1;
    }
    float vec2[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, coef2[6] = {0, 0, 0, 0, 0, 1};
    CHECK_STR("params: strength 0 is fine", restage_field_params(st.staged, vec2, coef2, msg), "(none)");
    ++g_checks;
    if (st.staged[1].s[3].w != 0.0f || st.staged[2].s[4].w != 1.0f || st.staged[0].s[4].y != 0.0f) { std::printf("MISMATCH restage params\n"); return 1; }
    coef2[5] = 0;
    CHECK_STR("params: r0", restage_field_params(st.staged, vec2, coef2, msg), "force field 2: r0 (coef[1]) must be above 0");
    coef2[5] = 1; coef2[2] = -1;
    CHECK_STR("params: drag", restage_field_params(st.staged, vec2, coef2, msg), "force field 1: negative drag coefficient");
    coef2[2] = 0; vec2[1] = inf;
    CHECK_STR("params: non-finite", restage_field_params(st.staged, vec2, coef2, msg), "force field 0: non-finite number");
    ++g_checks;
    if (st.staged[2].s[4].w != 1.0f) { std::printf("MISMATCH a refused params call changed the set\n"); return 1; }
    float pos2[9] = {5, 5, 5, 6, 6, 6, 7, 7, 7};
    ++g_checks;
    if (!restage_field_poses(st.staged, pos2, nullptr) || st.staged[2].s[1].x != 7.0f || st.staged[2].s[2].w != 1.0f) { std::printf("MISMATCH restage poses\n"); return 1; }
    pos2[4] = nan;
    ++g_checks;
    if (restage_field_poses(st.staged, pos2, nullptr) || st.staged[1].s[1].x != 6.0f) { std::printf("MISMATCH non-finite poses\n"); return 1; }
    std::printf("%d checks passed\n", g_checks);
    return 0;
}

static uint32_t word(FILE* f) {
    unsigned v = 0;
    if (std::fscanf(f, "%x", &v) != 1) { std::fprintf(stderr, "scene file: short or malformed\n"); std::exit(2); }
    return (uint32_t)v;
}
static float real(FILE* f) { return ff_u2f(word(f)); }

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: field_probe --messages | <scene file>\n"); return 2; }
    if (std::strcmp(argv[1], "--messages") == 0) return messages();
    FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    const uint32_t nb = word(f), nf = word(f), has_rot = word(f), has_mask = word(f), has_exponent = word(f);
    if (nb > (1u << 20) || nf > PHYS_MAX_FORCE_FIELDS) { std::fprintf(stderr, "scene file: counts out of range\n"); return 2; }
    std::vector<ff_body> body(nb);
    std::vector<v3> force(nb), torque(nb);
    for (uint32_t i = 0; i < nb; ++i) {
        ff_body& b = body[i];
        b.x.x = real(f); b.x.y = real(f); b.x.z = real(f);
        b.v.x = real(f); b.v.y = real(f); b.v.z = real(f);
        b.w.x = real(f); b.w.y = real(f); b.w.z = real(f);
        b.mass = real(f);
        b.category = word(f);
        force[i].x = real(f); force[i].y = real(f); force[i].z = real(f);
        torque[i].x = real(f); torque[i].y = real(f); torque[i].z = real(f);
    }
    std::vector<uint32_t> kind(nf), shape(nf), ex(nf);
    std::vector<uint16_t> mask(nf);
    std::vector<float> pos(3 * nf), rot(4 * nf), he(3 * nf), vec(3 * nf), coef(2 * nf);
    for (uint32_t k = 0; k < nf; ++k) {
        kind[k] = word(f); shape[k] = word(f);
        for (int a = 0; a < 3; ++a) pos[3 * k + a] = real(f);
        for (int a = 0; a < 4; ++a) rot[4 * k + a] = real(f);
        for (int a = 0; a < 3; ++a) he[3 * k + a] = real(f);
        mask[k] = (uint16_t)word(f);
        for (int a = 0; a < 3; ++a) vec[3 * k + a] = real(f);
        for (int a = 0; a < 2; ++a) coef[2 * k + a] = real(f);
        ex[k] = word(f);
    }
    std::fclose(f);
    std::string msg;
    const float* rotp = has_rot ? rot.data() : nullptr;
    const uint32_t* exp = has_exponent ? ex.data() : nullptr;
    if (const char* bad = field_set_error(nf, kind.data(), shape.data(), pos.data(), rotp, he.data(), vec.data(), coef.data(), exp, msg)) {
        std::printf("refused: %s\n", bad);
        return 3;
    }
    const FieldStaging st = stage_fields(nf, kind.data(), shape.data(), pos.data(), rotp, he.data(), has_mask ? mask.data() : nullptr, vec.data(),
                                         coef.data(), exp);
    std::vector<ff_record> rec(nf);
    for (uint32_t k = 0; k < nf; ++k) rec[k] = ff_record_make(&st.staged[k]);
    for (uint32_t i = 0; i < nb; ++i) {
        ff_sum whole;
        whole.F = whole.T = v3_make(0.0f, 0.0f, 0.0f);
        whole.acted = 0;
        ff_accumulate(rec.data(), nf, &body[i], st.masked ? 1 : 0, &force[i], &torque[i], &whole);
        // the kernel walks the records in tiles of 32 with the same sums: the same bits
        ff_sum tiled = whole;
        tiled.acted = 0;
        for (uint32_t t0 = 0; t0 < nf; t0 += 32) ff_accumulate(rec.data() + t0, nf - t0 < 32 ? nf - t0 : 32, &body[i], st.masked ? 1 : 0, &force[i], &torque[i], &tiled);
        const v3 F = whole.acted ? whole.F : force[i], T = whole.acted ? whole.T : torque[i];
        if (tiled.acted != whole.acted || (whole.acted && std::memcmp(&tiled, &whole, sizeof(v3) * 2) != 0)) {
            std::printf("MISMATCH body %u: a tiled walk differs from one walk\n", i);
            return 1;
        }
        std::printf("%d %08x %08x %08x %08x %08x %08x\n", whole.acted, ff_f2u(F.x), ff_f2u(F.y), ff_f2u(F.z), ff_f2u(T.x), ff_f2u(T.y), ff_f2u(T.z));
    }
    return 0;
}
