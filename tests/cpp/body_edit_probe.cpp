// body_edit_probe.cpp — the body edits' arithmetic (include/spec/body_edit.h), the ordering and the checks of a batch on host
// arrays (physics_amd/csrc/setup.hpp edit_order) and phys_sync's reading of the bad-edit bit (readout.hpp) with a host
// compiler alone: no HIP, no library (tests/test_body_edit_cpu.py builds and runs it, once under the address and
// undefined-behaviour sanitizers; tests/test_gpu_body_edit.py holds the kernels to its output bit for bit).
//
//   body_edit_probe --checks        the hand cases of edit_order / edit_gather, the refusals, the runs, sync_error
//   body_edit_probe <scene file>    applies a batch of impulses or forces twice - one entry after another in the order given,
//                                   and as the kernels do: ordered by id, one walk per run - checks that both give the same
//                                   bits, and prints per body the bits of v, w (impulses) or F, T (forces) and of the nine
//                                   words of the inverse inertia it used
//
// Scene file, every number a 32-bit word in hex (floats by their bits):
//   mode (0 impulses, 1 forces)  n_bodies  n_entries  layout (0 one shared diagonal tensor, 1 a diagonal per body, 2 full 3x3)
//   has_point  has_third (ang_impulse / torque)
//   per body:  x[3] v[3] inv_mass w[3] mass inertia[9] F[3] T[3]   (the tensor as phys_set_bodies takes it: inverted here as
//              stage_bodies inverts it, zeros when singular)
//   per entry: id vec[3] point[3] third[3]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../physics_amd/csrc/readout.hpp"

using namespace phys;

static int g_checks = 0;
#define CHECK(what, cond)                                                              \
    do {                                                                               \
        ++g_checks;                                                                    \
        if (!(cond)) {                                                                 \
            std::printf("MISMATCH %s:%d  %s\n", __FILE__, __LINE__, what);             \
            std::exit(1);                                                              \
        }                                                                              \
    } while (0)

static bool same(const std::vector<uint32_t>& got, std::initializer_list<uint32_t> want) { return got == std::vector<uint32_t>(want); }

static int checks() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    std::vector<float> val(3 * 8, 1.0f);
    for (size_t k = 0; k < val.size(); ++k) val[k] = (float)k;
    // empty input: a no-op whatever the pointers
    EditOrder o = edit_order(EditKind::Impulses, {0, nullptr, {nullptr, nullptr, nullptr}}, 10);
    CHECK("empty", o.code == PHYS_OK && o.order.empty() && o.ids.empty());
    // one entry
    const uint32_t one[1] = {7};
    o = edit_order(EditKind::Impulses, {1, one, {val.data(), nullptr, nullptr}}, 10);
    CHECK("one entry", o.code == PHYS_OK && same(o.order, {0}) && same(o.ids, {7}));
    // all entries with one id: the order given
    const uint32_t all[4] = {3, 3, 3, 3};
    o = edit_order(EditKind::Forces, {4, all, {val.data(), nullptr, nullptr}}, 10);
    CHECK("one id", o.code == PHYS_OK && same(o.order, {0, 1, 2, 3}) && same(o.ids, {3, 3, 3, 3}));
    CHECK("one id: one run", be_leads(o.ids.data(), 0) && !be_leads(o.ids.data(), 1) && !be_leads(o.ids.data(), 3) &&
                                 be_run_end(o.ids.data(), 4, 0) == 4u);
    // descending ids
    const uint32_t desc[4] = {9, 6, 4, 0};
    o = edit_order(EditKind::Velocities, {4, desc, {val.data(), nullptr, nullptr}}, 10);
    CHECK("descending", o.code == PHYS_OK && same(o.order, {3, 2, 1, 0}) && same(o.ids, {0, 4, 6, 9}));
    for (uint32_t i = 0; i < 4; ++i) CHECK("descending: four runs", be_leads(o.ids.data(), i) && be_run_end(o.ids.data(), 4, i) == i + 1u);
    // the issue's case: stable, so the two 2s and the two 5s keep the caller's order
    const uint32_t mix[5] = {5, 2, 5, 2, 9};
    o = edit_order(EditKind::Impulses, {5, mix, {val.data(), val.data(), nullptr}}, 10);
    CHECK("[5, 2, 5, 2, 9]", o.code == PHYS_OK && same(o.order, {1, 3, 0, 2, 4}) && same(o.ids, {2, 2, 5, 5, 9}));
    const uint32_t* s = o.ids.data();
    CHECK("run boundaries", be_leads(s, 0) && !be_leads(s, 1) && be_leads(s, 2) && !be_leads(s, 3) && be_leads(s, 4));
    CHECK("run ends", be_run_end(s, 5, 0) == 2u && be_run_end(s, 5, 2) == 4u && be_run_end(s, 5, 4) == 5u);
    for (uint32_t i = 0; i < 5; ++i) CHECK("ordered: nothing out of order", !be_out_of_order(s, i));
    CHECK("out of order", !be_out_of_order(mix, 0) && be_out_of_order(mix, 1) && !be_out_of_order(mix, 2) && be_out_of_order(mix, 3));
    const std::vector<float> g = edit_gather(o.order, val.data(), 3);
    CHECK("gather", g.size() == 15 && g[0] == 3.0f && g[2] == 5.0f && g[3] == 9.0f && g[6] == 0.0f && g[9] == 6.0f && g[12] == 12.0f);
    CHECK("gather: null stays null", edit_gather(o.order, (const float*)nullptr, 3).empty());
    const std::vector<float> g4 = edit_gather(o.order, val.data(), 4);
    CHECK("gather: four columns", g4.size() == 20 && g4[0] == 4.0f && g4[7] == 15.0f && g4[8] == 0.0f);
    // the refusals: nothing is ordered, the code and a text
    const uint32_t edge[2] = {1, 10};
    o = edit_order(EditKind::Poses, {2, edge, {val.data(), nullptr, nullptr}}, 10);
    CHECK("id == n_owned", o.code == PHYS_ERR_OUT_OF_RANGE && o.order.empty() && !o.message.empty());
    o = edit_order(EditKind::Poses, {2, edge, {val.data(), nullptr, nullptr}}, 11);
    CHECK("id == n_owned - 1", o.code == PHYS_OK);
    std::vector<float> bad(val);
    bad[4] = nan;
    o = edit_order(EditKind::Impulses, {5, mix, {bad.data(), nullptr, nullptr}}, 10);
    CHECK("NaN", o.code == PHYS_ERR_INVALID_ARG && o.order.empty());
    bad[4] = 4.0f; bad[14] = inf;
    o = edit_order(EditKind::Forces, {5, mix, {val.data(), nullptr, bad.data()}}, 10);
    CHECK("inf in an optional array", o.code == PHYS_ERR_INVALID_ARG);
    bad[14] = -inf;
    o = edit_order(EditKind::Poses, {3, mix, {nullptr, bad.data(), nullptr}}, 10);  // rot: four columns, entries 0..2 = floats 0..11
    CHECK("values beyond the batch are not read", o.code == PHYS_OK);
    o = edit_order(EditKind::Poses, {4, mix, {nullptr, bad.data(), nullptr}}, 10);
    CHECK("-inf in rot", o.code == PHYS_ERR_INVALID_ARG);
    o = edit_order(EditKind::Impulses, {5, nullptr, {val.data(), nullptr, nullptr}}, 10);
    CHECK("null ids", o.code == PHYS_ERR_INVALID_ARG);
    o = edit_order(EditKind::Impulses, {5, mix, {nullptr, val.data(), nullptr}}, 10);
    CHECK("null impulse", o.code == PHYS_ERR_INVALID_ARG);
    o = edit_order(EditKind::Forces, {5, mix, {nullptr, nullptr, val.data()}}, 10);
    CHECK("null force", o.code == PHYS_ERR_INVALID_ARG);
    o = edit_order(EditKind::Poses, {5, mix, {nullptr, nullptr, nullptr}}, 10);
    CHECK("poses: both optional", o.code == PHYS_OK);
    o = edit_order(EditKind::Velocities, {5, mix, {nullptr, nullptr, nullptr}}, 10);
    CHECK("velocities: both optional", o.code == PHYS_OK);
    o = edit_order(EditKind::Impulses, {1ull << 31, mix, {val.data(), nullptr, nullptr}}, 10);
    CHECK("n >= 2^31", o.code == PHYS_ERR_INVALID_ARG);
    CHECK("device checks: fine", edit_args_error(EditKind::Impulses, {5, mix, {val.data(), nullptr, nullptr}}) == nullptr);
    CHECK("device checks: n == 0", edit_args_error(EditKind::Impulses, {0, nullptr, {nullptr, nullptr, nullptr}}) == nullptr);
    CHECK("device checks: null ids", edit_args_error(EditKind::Poses, {5, nullptr, {val.data(), nullptr, nullptr}}) != nullptr);
    CHECK("device checks: null force", edit_args_error(EditKind::Forces, {5, mix, {nullptr, nullptr, nullptr}}) != nullptr);
    CHECK("columns", edit_cols(EditKind::Poses, 0) == 3 && edit_cols(EditKind::Poses, 1) == 4 && edit_cols(EditKind::Poses, 2) == 0 &&
                         edit_cols(EditKind::Velocities, 1) == 3 && edit_cols(EditKind::Velocities, 2) == 0 &&
                         edit_cols(EditKind::Impulses, 2) == 3 && edit_cols(EditKind::Forces, 1) == 3);

    // phys_sync: the bad-edit bit is an argument error, behind every other bit; bit 7 reads as it did
    const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    static_assert(kOvfBadEdit == 0x100u, "the bit the header documents");
    const SyncError capacity = sync_error(kOvfPairs, zero);
    SyncError e = sync_error(0x100u, zero);
    CHECK("sync_error(0x100)", e.code == PHYS_ERR_INVALID_ARG && e.message.find("body edit") != std::string::npos);
    e = sync_error(0x100u | kOvfPairs, zero);
    CHECK("sync_error(0x100 | pairs)", e.code == PHYS_ERR_CAPACITY && e.message == capacity.message);
    e = sync_error(0x80u, zero);
    CHECK("sync_error(0x80)", e.code == PHYS_ERR_CAPACITY && e.message == capacity.message);
    e = sync_error(0x100u | kOvfHandoff, zero);
    CHECK("sync_error(0x100 | hand-off)", e.code == PHYS_ERR_HIP);
    e = sync_error(0x100u | kOvfColors, zero);
    CHECK("sync_error(0x100 | colours)", e.code == PHYS_ERR_CAPACITY && e.message != capacity.message);
    CHECK("sync_error(0)", sync_error(0, zero).code == PHYS_OK);
    std::printf("%d checks passed\n", g_checks);
    return 0;
}

static uint32_t word(FILE* f) {
    unsigned v = 0;
    if (std::fscanf(f, "%x", &v) != 1) { std::fprintf(stderr, "scene file: short or malformed\n"); std::exit(2); }
    return (uint32_t)v;
}
static float real(FILE* f) {
    const uint32_t u = word(f);
    float x;
    std::memcpy(&x, &u, 4);
    return x;
}
static v3 real3(FILE* f) { v3 r; r.x = real(f); r.y = real(f); r.z = real(f); return r; }
static uint32_t bits(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }

struct Body { v3 x, v, w, F, T; float inv_mass, mass; m33 I; };

// one entry on its body: the header's functions, with the tensor the layout selects (0: body 0's diagonal for everyone)
static void apply(uint32_t mode, uint32_t layout, std::vector<Body>& body, uint32_t id, v3 vec, int has_point, v3 point, int has_third, v3 third) {
    Body& b = body[id];
    if (mode == 0) {
        const Body& t = body[layout == 0 ? 0 : id];
        be_impulse(b.x, b.inv_mass, layout != 2, v3_make(t.I.m[0], t.I.m[4], t.I.m[8]), &b.I, vec, has_point, point, has_third, third, &b.v, &b.w);
    } else {
        be_force(b.x, vec, has_point, point, has_third, third, &b.F, &b.T);
    }
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: body_edit_probe --checks | <scene file>\n"); return 2; }
    if (std::strcmp(argv[1], "--checks") == 0) return checks();
    FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    const uint32_t mode = word(f), nb = word(f), ne = word(f), layout = word(f), has_point = word(f), has_third = word(f);
    if (mode > 1 || layout > 2 || nb > (1u << 20) || ne > (1u << 20)) { std::fprintf(stderr, "scene file: header out of range\n"); return 2; }
    std::vector<Body> body(nb);
    for (Body& b : body) {
        b.x = real3(f); b.v = real3(f); b.inv_mass = real(f); b.w = real3(f); b.mass = real(f);
        m33 given;
        for (int k = 0; k < 9; ++k) given.m[k] = real(f);
        if (!m33_try_inverse(&given, &b.I))
            for (int k = 0; k < 9; ++k) b.I.m[k] = 0.0f;
        b.F = real3(f); b.T = real3(f);
    }
    std::vector<uint32_t> ids(ne);
    std::vector<float> vec(3 * (size_t)ne), point(3 * (size_t)ne), third(3 * (size_t)ne);
    for (uint32_t k = 0; k < ne; ++k) {
        ids[k] = word(f);
        for (int a = 0; a < 3; ++a) vec[3 * k + a] = real(f);
        for (int a = 0; a < 3; ++a) point[3 * k + a] = real(f);
        for (int a = 0; a < 3; ++a) third[3 * k + a] = real(f);
    }
    std::fclose(f);
    const EditKind kind = mode == 0 ? EditKind::Impulses : EditKind::Forces;
    const EditBatch batch = {ne, ids.data(), {vec.data(), has_point ? point.data() : nullptr, has_third ? third.data() : nullptr}};
    const EditOrder o = edit_order(kind, batch, nb);
    if (o.code != PHYS_OK) {
        std::printf("refused %d: %s\n", o.code, o.message.c_str());
        return 3;
    }
    const auto at = [](const std::vector<float>& a, uint32_t k) { return v3_make(a[3 * k], a[3 * k + 1], a[3 * k + 2]); };
    // one entry after another, in the order given
    std::vector<Body> seq(body);
    for (uint32_t k = 0; k < ne; ++k) apply(mode, layout, seq, ids[k], at(vec, k), (int)has_point, at(point, k), (int)has_third, at(third, k));
    // as the kernels do: ordered by id, each leader walks its run
    std::vector<Body> run(body);
    const std::vector<float> svec = edit_gather(o.order, vec.data(), 3), spoint = edit_gather(o.order, point.data(), 3),
                             sthird = edit_gather(o.order, third.data(), 3);
    for (uint32_t i = 0; i < ne; ++i) {
        if (!be_leads(o.ids.data(), i) || be_out_of_order(o.ids.data(), i)) continue;
        const uint32_t end = be_run_end(o.ids.data(), ne, i);
        for (uint32_t j = i; j < end; ++j) apply(mode, layout, run, o.ids[i], at(svec, j), (int)has_point, at(spoint, j), (int)has_third, at(sthird, j));
    }
    for (uint32_t i = 0; i < nb; ++i) {
        const v3 a[4] = {seq[i].v, seq[i].w, seq[i].F, seq[i].T}, b[4] = {run[i].v, run[i].w, run[i].F, run[i].T};
        if (std::memcmp(a, b, sizeof(a)) != 0) {
            std::printf("MISMATCH body %u: the walk over runs differs from one entry after another\n", i);
            return 1;
        }
        const v3 p = mode == 0 ? seq[i].v : seq[i].F, q = mode == 0 ? seq[i].w : seq[i].T;
        std::printf("%08x %08x %08x %08x %08x %08x", bits(p.x), bits(p.y), bits(p.z), bits(q.x), bits(q.y), bits(q.z));
        for (int k = 0; k < 9; ++k) std::printf(" %08x", bits(body[i].I.m[k]));
        std::printf("\n");
    }
    return 0;
}
