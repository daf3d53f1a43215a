// staging_probe.cpp — the query calls' host-only part (physics_amd/csrc/staging.hpp) against cases: where a call's arrays lie
// in its staging buffer, what the cast entry points refuse, and the bound on the number of arrays. Built by a host compiler
// alone with -fsanitize=address,undefined (tests/test_staging_cpu.py), so a write past StageLayout::arrays would end the run;
// exits non-zero at the first mismatch. The expected offsets are worked out BY HAND from the rules of the staging code as it
// stood in abi.hip: the arrays in declaration order, each at the next multiple of its alignment (that
// of its element, 16 for the overlap's rot), a null array taking no room. The sums are written next to each case.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../physics_amd/csrc/staging.hpp"

using namespace phys;

static int g_checks = 0;
#define CHECK(what, got, want)                                                                                          \
    do {                                                                                                                \
        ++g_checks;                                                                                                     \
        const long long g_ = (long long)(got), w_ = (long long)(want);                                                  \
        if (g_ != w_) {                                                                                                 \
            std::printf("MISMATCH %s:%d  %s: %s = %lld, expected %lld\n", __FILE__, __LINE__, what, #got, g_, w_);      \
            std::exit(1);                                                                                               \
        }                                                                                                               \
    } while (0)
#define CHECK_STR(what, got, want)                                                                                      \
    do {                                                                                                                \
        ++g_checks;                                                                                                     \
        const char* g_ = (got);                                                                                         \
        const std::string w_ = (want);                                                                                  \
        if (!g_ || w_ != g_) {                                                                                          \
            std::printf("MISMATCH %s:%d  %s:\n  got      \"%s\"\n  expected \"%s\"\n", __FILE__, __LINE__, what, g_ ? g_ : "(null)", w_.c_str()); \
            std::exit(1);                                                                                               \
        }                                                                                                               \
    } while (0)

// host arrays of up to 3 queries (their contents are never read here) and two stand-ins for the device buffers
static float g_origin[9], g_dir[9], g_rot[12], g_radius[3], g_half[3], g_max_t[3], g_normal[9], g_point[9], g_t[3];
static uint32_t g_ignore[3], g_body[3];
static uint16_t g_mask[3];
alignas(16) static uint8_t g_in[256], g_out[256];

static CastBatch full(uint64_t n) {
    return {n, g_origin, g_dir, g_rot, g_radius, g_half, g_max_t, g_ignore, g_mask, g_body, g_t, g_normal, g_point};
}

// offset of a staged array in its buffer, -1 for "no device pointer"
static long long off(const void* p, const uint8_t* base) { return p ? (long long)((const uint8_t*)p - base) : -1; }

struct Want { long long origin, dir, rot, radius, half_length, max_t, ignore_body, query_mask, in_total, body_out, t_out, normal_out, point_out, out_total; };

static void check_cast(const char* what, const CastBatch& b, const Want& w) {
    StageLayout in, out;
    stage_cast(b, in, out);
    CHECK(what, in.refused || out.refused, 0);
    CHECK(what, in.total, w.in_total);
    CHECK(what, out.total, w.out_total);
    const CastBatch d = staged_cast(b, g_in, g_out);
    CHECK(what, d.n, b.n);
    CHECK(what, off(d.origin, g_in), w.origin); CHECK(what, off(d.dir, g_in), w.dir); CHECK(what, off(d.rot, g_in), w.rot);
    CHECK(what, off(d.radius, g_in), w.radius); CHECK(what, off(d.half_length, g_in), w.half_length);
    CHECK(what, off(d.max_t, g_in), w.max_t); CHECK(what, off(d.ignore_body, g_in), w.ignore_body);
    CHECK(what, off(d.query_mask, g_in), w.query_mask);
    CHECK(what, off(d.body_out, g_out), w.body_out); CHECK(what, off(d.t_out, g_out), w.t_out);
    CHECK(what, off(d.normal_out, g_out), w.normal_out); CHECK(what, off(d.point_out, g_out), w.point_out);
    // what copy() moves: every array that is there, from its host array, its whole length, to where the kernel is pointed
    int present_in = 0, present_out = 0;
    for (const void* p : {(const void*)d.origin, (const void*)d.dir, (const void*)d.rot, (const void*)d.radius, (const void*)d.half_length,
                          (const void*)d.max_t, (const void*)d.ignore_body, (const void*)d.query_mask})
        if (p) CHECK(what, in.arrays[present_in++].offset, off(p, g_in));
    for (const void* p : {(const void*)d.body_out, (const void*)d.t_out, (const void*)d.normal_out, (const void*)d.point_out})
        if (p) CHECK(what, out.arrays[present_out++].offset, off(p, g_out));
    CHECK(what, in.count, present_in);
    CHECK(what, out.count, present_out);
    CHECK(what, in.arrays[0].host == (void*)b.origin, 1);
    CHECK(what, in.arrays[0].bytes, 12 * b.n);
    CHECK(what, out.arrays[0].host == (void*)b.body_out, 1);
    CHECK(what, out.arrays[0].bytes, 4 * b.n);
    if (b.query_mask) { CHECK(what, in.arrays[in.count - 1].host == (void*)b.query_mask, 1); CHECK(what, in.arrays[in.count - 1].bytes, 2 * b.n); }
}

static void cast_layout() {
    // n = 3: a float3 array is 36 bytes, a scalar array 12, rot 48, the u16 mask 6. Inputs, all there:
    //   origin 0..36, dir 36..72, rot 72..120, radius 120..132, half_length 132..144, max_t 144..156, ignore 156..168, mask 168..174
    // outputs: body 0..12, t 12..24, normal 24..60, point 60..96
    check_cast("all", full(3), {0, 36, 72, 120, 132, 144, 156, 168, 174, 0, 12, 24, 60, 96});
    CastBatch b = full(3);
    b.rot = nullptr;  // everything behind it 48 bytes lower
    check_cast("no rot", b, {0, 36, -1, 72, 84, 96, 108, 120, 126, 0, 12, 24, 60, 96});
    b = full(3); b.max_t = nullptr;  // ignore and mask 12 lower
    check_cast("no max_t", b, {0, 36, 72, 120, 132, -1, 144, 156, 162, 0, 12, 24, 60, 96});
    b = full(3); b.ignore_body = nullptr;  // the mask 12 lower
    check_cast("no ignore", b, {0, 36, 72, 120, 132, 144, -1, 156, 162, 0, 12, 24, 60, 96});
    b = full(3); b.query_mask = nullptr;  // the plain call: 6 bytes fewer
    check_cast("no mask", b, {0, 36, 72, 120, 132, 144, 156, -1, 168, 0, 12, 24, 60, 96});
    b = full(3); b.normal_out = nullptr;  // point where normal was
    check_cast("no normal", b, {0, 36, 72, 120, 132, 144, 156, 168, 174, 0, 12, -1, 24, 60});
    b = full(3); b.point_out = nullptr;
    check_cast("no point", b, {0, 36, 72, 120, 132, 144, 156, 168, 174, 0, 12, 24, -1, 60});
    // n = 1: 12, 12, 16, 4, 4, 4, 4, 2 bytes: 0, 12, 24, 40, 44, 48, 52, 56..58; outputs 4, 4, 12, 12: 0, 4, 8, 20..32
    check_cast("one", full(1), {0, 12, 24, 40, 44, 48, 52, 56, 58, 0, 4, 8, 20, 32});
    // the ray and ball calls are the same walk without rot, half_length and point_out (and, for rays, radius): what their own
    // declarations gave. Balls: origin 0, dir 36, radius 72, max_t 84, ignore 96, mask 108..114; rays: max_t 72, ignore 84, mask 96..102
    b = full(3); b.rot = nullptr; b.half_length = nullptr; b.point_out = nullptr;
    check_cast("ball", b, {0, 36, -1, 72, -1, 84, 96, 108, 114, 0, 12, 24, -1, 60});
    b.radius = nullptr;
    check_cast("ray", b, {0, 36, -1, -1, -1, 72, 84, 96, 102, 0, 12, 24, -1, 60});
    // every optional array absent at once (a ray): origin, dir alone, body and t alone
    b.max_t = nullptr; b.ignore_body = nullptr; b.query_mask = nullptr; b.normal_out = nullptr;
    check_cast("bare ray", b, {0, 36, -1, -1, -1, -1, -1, -1, 72, 0, 12, -1, -1, 24});
}

// phys_overlap's declaration order (abi.hip overlap_host): shape_type, pos, half_extent, ignore_body, rot at 16 bytes, query_mask
struct OverlapWant { long long type, pos, he, ignore, rot, mask, total; };
static void check_overlap(const char* what, uint64_t n, bool with_ignore, bool with_rot, bool with_mask, const OverlapWant& w) {
    StageLayout in;
    const auto s_type = in.add(g_body, n);
    const auto s_pos = in.add(g_origin, 3 * n), s_he = in.add(g_dir, 3 * n);
    const auto s_ignore = in.add(with_ignore ? g_ignore : nullptr, n);
    const auto s_rot = in.add(with_rot ? g_rot : nullptr, 4 * n, 16);
    const auto s_mask = in.add(with_mask ? g_mask : nullptr, n);
    CHECK(what, in.refused, 0);
    CHECK(what, off(in.at(g_in, s_type), g_in), w.type); CHECK(what, off(in.at(g_in, s_pos), g_in), w.pos);
    CHECK(what, off(in.at(g_in, s_he), g_in), w.he); CHECK(what, off(in.at(g_in, s_ignore), g_in), w.ignore);
    CHECK(what, off(in.at(g_in, s_rot), g_in), w.rot); CHECK(what, off(in.at(g_in, s_mask), g_in), w.mask);
    CHECK(what, in.total, w.total);
}

static void overlap_layout() {
    // n = 3: type 0..12, pos 12..48, he 48..84, ignore 84..96, rot at 96 (a multiple of 16 as it stands) ..144, mask 144..150
    check_overlap("all", 3, true, true, true, {0, 12, 48, 84, 96, 144, 150});
    // without ignore the inputs end at 84: rot is padded up to 96 all the same
    check_overlap("no ignore", 3, false, true, true, {0, 12, 48, -1, 96, 144, 150});
    check_overlap("no rot", 3, true, false, true, {0, 12, 48, 84, -1, 96, 102});
    check_overlap("no mask", 3, true, true, false, {0, 12, 48, 84, 96, -1, 144});
    // n = 1: type 0..4, pos 4..16, he 16..28, ignore 28..32, rot 32..48, mask 48..50; without ignore rot is padded from 28 to 32
    check_overlap("one", 1, true, true, true, {0, 4, 16, 28, 32, 48, 50});
    check_overlap("one, no ignore", 1, false, true, true, {0, 4, 16, -1, 32, 48, 50});
    // n = 2: the inputs end at 8 + 24 + 24 + 8 = 64 (no padding), without ignore at 56: rot at 64 both times, ..96, mask ..100
    check_overlap("two", 2, true, true, true, {0, 8, 32, 56, 64, 96, 100});
    check_overlap("two, no ignore", 2, false, true, true, {0, 8, 32, -1, 64, 96, 100});
    // a 4-byte array behind the 6 bytes of three u16 masks starts at 8, not at 6
    StageLayout l;
    const auto s_mask = l.add(g_mask, 3);
    const auto s_word = l.add(g_ignore, 3);
    CHECK("padding", off(l.at(g_in, s_mask), g_in), 0);
    CHECK("padding", off(l.at(g_in, s_word), g_in), 8);
    CHECK("padding", l.total, 20);
}

// the ninth array is refused: not written anywhere, the eight before it as they were (the sanitizers watch the rest)
static void bound() {
    static_assert(StageLayout::kMaxArrays == 8, "the cases below declare kMaxArrays + 1 arrays");
    StageLayout l;
    StageLayout::Slot<float> s[9];
    for (int k = 0; k < 9; ++k) s[k] = l.add(g_radius, 3);
    CHECK("bound", l.refused, 1);
    CHECK("bound", l.count, 8);
    CHECK("bound", l.total, 8 * 12);
    CHECK("bound", s[7].index, 7);
    CHECK("bound", off(l.at(g_in, s[7]), g_in), 84);
    CHECK("bound", s[8].index, -1);
    CHECK("bound", l.at(g_in, s[8]) == nullptr, 1);
    (void)l.add(g_radius, 3);  // and again
    CHECK("bound", l.count, 8);
    CHECK("bound", l.at(g_in, StageLayout::Slot<float>{8}) == nullptr, 1);   // no slot reaches past the declared arrays
    CHECK("bound", l.at(g_in, StageLayout::Slot<float>{1000}) == nullptr, 1);
    // a null array is not counted: eight arrays and any number of absent ones fit
    StageLayout m;
    for (int k = 0; k < 8; ++k) { (void)m.add(g_radius, 3); (void)m.add((const float*)nullptr, 3); }
    CHECK("bound", m.refused, 0);
    CHECK("bound", m.count, 8);
}

// the argument check: the parent's texts, per family
static void cast_args() {
    struct Family { CastKind kind; const char* too_many; const char* null_array; bool radius, half_length; };
    const Family families[] = {
        {CastKind::Ray, "phys_raycast: n_rays must be below 2^31", "phys_raycast: null origin, dir, body_out or t_out", false, false},
        {CastKind::Sphere, "phys_spherecast: n must be below 2^31", "phys_spherecast: null origin, dir, radius, body_out or t_out", true, false},
        {CastKind::Capsule, "phys_capsulecast: n must be below 2^31",
         "phys_capsulecast: null origin, dir, radius, half_length, body_out or t_out", true, true},
    };
    for (const Family& f : families) {
        CastBatch b = full(3);
        CHECK("args", cast_args_error(f.kind, b) == nullptr, 1);
        // each required pointer null in turn
        b = full(3); b.origin = nullptr; CHECK_STR("origin", cast_args_error(f.kind, b), f.null_array);
        b = full(3); b.dir = nullptr; CHECK_STR("dir", cast_args_error(f.kind, b), f.null_array);
        b = full(3); b.body_out = nullptr; CHECK_STR("body_out", cast_args_error(f.kind, b), f.null_array);
        b = full(3); b.t_out = nullptr; CHECK_STR("t_out", cast_args_error(f.kind, b), f.null_array);
        b = full(3); b.radius = nullptr;
        if (f.radius) CHECK_STR("radius", cast_args_error(f.kind, b), f.null_array);
        else CHECK("radius", cast_args_error(f.kind, b) == nullptr, 1);
        b = full(3); b.half_length = nullptr;
        if (f.half_length) CHECK_STR("half_length", cast_args_error(f.kind, b), f.null_array);
        else CHECK("half_length", cast_args_error(f.kind, b) == nullptr, 1);
        // the optional ones, one at a time and all at once
        b = full(3); b.rot = nullptr; CHECK("rot", cast_args_error(f.kind, b) == nullptr, 1);
        b = full(3); b.max_t = nullptr; CHECK("max_t", cast_args_error(f.kind, b) == nullptr, 1);
        b = full(3); b.ignore_body = nullptr; CHECK("ignore_body", cast_args_error(f.kind, b) == nullptr, 1);
        b = full(3); b.query_mask = nullptr; CHECK("query_mask", cast_args_error(f.kind, b) == nullptr, 1);
        b = full(3); b.normal_out = nullptr; CHECK("normal_out", cast_args_error(f.kind, b) == nullptr, 1);
        b = full(3); b.point_out = nullptr; CHECK("point_out", cast_args_error(f.kind, b) == nullptr, 1);
        b = full(3); b.rot = nullptr; b.max_t = nullptr; b.ignore_body = nullptr; b.query_mask = nullptr; b.normal_out = nullptr; b.point_out = nullptr;
        CHECK("optional", cast_args_error(f.kind, b) == nullptr, 1);
        // the count: 2^31 - 1 passes, 2^31 does not, and that is said before a null array is
        b = full((1ull << 31) - 1); CHECK("n", cast_args_error(f.kind, b) == nullptr, 1);
        b = full(1ull << 31); CHECK_STR("n", cast_args_error(f.kind, b), f.too_many);
        b = CastBatch{}; b.n = 1ull << 31; CHECK_STR("n", cast_args_error(f.kind, b), f.too_many);
        b = full(~0ull); CHECK_STR("n", cast_args_error(f.kind, b), f.too_many);
        // no queries: nothing is required
        b = CastBatch{}; CHECK("empty", cast_args_error(f.kind, b) == nullptr, 1);
    }
}

int main() {
    cast_layout();
    overlap_layout();
    bound();
    cast_args();
    std::printf("staging_probe: %d checks passed\n", g_checks);
    return 0;
}
