// staging_probe.cpp — the query calls' host-only part (physics_amd/csrc/staging.hpp) against cases: where a call's arrays lie
// in its staging buffers (casts, move-and-slide, character walking, depenetration, overlaps), what their entry points refuse,
// and the bound on the number of arrays. Built by a host compiler
// alone with -fsanitize=address,undefined (tests/test_staging_cpu.py), so a write past StageLayout::arrays would end the run;
// exits non-zero at the first mismatch. The expected offsets are worked out BY HAND from the rules of the staging code as it
// stood in abi.hip: the arrays in declaration order, each at the next multiple of its alignment (that
// of its element, 16 for the overlap's rot), a null array taking no room. The sums are written next to each case.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>
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

// host arrays of up to 3 queries (their contents are never read here) and three stand-ins for the device buffers
static float g_origin[9], g_dir[9], g_rot[12], g_radius[3], g_half[3], g_max_t[3], g_normal[9], g_point[9], g_t[3];
static uint32_t g_ignore[3], g_body[3];
static uint16_t g_mask[3];
// ... of the capsule query calls: per query, and up to 4 hit slots per query
static float g_pos_out[9], g_remaining[9], g_floor_normal[9], g_floor_point[9], g_hit_normal[36], g_hit_point[36], g_hit_depth[12];
static uint32_t g_grounded[3], g_status[3], g_floor_body[3], g_hit_body[12];
alignas(16) static uint8_t g_in[512], g_out[512], g_slots[512];
static uint8_t* const g_base[3] = {g_in, g_out, g_slots};  // inputs, per-query outputs, the character's hit slots

static CastBatch full(uint64_t n) {
    return {n, g_origin, g_dir, g_rot, g_radius, g_half, g_max_t, g_ignore, g_mask, g_body, g_t, g_normal, g_point};
}

// offset of a staged array in its buffer, -1 for "no device pointer"
static long long off(const void* p, const uint8_t* base) { return p ? (long long)((const uint8_t*)p - base) : -1; }

struct Want { long long origin, dir, rot, radius, half_length, max_t, ignore_body, query_mask, in_total, body_out, t_out, normal_out, point_out, out_total; };

static void check_cast(const char* what, const CastBatch& b, const Want& w) {
    StageLayout l[3];
    stage(b, l);
    const StageLayout &in = l[0], &out = l[1];
    CHECK(what, l[2].count, 0);
    CHECK(what, in.refused || out.refused, 0);
    CHECK(what, in.total, w.in_total);
    CHECK(what, out.total, w.out_total);
    const CastBatch d = staged(b, g_base);
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
        CHECK("args", args_error(f.kind, b) == nullptr, 1);
        // each required pointer null in turn
        b = full(3); b.origin = nullptr; CHECK_STR("origin", args_error(f.kind, b), f.null_array);
        b = full(3); b.dir = nullptr; CHECK_STR("dir", args_error(f.kind, b), f.null_array);
        b = full(3); b.body_out = nullptr; CHECK_STR("body_out", args_error(f.kind, b), f.null_array);
        b = full(3); b.t_out = nullptr; CHECK_STR("t_out", args_error(f.kind, b), f.null_array);
        b = full(3); b.radius = nullptr;
        if (f.radius) CHECK_STR("radius", args_error(f.kind, b), f.null_array);
        else CHECK("radius", args_error(f.kind, b) == nullptr, 1);
        b = full(3); b.half_length = nullptr;
        if (f.half_length) CHECK_STR("half_length", args_error(f.kind, b), f.null_array);
        else CHECK("half_length", args_error(f.kind, b) == nullptr, 1);
        // the optional ones, one at a time and all at once
        b = full(3); b.rot = nullptr; CHECK("rot", args_error(f.kind, b) == nullptr, 1);
        b = full(3); b.max_t = nullptr; CHECK("max_t", args_error(f.kind, b) == nullptr, 1);
        b = full(3); b.ignore_body = nullptr; CHECK("ignore_body", args_error(f.kind, b) == nullptr, 1);
        b = full(3); b.query_mask = nullptr; CHECK("query_mask", args_error(f.kind, b) == nullptr, 1);
        b = full(3); b.normal_out = nullptr; CHECK("normal_out", args_error(f.kind, b) == nullptr, 1);
        b = full(3); b.point_out = nullptr; CHECK("point_out", args_error(f.kind, b) == nullptr, 1);
        b = full(3); b.rot = nullptr; b.max_t = nullptr; b.ignore_body = nullptr; b.query_mask = nullptr; b.normal_out = nullptr; b.point_out = nullptr;
        CHECK("optional", args_error(f.kind, b) == nullptr, 1);
        // the count: 2^31 - 1 passes, 2^31 does not, and that is said before a null array is
        b = full((1ull << 31) - 1); CHECK("n", args_error(f.kind, b) == nullptr, 1);
        b = full(1ull << 31); CHECK_STR("n", args_error(f.kind, b), f.too_many);
        b = CastBatch{}; b.n = 1ull << 31; CHECK_STR("n", args_error(f.kind, b), f.too_many);
        b = full(~0ull); CHECK_STR("n", args_error(f.kind, b), f.too_many);
        // no queries: nothing is required
        b = CastBatch{}; CHECK("empty", args_error(f.kind, b) == nullptr, 1);
    }
}

// ---- the capsule query calls: move-and-slide, character walking, depenetration ----
// one array of a staged call: the device pointer it came out with, its host array, its buffer (0 inputs, 1 per-query outputs,
// 2 the character's hit slots), its bytes per query and its hand-worked offset (-1: the array is not there)
struct At { const void* dev; const void* host; int group; long long bytes_per_query, want; };

// every array where it is wanted, and what copy() moves: each array that is there, in declaration order, from its host array,
// its whole length, to where the kernel is pointed; the buffers as large as the sums say
static void check_arrays(const char* what, uint64_t n, std::initializer_list<At> arrays, const StageLayout (&l)[3], long long in_total,
                         long long out_total, long long slots_total) {
    int present[3] = {0, 0, 0};
    for (const At& a : arrays) {
        CHECK(what, off(a.dev, g_base[a.group]), a.want);
        CHECK(what, a.dev != nullptr, a.host != nullptr);
        if (!a.dev) continue;
        const StageLayout::Array& s = l[a.group].arrays[present[a.group]++];
        CHECK(what, s.offset, a.want);
        CHECK(what, s.host == a.host, 1);
        CHECK(what, s.bytes, a.bytes_per_query * (long long)n);
    }
    const long long totals[3] = {in_total, out_total, slots_total};
    for (int g = 0; g < 3; ++g) {
        CHECK(what, l[g].refused, 0);
        CHECK(what, l[g].count, present[g]);
        CHECK(what, l[g].total, totals[g]);
    }
}

static SlideBatch slide_full(uint64_t n) {
    return {n, g_origin, g_dir, g_rot, g_radius, g_half, 0.01f, 2u, g_ignore, g_mask, g_pos_out, g_remaining, g_status, g_hit_body, g_hit_normal, g_hit_point};
}
struct SlideWant { long long pos, motion, rot, radius, half_length, ignore_body, query_mask, in_total,
                             pos_out, remaining_out, status_out, hit_body_out, hit_normal_out, hit_point_out, out_total; };

static void check_slide(const char* what, const SlideBatch& b, const SlideWant& w) {
    StageLayout l[3];
    stage(b, l);
    const SlideBatch d = staged(b, g_base);
    CHECK(what, d.n, b.n); CHECK(what, d.max_slides, b.max_slides); CHECK(what, d.skin == b.skin, 1);
    // max_slides = 2: a slot array holds 2 per query
    check_arrays(what, b.n, {{d.pos, b.pos, 0, 12, w.pos}, {d.motion, b.motion, 0, 12, w.motion}, {d.rot, b.rot, 0, 16, w.rot},
                             {d.radius, b.radius, 0, 4, w.radius}, {d.half_length, b.half_length, 0, 4, w.half_length},
                             {d.ignore_body, b.ignore_body, 0, 4, w.ignore_body}, {d.query_mask, b.query_mask, 0, 2, w.query_mask},
                             {d.pos_out, b.pos_out, 1, 12, w.pos_out}, {d.remaining_out, b.remaining_out, 1, 12, w.remaining_out},
                             {d.status_out, b.status_out, 1, 4, w.status_out}, {d.hit_body_out, b.hit_body_out, 1, 8, w.hit_body_out},
                             {d.hit_normal_out, b.hit_normal_out, 1, 24, w.hit_normal_out}, {d.hit_point_out, b.hit_point_out, 1, 24, w.hit_point_out}},
                 l, w.in_total, w.out_total, 0);
}

static void slide_layout() {
    // n = 3, max_slides = 2: float3 arrays 36 bytes, scalars 12, rot 48, the mask 6; hit_body 2 * 3 * 4 = 24, hit_normal and
    // hit_point 3 * 2 * 3 * 4 = 72. Inputs: pos 0..36, motion 36..72, rot 72..120, radius 120..132, half_length 132..144,
    // ignore 144..156, mask 156..162. Outputs: pos_out 0..36, remaining 36..72, status 72..84, hit_body 84..108,
    // hit_normal 108..180, hit_point 180..252
    check_slide("all", slide_full(3), {0, 36, 72, 120, 132, 144, 156, 162, 0, 36, 72, 84, 108, 180, 252});
    SlideBatch b = slide_full(3);
    b.rot = nullptr;  // everything behind it 48 lower
    check_slide("no rot", b, {0, 36, -1, 72, 84, 96, 108, 114, 0, 36, 72, 84, 108, 180, 252});
    b = slide_full(3); b.ignore_body = nullptr;  // the mask 12 lower
    check_slide("no ignore", b, {0, 36, 72, 120, 132, -1, 144, 150, 0, 36, 72, 84, 108, 180, 252});
    b = slide_full(3); b.query_mask = nullptr;
    check_slide("no mask", b, {0, 36, 72, 120, 132, 144, -1, 156, 0, 36, 72, 84, 108, 180, 252});
    b = slide_full(3); b.remaining_out = nullptr;  // everything behind it 36 lower
    check_slide("no remaining", b, {0, 36, 72, 120, 132, 144, 156, 162, 0, -1, 36, 48, 72, 144, 216});
    b = slide_full(3); b.hit_body_out = nullptr;  // the two behind it 24 lower
    check_slide("no hit_body", b, {0, 36, 72, 120, 132, 144, 156, 162, 0, 36, 72, -1, 84, 156, 228});
    b = slide_full(3); b.hit_normal_out = nullptr;  // hit_point where it was
    check_slide("no hit_normal", b, {0, 36, 72, 120, 132, 144, 156, 162, 0, 36, 72, 84, -1, 108, 180});
    b = slide_full(3); b.hit_point_out = nullptr;
    check_slide("no hit_point", b, {0, 36, 72, 120, 132, 144, 156, 162, 0, 36, 72, 84, 108, -1, 180});
    // every optional array absent at once: pos, motion, radius, half_length; pos_out, status
    b = slide_full(3); b.rot = nullptr; b.ignore_body = nullptr; b.query_mask = nullptr;
    b.remaining_out = nullptr; b.hit_body_out = nullptr; b.hit_normal_out = nullptr; b.hit_point_out = nullptr;
    check_slide("bare", b, {0, 36, -1, 72, 84, -1, -1, 96, 0, -1, 36, -1, -1, -1, 48});
    // n = 1: 12, 12, 16, 4, 4, 4, 2 bytes: 0, 12, 24, 40, 44, 48, 52..54; outputs 12, 12, 4, 8, 24, 24: 0, 12, 24, 28, 36, 60..84
    check_slide("one", slide_full(1), {0, 12, 24, 40, 44, 48, 52, 54, 0, 12, 24, 28, 36, 60, 84});
}

static CharacterBatch character_full(uint64_t n) {
    return {n, g_origin, g_dir, g_rot, g_radius, g_half, g_grounded, 0.01f, 2u, 0.3f, 0.2f, 0.7071068f, g_ignore, g_mask, g_pos_out, g_remaining,
            g_status, g_floor_body, g_floor_normal, g_floor_point, g_hit_body, g_hit_normal, g_hit_point};
}
struct CharacterWant { long long pos, motion, rot, radius, half_length, grounded_in, ignore_body, query_mask, in_total,
                                 pos_out, remaining_out, status_out, floor_body_out, floor_normal_out, floor_point_out, out_total,
                                 hit_body_out, hit_normal_out, hit_point_out, slots_total; };

static void check_character(const char* what, const CharacterBatch& b, const CharacterWant& w) {
    StageLayout l[3];
    stage(b, l);
    const CharacterBatch d = staged(b, g_base);
    CHECK(what, d.n, b.n); CHECK(what, d.max_slides, b.max_slides);
    CHECK(what, d.skin == b.skin && d.step_height == b.step_height && d.snap_distance == b.snap_distance && d.min_floor_ny == b.min_floor_ny, 1);
    // max_slides = 2: a slot array holds 2 * 2 = 4 per query
    check_arrays(what, b.n, {{d.pos, b.pos, 0, 12, w.pos}, {d.motion, b.motion, 0, 12, w.motion}, {d.rot, b.rot, 0, 16, w.rot},
                             {d.radius, b.radius, 0, 4, w.radius}, {d.half_length, b.half_length, 0, 4, w.half_length},
                             {d.grounded_in, b.grounded_in, 0, 4, w.grounded_in}, {d.ignore_body, b.ignore_body, 0, 4, w.ignore_body},
                             {d.query_mask, b.query_mask, 0, 2, w.query_mask},
                             {d.pos_out, b.pos_out, 1, 12, w.pos_out}, {d.remaining_out, b.remaining_out, 1, 12, w.remaining_out},
                             {d.status_out, b.status_out, 1, 4, w.status_out}, {d.floor_body_out, b.floor_body_out, 1, 4, w.floor_body_out},
                             {d.floor_normal_out, b.floor_normal_out, 1, 12, w.floor_normal_out},
                             {d.floor_point_out, b.floor_point_out, 1, 12, w.floor_point_out},
                             {d.hit_body_out, b.hit_body_out, 2, 16, w.hit_body_out}, {d.hit_normal_out, b.hit_normal_out, 2, 48, w.hit_normal_out},
                             {d.hit_point_out, b.hit_point_out, 2, 48, w.hit_point_out}},
                 l, w.in_total, w.out_total, w.slots_total);
}

static void character_layout() {
    // n = 3, max_slides = 2 (4 slots per query): inputs pos 0..36, motion 36..72, rot 72..120, radius 120..132, half_length
    // 132..144, grounded 144..156, ignore 156..168, mask 168..174. Per-query outputs: pos_out 0..36, remaining 36..72, status
    // 72..84, floor_body 84..96, floor_normal 96..132, floor_point 132..168. Hit slots, a buffer of their own: hit_body
    // 4 * 3 * 4 = 48: 0..48, hit_normal 3 * 48 = 144: 48..192, hit_point 192..336. The three totals: 174, 168, 336
    check_character("all", character_full(3), {0, 36, 72, 120, 132, 144, 156, 168, 174, 0, 36, 72, 84, 96, 132, 168, 0, 48, 192, 336});
    CharacterBatch b = character_full(3);
    b.rot = nullptr;  // everything behind it 48 lower
    check_character("no rot", b, {0, 36, -1, 72, 84, 96, 108, 120, 126, 0, 36, 72, 84, 96, 132, 168, 0, 48, 192, 336});
    b = character_full(3); b.grounded_in = nullptr;  // ignore and mask 12 lower
    check_character("no grounded", b, {0, 36, 72, 120, 132, -1, 144, 156, 162, 0, 36, 72, 84, 96, 132, 168, 0, 48, 192, 336});
    b = character_full(3); b.ignore_body = nullptr;
    check_character("no ignore", b, {0, 36, 72, 120, 132, 144, -1, 156, 162, 0, 36, 72, 84, 96, 132, 168, 0, 48, 192, 336});
    b = character_full(3); b.query_mask = nullptr;
    check_character("no mask", b, {0, 36, 72, 120, 132, 144, 156, -1, 168, 0, 36, 72, 84, 96, 132, 168, 0, 48, 192, 336});
    b = character_full(3); b.remaining_out = nullptr;  // everything behind it 36 lower
    check_character("no remaining", b, {0, 36, 72, 120, 132, 144, 156, 168, 174, 0, -1, 36, 48, 60, 96, 132, 0, 48, 192, 336});
    b = character_full(3); b.floor_body_out = nullptr;  // the two behind it 12 lower
    check_character("no floor_body", b, {0, 36, 72, 120, 132, 144, 156, 168, 174, 0, 36, 72, -1, 84, 120, 156, 0, 48, 192, 336});
    b = character_full(3); b.floor_normal_out = nullptr;  // floor_point where it was
    check_character("no floor_normal", b, {0, 36, 72, 120, 132, 144, 156, 168, 174, 0, 36, 72, 84, -1, 96, 132, 0, 48, 192, 336});
    b = character_full(3); b.floor_point_out = nullptr;
    check_character("no floor_point", b, {0, 36, 72, 120, 132, 144, 156, 168, 174, 0, 36, 72, 84, 96, -1, 132, 0, 48, 192, 336});
    b = character_full(3); b.hit_body_out = nullptr;  // the two behind it 48 lower
    check_character("no hit_body", b, {0, 36, 72, 120, 132, 144, 156, 168, 174, 0, 36, 72, 84, 96, 132, 168, -1, 0, 144, 288});
    b = character_full(3); b.hit_normal_out = nullptr;  // hit_point where it was
    check_character("no hit_normal", b, {0, 36, 72, 120, 132, 144, 156, 168, 174, 0, 36, 72, 84, 96, 132, 168, 0, -1, 48, 192});
    b = character_full(3); b.hit_point_out = nullptr;
    check_character("no hit_point", b, {0, 36, 72, 120, 132, 144, 156, 168, 174, 0, 36, 72, 84, 96, 132, 168, 0, 48, -1, 192});
    // no hit slot wanted at all: the third buffer is empty
    b = character_full(3); b.hit_body_out = nullptr; b.hit_normal_out = nullptr; b.hit_point_out = nullptr;
    check_character("no slots", b, {0, 36, 72, 120, 132, 144, 156, 168, 174, 0, 36, 72, 84, 96, 132, 168, -1, -1, -1, 0});
    // n = 1: inputs 12, 12, 16, 4, 4, 4, 4, 2: 0, 12, 24, 40, 44, 48, 52, 56..58; outputs 12, 12, 4, 4, 12, 12: 0, 12, 24, 28, 32,
    // 44..56; slots 16, 48, 48: 0, 16, 64..112
    check_character("one", character_full(1), {0, 12, 24, 40, 44, 48, 52, 56, 58, 0, 12, 24, 28, 32, 44, 56, 0, 16, 64, 112});
}

// phys_depenetrate (probe = false, max_iters = 2) and phys_penetration (probe = true: max_iters 1, no pos_out and status_out,
// the slot arrays are the call's body_out, normal_out and depth_out)
static DepenBatch depen_full(uint64_t n, bool probe) {
    if (probe) return {n, g_origin, g_rot, g_radius, g_half, 0.0f, 1u, true, g_ignore, g_mask, nullptr, nullptr, g_hit_body, g_hit_normal, g_hit_depth};
    return {n, g_origin, g_rot, g_radius, g_half, 0.01f, 2u, false, g_ignore, g_mask, g_pos_out, g_status, g_hit_body, g_hit_normal, g_hit_depth};
}
struct DepenWant { long long pos, rot, radius, half_length, ignore_body, query_mask, in_total,
                             pos_out, status_out, hit_body_out, hit_normal_out, hit_depth_out, out_total; };

static void check_depen(const char* what, const DepenBatch& b, const DepenWant& w) {
    StageLayout l[3];
    stage(b, l);
    const DepenBatch d = staged(b, g_base);
    CHECK(what, d.n, b.n); CHECK(what, d.max_iters, b.max_iters); CHECK(what, d.probe, b.probe); CHECK(what, d.gap == b.gap, 1);
    const long long k = b.probe ? 1 : 2;  // slots per query
    check_arrays(what, b.n, {{d.pos, b.pos, 0, 12, w.pos}, {d.rot, b.rot, 0, 16, w.rot}, {d.radius, b.radius, 0, 4, w.radius},
                             {d.half_length, b.half_length, 0, 4, w.half_length}, {d.ignore_body, b.ignore_body, 0, 4, w.ignore_body},
                             {d.query_mask, b.query_mask, 0, 2, w.query_mask},
                             {d.pos_out, b.pos_out, 1, 12, w.pos_out}, {d.status_out, b.status_out, 1, 4, w.status_out},
                             {d.hit_body_out, b.hit_body_out, 1, 4 * k, w.hit_body_out}, {d.hit_normal_out, b.hit_normal_out, 1, 12 * k, w.hit_normal_out},
                             {d.hit_depth_out, b.hit_depth_out, 1, 4 * k, w.hit_depth_out}},
                 l, w.in_total, w.out_total, 0);
}

static void depen_layout() {
    // phys_depenetrate, n = 3, max_iters = 2. Inputs: pos 0..36, rot 36..84, radius 84..96, half_length 96..108, ignore 108..120,
    // mask 120..126. Outputs: pos_out 0..36, status 36..48, hit_body 2 * 3 * 4 = 24: 48..72, hit_normal 72: 72..144, hit_depth
    // 24: 144..168
    check_depen("all", depen_full(3, false), {0, 36, 84, 96, 108, 120, 126, 0, 36, 48, 72, 144, 168});
    DepenBatch b = depen_full(3, false);
    b.rot = nullptr;  // everything behind it 48 lower
    check_depen("no rot", b, {0, -1, 36, 48, 60, 72, 78, 0, 36, 48, 72, 144, 168});
    b = depen_full(3, false); b.ignore_body = nullptr;
    check_depen("no ignore", b, {0, 36, 84, 96, -1, 108, 114, 0, 36, 48, 72, 144, 168});
    b = depen_full(3, false); b.query_mask = nullptr;
    check_depen("no mask", b, {0, 36, 84, 96, 108, -1, 120, 0, 36, 48, 72, 144, 168});
    b = depen_full(3, false); b.hit_body_out = nullptr;  // the two behind it 24 lower
    check_depen("no hit_body", b, {0, 36, 84, 96, 108, 120, 126, 0, 36, -1, 48, 120, 144});
    b = depen_full(3, false); b.hit_normal_out = nullptr;  // hit_depth where it was
    check_depen("no hit_normal", b, {0, 36, 84, 96, 108, 120, 126, 0, 36, 48, -1, 72, 96});
    b = depen_full(3, false); b.hit_depth_out = nullptr;
    check_depen("no hit_depth", b, {0, 36, 84, 96, 108, 120, 126, 0, 36, 48, 72, -1, 144});
    // n = 1: inputs 12, 16, 4, 4, 4, 2: 0, 12, 28, 32, 36, 40..42; outputs 12, 4, 8, 24, 8: 0, 12, 16, 24, 48..56
    check_depen("one", depen_full(1, false), {0, 12, 28, 32, 36, 40, 42, 0, 12, 16, 24, 48, 56});
    // phys_penetration, n = 3: the same inputs; outputs body 0..12, normal 12..48, depth 48..60
    check_depen("probe", depen_full(3, true), {0, 36, 84, 96, 108, 120, 126, -1, -1, 0, 12, 48, 60});
    b = depen_full(3, true); b.rot = nullptr;
    check_depen("probe, no rot", b, {0, -1, 36, 48, 60, 72, 78, -1, -1, 0, 12, 48, 60});
    b = depen_full(3, true); b.ignore_body = nullptr;
    check_depen("probe, no ignore", b, {0, 36, 84, 96, -1, 108, 114, -1, -1, 0, 12, 48, 60});
    b = depen_full(3, true); b.query_mask = nullptr;
    check_depen("probe, no mask", b, {0, 36, 84, 96, 108, -1, 120, -1, -1, 0, 12, 48, 60});
    b = depen_full(3, true); b.hit_normal_out = nullptr;  // normal_out not wanted: depth where it was
    check_depen("probe, no normal", b, {0, 36, 84, 96, 108, 120, 126, -1, -1, 0, -1, 12, 24});
    // n = 1: outputs 4, 12, 4: 0, 4, 16..20
    check_depen("probe, one", depen_full(1, true), {0, 12, 28, 32, 36, 40, 42, -1, -1, 0, 4, 16, 20});
}

// ---- what the capsule query calls refuse: the parent's texts at their boundary values, in the parent's order ----
static const float kInf = std::numeric_limits<float>::infinity(), kNaN = std::numeric_limits<float>::quiet_NaN(),
                   kDenormal = std::numeric_limits<float>::denorm_min();

// the count: 2^31 - 1 passes, 2^31 does not, with or without arrays
template <class Batch, class Err>
static void check_count(Batch b, Err err, const char* text) {
    b.n = (1ull << 31) - 1; CHECK("n", err(b) == nullptr, 1);
    b.n = 1ull << 31; CHECK_STR("n", err(b), text);
    b.n = ~0ull; CHECK_STR("n", err(b), text);
}
// a length of the call (skin, max_gap, step_height, snap_distance): finite and not negative. -0 and FLT_MAX pass; +inf, NaN and
// anything below zero do not
template <class Batch, class Err>
static void check_length(Batch b, float Batch::*field, Err err, const char* text) {
    for (float ok : {-0.0f, 0.0f, kDenormal, FLT_MAX}) { b.*field = ok; CHECK(text, err(b) == nullptr, 1); }
    for (float bad : {kInf, kNaN, -kDenormal, -FLT_MAX, -kInf}) { b.*field = bad; CHECK_STR("length", err(b), text); }
}
// a count of rounds (max_slides, max_iters): 1 .. 8
template <class Batch, class Err>
static void check_rounds(Batch b, uint32_t Batch::*field, Err err, const char* text) {
    for (uint32_t ok : {1u, 8u}) { b.*field = ok; CHECK(text, err(b) == nullptr, 1); }
    for (uint32_t bad : {0u, 9u, ~0u}) { b.*field = bad; CHECK_STR("rounds", err(b), text); }
}
// a required array: null with n = 1 is refused, with n = 0 nothing is required; an optional one may be null
#define CHECK_REQUIRED(make, err, member, text)                                          \
    do {                                                                                 \
        auto b_ = make; b_.n = 1; b_.member = nullptr; CHECK_STR(#member, err(b_), text); \
        b_.n = 0; CHECK(#member, err(b_) == nullptr, 1);                                 \
    } while (0)
#define CHECK_OPTIONAL(make, err, member)                                                \
    do { auto b_ = make; b_.n = 1; b_.member = nullptr; CHECK(#member, err(b_) == nullptr, 1); } while (0)

static void slide_args() {
    const auto err = [](const SlideBatch& b) { return args_error(b); };
    const char* const too_many = "phys_move_and_slide: n must be below 2^31";
    const char* const bad_skin = "phys_move_and_slide: skin must be finite and not negative";
    const char* const bad_rounds = "phys_move_and_slide: max_slides must be 1 .. 8";
    const char* const null_array = "phys_move_and_slide: null pos, motion, radius, half_length, pos_out or status_out";
    CHECK("args", err(slide_full(3)) == nullptr, 1);
    check_count(slide_full(3), err, too_many);
    check_length(slide_full(3), &SlideBatch::skin, err, bad_skin);
    check_rounds(slide_full(3), &SlideBatch::max_slides, err, bad_rounds);
    CHECK_REQUIRED(slide_full(1), err, pos, null_array); CHECK_REQUIRED(slide_full(1), err, motion, null_array);
    CHECK_REQUIRED(slide_full(1), err, radius, null_array); CHECK_REQUIRED(slide_full(1), err, half_length, null_array);
    CHECK_REQUIRED(slide_full(1), err, pos_out, null_array); CHECK_REQUIRED(slide_full(1), err, status_out, null_array);
    CHECK_OPTIONAL(slide_full(1), err, rot); CHECK_OPTIONAL(slide_full(1), err, ignore_body); CHECK_OPTIONAL(slide_full(1), err, query_mask);
    CHECK_OPTIONAL(slide_full(1), err, remaining_out); CHECK_OPTIONAL(slide_full(1), err, hit_body_out);
    CHECK_OPTIONAL(slide_full(1), err, hit_normal_out); CHECK_OPTIONAL(slide_full(1), err, hit_point_out);
    // the order: the count, the skin, max_slides, the arrays; the per-call values are checked with no queries too
    SlideBatch b = {};
    b.n = 1ull << 31; b.skin = kNaN; CHECK_STR("order", err(b), too_many);
    b.n = 1; CHECK_STR("order", err(b), bad_skin);
    b.skin = 0.0f; CHECK_STR("order", err(b), bad_rounds);
    b.max_slides = 1; CHECK_STR("order", err(b), null_array);
    b.n = 0; CHECK("empty", err(b) == nullptr, 1);
    b.max_slides = 0; CHECK_STR("empty", err(b), bad_rounds);
    b.skin = kInf; CHECK_STR("empty", err(b), bad_skin);
}

static void character_args() {
    const auto err = [](const CharacterBatch& b) { return args_error(b); };
    const char* const too_many = "phys_character_move: n must be below 2^31";
    const char* const bad_skin = "phys_character_move: skin must be finite and not negative";
    const char* const bad_rounds = "phys_character_move: max_slides must be 1 .. 8";
    const char* const bad_step = "phys_character_move: step_height must be finite and not negative";
    const char* const bad_snap = "phys_character_move: snap_distance must be finite and not negative";
    const char* const bad_floor = "phys_character_move: min_floor_ny must lie in (0, 1]";
    const char* const null_array = "phys_character_move: null pos, motion, radius, half_length, pos_out or status_out";
    CHECK("args", err(character_full(3)) == nullptr, 1);
    check_count(character_full(3), err, too_many);
    check_length(character_full(3), &CharacterBatch::skin, err, bad_skin);
    check_rounds(character_full(3), &CharacterBatch::max_slides, err, bad_rounds);
    check_length(character_full(3), &CharacterBatch::step_height, err, bad_step);
    check_length(character_full(3), &CharacterBatch::snap_distance, err, bad_snap);
    // min_floor_ny in (0, 1]: a denormal and 1 pass; 0, -0, the float above 1, NaN and +inf do not
    CharacterBatch b = character_full(3);
    for (float ok : {kDenormal, 0.7071068f, 1.0f}) { b.min_floor_ny = ok; CHECK("min_floor_ny", err(b) == nullptr, 1); }
    for (float bad : {0.0f, -0.0f, std::nextafterf(1.0f, 2.0f), -kDenormal, kNaN, kInf}) { b.min_floor_ny = bad; CHECK_STR("min_floor_ny", err(b), bad_floor); }
    CHECK_REQUIRED(character_full(1), err, pos, null_array); CHECK_REQUIRED(character_full(1), err, motion, null_array);
    CHECK_REQUIRED(character_full(1), err, radius, null_array); CHECK_REQUIRED(character_full(1), err, half_length, null_array);
    CHECK_REQUIRED(character_full(1), err, pos_out, null_array); CHECK_REQUIRED(character_full(1), err, status_out, null_array);
    CHECK_OPTIONAL(character_full(1), err, rot); CHECK_OPTIONAL(character_full(1), err, grounded_in); CHECK_OPTIONAL(character_full(1), err, ignore_body);
    CHECK_OPTIONAL(character_full(1), err, query_mask); CHECK_OPTIONAL(character_full(1), err, remaining_out);
    CHECK_OPTIONAL(character_full(1), err, floor_body_out); CHECK_OPTIONAL(character_full(1), err, floor_normal_out);
    CHECK_OPTIONAL(character_full(1), err, floor_point_out); CHECK_OPTIONAL(character_full(1), err, hit_body_out);
    CHECK_OPTIONAL(character_full(1), err, hit_normal_out); CHECK_OPTIONAL(character_full(1), err, hit_point_out);
    // the order: the count, skin, max_slides, step_height, snap_distance, min_floor_ny, the arrays
    b = CharacterBatch{};
    b.n = 1ull << 31; b.skin = kNaN; b.step_height = kNaN; b.snap_distance = kNaN; CHECK_STR("order", err(b), too_many);
    b.n = 1; CHECK_STR("order", err(b), bad_skin);
    b.skin = 0.0f; CHECK_STR("order", err(b), bad_rounds);
    b.max_slides = 8; CHECK_STR("order", err(b), bad_step);
    b.step_height = 0.0f; CHECK_STR("order", err(b), bad_snap);
    b.snap_distance = 0.0f; CHECK_STR("order", err(b), bad_floor);
    b.min_floor_ny = 1.0f; CHECK_STR("order", err(b), null_array);
    b.n = 0; CHECK("empty", err(b) == nullptr, 1);
    b.min_floor_ny = 0.0f; CHECK_STR("empty", err(b), bad_floor);
}

static void depen_args() {
    const auto err = [](const DepenBatch& b) { return args_error(b); };
    // phys_depenetrate
    const char* too_many = "phys_depenetrate: n must be below 2^31";
    const char* bad_gap = "phys_depenetrate: skin must be finite and not negative";
    const char* const bad_rounds = "phys_depenetrate: max_iters must be 1 .. 8";
    const char* null_array = "phys_depenetrate: null pos, radius, half_length, pos_out or status_out";
    CHECK("args", err(depen_full(3, false)) == nullptr, 1);
    check_count(depen_full(3, false), err, too_many);
    check_length(depen_full(3, false), &DepenBatch::gap, err, bad_gap);
    check_rounds(depen_full(3, false), &DepenBatch::max_iters, err, bad_rounds);
    CHECK_REQUIRED(depen_full(1, false), err, pos, null_array); CHECK_REQUIRED(depen_full(1, false), err, radius, null_array);
    CHECK_REQUIRED(depen_full(1, false), err, half_length, null_array); CHECK_REQUIRED(depen_full(1, false), err, pos_out, null_array);
    CHECK_REQUIRED(depen_full(1, false), err, status_out, null_array);
    CHECK_OPTIONAL(depen_full(1, false), err, rot); CHECK_OPTIONAL(depen_full(1, false), err, ignore_body);
    CHECK_OPTIONAL(depen_full(1, false), err, query_mask); CHECK_OPTIONAL(depen_full(1, false), err, hit_body_out);
    CHECK_OPTIONAL(depen_full(1, false), err, hit_normal_out); CHECK_OPTIONAL(depen_full(1, false), err, hit_depth_out);
    // the order: the count, the skin, max_iters, the arrays
    DepenBatch b = {};
    b.n = 1ull << 31; b.gap = kNaN; CHECK_STR("order", err(b), too_many);
    b.n = 1; CHECK_STR("order", err(b), bad_gap);
    b.gap = 0.0f; CHECK_STR("order", err(b), bad_rounds);
    b.max_iters = 1; CHECK_STR("order", err(b), null_array);
    b.n = 0; CHECK("empty", err(b) == nullptr, 1);
    b.max_iters = 9; CHECK_STR("empty", err(b), bad_rounds);
    // phys_penetration: its own texts and required arrays (body_out and depth_out are the batch's hit_body_out and
    // hit_depth_out); max_iters is the entry point's 1 and is not looked at
    too_many = "phys_penetration: n must be below 2^31";
    bad_gap = "phys_penetration: max_gap must be finite and not negative";
    null_array = "phys_penetration: null pos, radius, half_length, body_out or depth_out";
    CHECK("args", err(depen_full(3, true)) == nullptr, 1);
    check_count(depen_full(3, true), err, too_many);
    check_length(depen_full(3, true), &DepenBatch::gap, err, bad_gap);
    b = depen_full(3, true);
    for (uint32_t any : {0u, 1u, 8u, 9u}) { b.max_iters = any; CHECK("probe max_iters", err(b) == nullptr, 1); }
    CHECK_REQUIRED(depen_full(1, true), err, pos, null_array); CHECK_REQUIRED(depen_full(1, true), err, radius, null_array);
    CHECK_REQUIRED(depen_full(1, true), err, half_length, null_array); CHECK_REQUIRED(depen_full(1, true), err, hit_body_out, null_array);
    CHECK_REQUIRED(depen_full(1, true), err, hit_depth_out, null_array);
    CHECK_OPTIONAL(depen_full(1, true), err, rot); CHECK_OPTIONAL(depen_full(1, true), err, ignore_body);
    CHECK_OPTIONAL(depen_full(1, true), err, query_mask); CHECK_OPTIONAL(depen_full(1, true), err, hit_normal_out);
    CHECK_OPTIONAL(depen_full(1, true), err, pos_out); CHECK_OPTIONAL(depen_full(1, true), err, status_out);
    b = DepenBatch{}; b.probe = true;
    b.n = 1ull << 31; b.gap = kNaN; CHECK_STR("order", err(b), too_many);
    b.n = 1; CHECK_STR("order", err(b), bad_gap);
    b.gap = 0.0f; CHECK_STR("order", err(b), null_array);
    b.n = 0; CHECK("empty", err(b) == nullptr, 1);
    b.gap = kInf; CHECK_STR("empty", err(b), bad_gap);
}

int main() {
    cast_layout();
    overlap_layout();
    bound();
    cast_args();
    slide_layout();
    character_layout();
    depen_layout();
    slide_args();
    character_args();
    depen_args();
    std::printf("staging_probe: %d checks passed\n", g_checks);
    return 0;
}
