// staging.hpp — how a query call describes its arrays, once: a batch struct per family (casts,
// move-and-slide, character walking, depenetration) with its one array list `arrays`, what its entry points check of it
// (args_error), and where a call's host arrays lie in the device buffers they are staged in (StageLayout, stage, staged).
// Host-only like setup.hpp (no HIP, no phys_world), held to tests/cpp/staging_probe.cpp. abi.hip keeps the buffers, the copies
// and the launch: one host path and one device path for every batch here.
//
// A batch's `arrays(b, f)` names every array once, in the order they are staged: f(member, elements per query, group). The
// groups go to a buffer each, so only the order within a group is layout.
#pragma once
#include <cstddef>
#include <cstdint>

namespace phys {

// the buffers a call's arrays are staged in: the inputs, the per-query outputs, and the character's hit slots (that call has
// nine outputs, a layout holds eight arrays)
enum StageGroup { kStageIn, kStageOut, kStageSlots, kStageGroups };

// what every entry point checks of its per-call values, stated once
inline bool count_ok(uint64_t n) { return n < (1ull << 31); }                     // the kernels index queries with 32 bits
inline bool length_ok(float x) { return x >= 0.0f && x <= 3.4028235e38f; }         // finite and not negative (-0 passes, NaN does not)
constexpr uint32_t kSlideMaxSlides = 8, kDepenMaxIters = 8;
inline bool rounds_ok(uint32_t k) { return k >= 1u && k <= 8u; }                   // max_slides, max_iters: "1 .. 8" in the texts
static_assert(kSlideMaxSlides == 8 && kDepenMaxIters == 8, "rounds_ok and the refusal texts say 1 .. 8");

enum class CastKind { Ray, Sphere, Capsule, Box };

// the arrays of one cast call, n queries; host pointers or device pointers alike
struct CastBatch {
    uint64_t n;
    const float *origin, *dir;         // 3 per query
    const float* rot;                  // capsules and boxes: [i, j, k, w] per query; null: identity
    const float *radius, *half_length; // balls and capsules; capsules
    const float* max_t;                // null: +inf
    const uint32_t* ignore_body;       // null: none
    const uint16_t* query_mask;        // null: the plain call, otherwise the _filtered one
    uint32_t* body_out;
    float* t_out;
    float *normal_out, *point_out;     // 3 per query; null: not wanted (point_out: capsules and boxes)
    const float* half_extent;          // boxes: 3 per query (the last member: the kinds before it leave it null)

    template <class Batch, class F>
    static void arrays(Batch& b, F&& f) {
        f(b.origin, 3, kStageIn); f(b.dir, 3, kStageIn); f(b.rot, 4, kStageIn); f(b.radius, 1, kStageIn); f(b.half_length, 1, kStageIn);
        f(b.max_t, 1, kStageIn); f(b.ignore_body, 1, kStageIn); f(b.half_extent, 3, kStageIn); f(b.query_mask, 1, kStageIn);
        f(b.body_out, 1, kStageOut); f(b.t_out, 1, kStageOut); f(b.normal_out, 3, kStageOut); f(b.point_out, 3, kStageOut);
    }
};

// what every entry point of a family checks before it touches anything: the text of the refusal, null when the call may go
// on. Each family names its own required arrays; everything else is optional.
inline const char* args_error(CastKind kind, const CastBatch& b) {
    static const char* const too_many[] = {"phys_raycast: n_rays must be below 2^31", "phys_spherecast: n must be below 2^31",
                                           "phys_capsulecast: n must be below 2^31", "phys_boxcast: n must be below 2^31"};
    static const char* const null_array[] = {"phys_raycast: null origin, dir, body_out or t_out",
                                             "phys_spherecast: null origin, dir, radius, body_out or t_out",
                                             "phys_capsulecast: null origin, dir, radius, half_length, body_out or t_out",
                                             "phys_boxcast: null origin, dir, half_extent, body_out or t_out"};
    if (!count_ok(b.n)) return too_many[(int)kind];
    const bool round = kind == CastKind::Sphere || kind == CastKind::Capsule;
    const bool missing = !b.origin || !b.dir || (round && !b.radius) || (kind == CastKind::Capsule && !b.half_length) ||
                         (kind == CastKind::Box && !b.half_extent) || !b.body_out || !b.t_out;
    return b.n && missing ? null_array[(int)kind] : nullptr;
}

// ---- move-and-slide (phys_move_and_slide): the arrays of one call, n characters; host pointers or device
// pointers alike. Slot k of query i lies at index k * n + i of the hit arrays.
struct SlideBatch {
    uint64_t n;
    const float *pos, *motion;         // 3 per query
    const float* rot;                  // [i, j, k, w] per query; null: identity
    const float *radius, *half_length; // per query
    float skin;                        // the call's: finite, >= 0
    uint32_t max_slides;               // the call's: 1 .. 8
    const uint32_t* ignore_body;       // null: none
    const uint16_t* query_mask;        // null: no filtering
    float *pos_out, *remaining_out;    // 3 per query; remaining_out may be null
    uint32_t* status_out;
    uint32_t* hit_body_out;            // max_slides per query; null: not wanted
    float *hit_normal_out, *hit_point_out;  // 3 * max_slides per query; null: not wanted

    template <class Batch, class F>
    static void arrays(Batch& b, F&& f) {
        const size_t k = b.max_slides;
        f(b.pos, 3, kStageIn); f(b.motion, 3, kStageIn); f(b.rot, 4, kStageIn); f(b.radius, 1, kStageIn); f(b.half_length, 1, kStageIn);
        f(b.ignore_body, 1, kStageIn); f(b.query_mask, 1, kStageIn);
        f(b.pos_out, 3, kStageOut); f(b.remaining_out, 3, kStageOut); f(b.status_out, 1, kStageOut);
        f(b.hit_body_out, k, kStageOut); f(b.hit_normal_out, 3 * k, kStageOut); f(b.hit_point_out, 3 * k, kStageOut);
    }
};

inline const char* args_error(const SlideBatch& b) {
    if (!count_ok(b.n)) return "phys_move_and_slide: n must be below 2^31";
    if (!length_ok(b.skin)) return "phys_move_and_slide: skin must be finite and not negative";
    if (!rounds_ok(b.max_slides)) return "phys_move_and_slide: max_slides must be 1 .. 8";
    const bool missing = !b.pos || !b.motion || !b.radius || !b.half_length || !b.pos_out || !b.status_out;
    return b.n && missing ? "phys_move_and_slide: null pos, motion, radius, half_length, pos_out or status_out" : nullptr;
}

// ---- character walking (phys_character_move): the arrays of one call, n characters; host pointers or
// device pointers alike. Slot k of query i lies at index k * n + i of the hit arrays, 2 * max_slides slots per query.
struct CharacterBatch {
    uint64_t n;
    const float *pos, *motion;         // 3 per query
    const float* rot;                  // [i, j, k, w] per query; null: identity
    const float *radius, *half_length; // per query
    const uint32_t* grounded_in;       // per query, non-zero: stood on a floor when its last call ended; null: nobody did
    float skin;                        // the call's: finite, >= 0
    uint32_t max_slides;               // the call's: 1 .. 8
    float step_height, snap_distance;  // the call's: finite, >= 0
    float min_floor_ny;                // the call's: in (0, 1]
    const uint32_t* ignore_body;       // null: none
    const uint16_t* query_mask;        // null: no filtering
    float *pos_out, *remaining_out;    // 3 per query; remaining_out may be null
    uint32_t* status_out;
    uint32_t* floor_body_out;          // per query; null: not wanted
    float *floor_normal_out, *floor_point_out;  // 3 per query; null: not wanted
    uint32_t* hit_body_out;            // 2 * max_slides per query; null: not wanted
    float *hit_normal_out, *hit_point_out;  // 3 * 2 * max_slides per query; null: not wanted

    template <class Batch, class F>
    static void arrays(Batch& b, F&& f) {
        const size_t k = 2 * (size_t)b.max_slides;
        f(b.pos, 3, kStageIn); f(b.motion, 3, kStageIn); f(b.rot, 4, kStageIn); f(b.radius, 1, kStageIn); f(b.half_length, 1, kStageIn);
        f(b.grounded_in, 1, kStageIn); f(b.ignore_body, 1, kStageIn); f(b.query_mask, 1, kStageIn);
        f(b.pos_out, 3, kStageOut); f(b.remaining_out, 3, kStageOut); f(b.status_out, 1, kStageOut);
        f(b.floor_body_out, 1, kStageOut); f(b.floor_normal_out, 3, kStageOut); f(b.floor_point_out, 3, kStageOut);
        f(b.hit_body_out, k, kStageSlots); f(b.hit_normal_out, 3 * k, kStageSlots); f(b.hit_point_out, 3 * k, kStageSlots);
    }
};

inline const char* args_error(const CharacterBatch& b) {
    if (!count_ok(b.n)) return "phys_character_move: n must be below 2^31";
    if (!length_ok(b.skin)) return "phys_character_move: skin must be finite and not negative";
    if (!rounds_ok(b.max_slides)) return "phys_character_move: max_slides must be 1 .. 8";
    if (!length_ok(b.step_height)) return "phys_character_move: step_height must be finite and not negative";
    if (!length_ok(b.snap_distance)) return "phys_character_move: snap_distance must be finite and not negative";
    if (!(b.min_floor_ny > 0.0f && b.min_floor_ny <= 1.0f)) return "phys_character_move: min_floor_ny must lie in (0, 1]";
    const bool missing = !b.pos || !b.motion || !b.radius || !b.half_length || !b.pos_out || !b.status_out;
    return b.n && missing ? "phys_character_move: null pos, motion, radius, half_length, pos_out or status_out" : nullptr;
}

// ---- depenetration (phys_penetration and phys_depenetrate): the arrays of one call, n capsules; host
// pointers or device pointers alike. probe: phys_penetration, one probe and no move: gap is the call's max_gap, max_iters 1, and
// the one slot per query is the answer (hit_body_out = body_out, hit_normal_out = normal_out, hit_depth_out = depth_out;
// pos_out and status_out null). Otherwise phys_depenetrate: gap is the call's skin, slot k of query i lies at index k * n + i.
struct DepenBatch {
    uint64_t n;
    const float* pos;                  // 3 per query
    const float* rot;                  // [i, j, k, w] per query; null: identity
    const float *radius, *half_length; // per query
    float gap;                         // the call's max_gap or skin: finite, >= 0
    uint32_t max_iters;                // the call's: 1 .. 8
    bool probe;
    const uint32_t* ignore_body;       // null: none
    const uint16_t* query_mask;        // null: no filtering
    float* pos_out;                    // 3 per query
    uint32_t* status_out;
    uint32_t* hit_body_out;            // max_iters per query
    float* hit_normal_out;             // 3 * max_iters per query
    float* hit_depth_out;              // max_iters per query

    template <class Batch, class F>
    static void arrays(Batch& b, F&& f) {
        const size_t k = b.max_iters;
        f(b.pos, 3, kStageIn); f(b.rot, 4, kStageIn); f(b.radius, 1, kStageIn); f(b.half_length, 1, kStageIn);
        f(b.ignore_body, 1, kStageIn); f(b.query_mask, 1, kStageIn);
        f(b.pos_out, 3, kStageOut); f(b.status_out, 1, kStageOut);
        f(b.hit_body_out, k, kStageOut); f(b.hit_normal_out, 3 * k, kStageOut); f(b.hit_depth_out, k, kStageOut);
    }
};

inline const char* args_error(const DepenBatch& b) {
    if (b.probe) {
        if (!count_ok(b.n)) return "phys_penetration: n must be below 2^31";
        if (!length_ok(b.gap)) return "phys_penetration: max_gap must be finite and not negative";
        const bool missing = !b.pos || !b.radius || !b.half_length || !b.hit_body_out || !b.hit_depth_out;
        return b.n && missing ? "phys_penetration: null pos, radius, half_length, body_out or depth_out" : nullptr;
    }
    if (!count_ok(b.n)) return "phys_depenetrate: n must be below 2^31";
    if (!length_ok(b.gap)) return "phys_depenetrate: skin must be finite and not negative";
    if (!rounds_ok(b.max_iters)) return "phys_depenetrate: max_iters must be 1 .. 8";
    const bool missing = !b.pos || !b.radius || !b.half_length || !b.pos_out || !b.status_out;
    return b.n && missing ? "phys_depenetrate: null pos, radius, half_length, pos_out or status_out" : nullptr;
}

// The layout of a call's host arrays in ONE device buffer: a bump allocator. The call declares its arrays in order (add);
// `total` is then the size of the buffer, and at() gives each array's place in it.
struct StageLayout {
    static constexpr int kMaxArrays = 8;
    struct Array { void* host; size_t bytes, offset; };
    template <typename T>
    struct Slot { int index; };  // what add() gives and at() takes: which array of T, -1 when it is not there
    Array arrays[kMaxArrays] = {};
    int count = 0;
    size_t total = 0;
    bool refused = false;  // an array beyond kMaxArrays was declared: the call fails (abi.hip Staging::reserve), nothing is written
    // `n` elements at the next multiple of `align` bytes; a null array takes no room
    template <typename T>
    Slot<T> add(const T* host, size_t n, size_t align = alignof(T)) {
        if (!host) return {-1};
        if (count == kMaxArrays) { refused = true; return {-1}; }
        const size_t offset = (total + align - 1) / align * align;
        arrays[count] = {const_cast<T*>(host), n * sizeof(T), offset};
        total = offset + n * sizeof(T);
        return {count++};
    }
    // the device array of a slot in the buffer at `base`, null for a null host array
    template <typename T>
    T* at(uint8_t* base, Slot<T> s) const {
        return s.index >= 0 && s.index < count ? reinterpret_cast<T*>(base + arrays[s.index].offset) : nullptr;
    }
};

// a call on host arrays declares them, each in its group's layout (Layout: a StageLayout or what abi.hip derives from it) ...
template <class Batch, class Layout>
inline void stage(const Batch& host, Layout (&layouts)[kStageGroups]) {
    Batch::arrays(host, [&](auto* array, size_t per_query, StageGroup g) { layouts[g].add(array, per_query * host.n); });
}
// ... and is the same batch on the device once the buffers are there: the same declarations again, over their bases
template <class Batch>
inline Batch staged(const Batch& host, uint8_t* const (&bases)[kStageGroups]) {
    Batch dev = host;
    StageLayout l[kStageGroups];
    Batch::arrays(dev, [&](auto*& array, size_t per_query, StageGroup g) { array = l[g].at(bases[g], l[g].add(array, per_query * host.n)); });
    return dev;
}

}  // namespace phys
