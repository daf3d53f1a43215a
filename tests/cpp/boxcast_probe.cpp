// boxcast_probe.cpp — the box cast's arithmetic (include/spec/box_cast.h) with a host compiler alone: no HIP, no library, no grid
// (tests/test_boxcast_cpu.py builds and runs it, once under the address and undefined-behaviour sanitizers). It runs every query
// against every target as the kernel (physics_amd/csrc/boxcast.hip, k_bx_trace) runs it against its candidates: the query's own
// checks, the ground, every target with bx_test under the least (t, id), then bx_contact once for the winner.
//
//   boxcast_probe --args          the argument checks of the four phys_boxcast entry points (physics_amd/csrc/staging.hpp args_error)
//   boxcast_probe <scene file>    prints, per query, the bits of: id t normal[3] point[3]
//
// Scene file, every number a 32-bit word in hex (floats by their bits):
//   n_targets n_queries has_ground ground_y
//   per target: shape id pos[3] rot[4] half_extent[3]
//   per query:  origin[3] dir[3] has_rot rot[4] half_extent[3] max_t ignore
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/spec/box_cast.h"
#include "../../physics_amd/csrc/staging.hpp"

static const uint32_t kMiss = 0xFFFFFFFEu, kGround = 0xFFFFFFFFu;

static uint32_t word(FILE* f) {
    unsigned v = 0;
    if (std::fscanf(f, "%x", &v) != 1) { std::fprintf(stderr, "scene file: short or malformed\n"); std::exit(2); }
    return (uint32_t)v;
}
static float u2f(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static uint32_t f2u(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static float real(FILE* f) { return u2f(word(f)); }
static v3 real3(FILE* f) { v3 r; r.x = real(f); r.y = real(f); r.z = real(f); return r; }
static quat real4(FILE* f) { quat q; q.i = real(f); q.j = real(f); q.k = real(f); q.w = real(f); return q; }
static bool finite3(v3 a) { return bx_finite(a.x) && bx_finite(a.y) && bx_finite(a.z); }

// what every phys_boxcast entry point checks before it touches anything, with the texts of the refusals
static int args() {
    using namespace phys;
    static float f[16];
    static uint32_t u[4];
    static uint16_t m[4];
    int checks = 0;
    const char* too_many = "phys_boxcast: n must be below 2^31";
    const char* null_array = "phys_boxcast: null origin, dir, half_extent, body_out or t_out";
    auto full = [&](uint64_t n) { return CastBatch{n, f, f, f, nullptr, nullptr, f, u, m, u, f, f, f, f}; };
    auto same = [&](const char* got, const char* want) {
        ++checks;
        const std::string g = got ? got : "(none)", w = want ? want : "(none)";
        if (g != w) { std::printf("MISMATCH got \"%s\" expected \"%s\"\n", g.c_str(), w.c_str()); std::exit(1); }
    };
    CastBatch b = full(3);
    same(args_error(CastKind::Box, b), nullptr);
    b = full(3); b.origin = nullptr; same(args_error(CastKind::Box, b), null_array);
    b = full(3); b.dir = nullptr; same(args_error(CastKind::Box, b), null_array);
    b = full(3); b.half_extent = nullptr; same(args_error(CastKind::Box, b), null_array);
    b = full(3); b.body_out = nullptr; same(args_error(CastKind::Box, b), null_array);
    b = full(3); b.t_out = nullptr; same(args_error(CastKind::Box, b), null_array);
    // radius and half_length are not a box cast's; everything else is optional
    b = full(3); b.rot = nullptr; b.max_t = nullptr; b.ignore_body = nullptr; b.query_mask = nullptr; b.normal_out = nullptr; b.point_out = nullptr;
    same(args_error(CastKind::Box, b), nullptr);
    // the count: 2^31 - 1 passes, 2^31 does not, and that is said before a null array is; no queries: nothing is required
    same(args_error(CastKind::Box, full((1ull << 31) - 1)), nullptr);
    same(args_error(CastKind::Box, full(1ull << 31)), too_many);
    b = CastBatch{}; b.n = 1ull << 31; same(args_error(CastKind::Box, b), too_many);
    same(args_error(CastKind::Box, CastBatch{}), nullptr);
    // the other kinds do not ask for half_extent, and a capsule cast's texts are what they were
    b = full(3); b.half_extent = nullptr; b.radius = f; b.half_length = f;
    same(args_error(CastKind::Capsule, b), nullptr);
    b.radius = nullptr;
    same(args_error(CastKind::Capsule, b), "phys_capsulecast: null origin, dir, radius, half_length, body_out or t_out");
    // staged before the mask: seven input arrays, the mask last
    StageLayout l[kStageGroups];
    b = full(3);
    stage(b, l);
    ++checks;
    if (l[kStageIn].refused || l[kStageIn].count != 7 || l[kStageIn].arrays[6].host != (void*)m || l[kStageIn].arrays[5].bytes != 36 ||
        l[kStageOut].count != 4) { std::printf("MISMATCH staging\n"); return 1; }
    std::printf("%d checks passed\n", checks);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: boxcast_probe --args | <scene file>\n"); return 2; }
    if (std::strcmp(argv[1], "--args") == 0) return args();
    FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    const uint32_t nt = word(f), nq = word(f), has_ground = word(f);
    const float ground_y = real(f);
    if (nt > (1u << 20) || nq > (1u << 20)) { std::fprintf(stderr, "scene file: counts out of range\n"); return 2; }
    std::vector<bx_target> tg(nt);
    std::vector<uint32_t> id(nt);
    for (uint32_t k = 0; k < nt; ++k) {
        tg[k].shape = word(f);
        id[k] = word(f);
        tg[k].c = real3(f);
        tg[k].q = real4(f);
        tg[k].h = real3(f);
    }
    for (uint32_t i = 0; i < nq; ++i) {
        const v3 o = real3(f), d = real3(f);
        const uint32_t has_rot = word(f);
        const quat rot = real4(f);
        const v3 he = real3(f);
        const float tmax = real(f);
        const uint32_t ignore = word(f);
        float best_t = BX_INF;
        uint32_t best_id = kMiss, best_k = 0;
        v3 n = v3_make(0.0f, 0.0f, 0.0f), point = v3_make(0.0f, 0.0f, 0.0f);
        const float len = det_sqrtf((d.x * d.x + d.y * d.y) + d.z * d.z);
        if (len > 0.0f && len <= 3.0e38f && finite3(o) && finite3(d) && tmax >= 0.0f && bx_valid(he, has_rot != 0, rot)) {
            const v3 u = v3_make(d.x / len, d.y / len, d.z / len);
            const bx_query q = bx_query_make(o, u, has_rot != 0, rot, he);
            if (has_ground) {
                const float gy = ground_y + bx_ground_reach(&q);
                float t = -1.0f;
                v3 gn = v3_make(0.0f, 0.0f, 0.0f);
                if (o.y <= gy) { t = 0.0f; gn = v3_neg(u); }
                else if (u.y < 0.0f) { t = (gy - o.y) / u.y; gn = v3_make(0.0f, 1.0f, 0.0f); }
                if (t >= 0.0f && t <= tmax) { best_t = t; best_id = kGround; n = gn; }
            }
            for (uint32_t k = 0; k < nt; ++k) {
                if (tg[k].shape != BX_SHAPE_SPHERE && tg[k].shape != BX_SHAPE_BOX && tg[k].shape != BX_SHAPE_CAPSULE) continue;
                if (id[k] == ignore) continue;
                float t;
                v3 tn;
                if (bx_test(&q, &tg[k], &t, &tn) == 0) continue;
                if (t <= tmax && (t < best_t || (t == best_t && id[k] < best_id))) { best_t = t; best_id = id[k]; best_k = k; n = tn; }
            }
            if (best_id == kGround && best_t > 0.0f) point = bx_ground_point(&q, best_t, ground_y);
            else if (best_id != kMiss && best_t > 0.0f) bx_contact(&q, &tg[best_k], best_t, &n, &point);
        }
        std::printf("%08x %08x %08x %08x %08x %08x %08x %08x\n", best_id, f2u(best_t), f2u(n.x), f2u(n.y), f2u(n.z), f2u(point.x), f2u(point.y),
                    f2u(point.z));
    }
    std::fclose(f);
    return 0;
}
