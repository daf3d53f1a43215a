// boxcast.hip — batched box casts against the current poses (phys_boxcast and its _device / _filtered variants; DESIGN.md
// section 30): an oriented box translated along a direction without turning, against the bodies, the statics and the ground.
//
// A read-only query like the other casts: it walks the query grid of launch_query_grid (raycast.hip), grown by the call's largest
// valid |half_extent| (k_bx_grow below writes it into the header's grow slot, as k_sc_grow does for the other sweeps), and writes
// nothing an update or phys_broadphase reads.
//
// k_bx_trace: one query per lane. The ground, then every static, then the DDA of the box's centre line through the grid, every
// candidate tested exactly with bx_test (include/spec/box_cast.h: the whole arithmetic, which a host probe runs too); the walk
// keeps the least (t, id) and the record that gave it, and bx_contact finds the touched point (and, for round targets, the
// normal) once per query after the walk.
// The DDA is rc_walk's (cast_walk.hpp) restated, not a further mode of it (the statics and the cells share one candidate loop here): the kernels that rc_walk is inlined into stay
// instruction for instruction what they were (DESIGN.md section 30 says why that outranks one statement of the loop).
#include <cstdio>

#include "../../include/spec/box_cast.h"
#include "cast_walk.hpp"

namespace phys {

namespace {

static_assert(BX_SHAPE_SPHERE == PHYS_SHAPE_SPHERE && BX_SHAPE_BOX == PHYS_SHAPE_BOX && BX_SHAPE_CAPSULE == PHYS_SHAPE_CAPSULE,
              "shape codes mismatch");
constexpr int kBxMaxGrowBlocks = 1024;

// what the box cast adds to the cast kernels' arguments
struct BoxArgs {
    const float* rot;          // [i, j, k, w] per query; null: identity
    const float* half_extent;  // 3 per query
    float* point_out;          // 3 per query; null: not wanted
};

__device__ __forceinline__ bx_target bx_record(const float4* __restrict__ rec, uint32_t k, uint32_t& id) {
    const float4 a = rec[3 * (size_t)k], q4 = rec[3 * (size_t)k + 1], c = rec[3 * (size_t)k + 2];
    bx_target tg;
    tg.shape = __float_as_uint(a.w);
    tg.c = v3_make(a.x, a.y, a.z);
    tg.q.i = q4.x; tg.q.j = q4.y; tg.q.k = q4.z; tg.q.w = q4.w;
    tg.h = v3_make(c.x, c.y, c.z);
    id = __float_as_uint(c.w);
    return tg;
}

// the least (t, id) so far and the record that gave it, in scalars (a struct handed on by reference ended in private memory in one
// instance)
#define BX_CANDIDATE(REC, K, IS_STATIC, TMAX, IGNORE)                                                          \
    do {                                                                                                       \
        uint32_t id_;                                                                                          \
        const bx_target tg_ = bx_record(REC, K, id_);                                                          \
        float t_;                                                                                              \
        v3 n_;                                                                                                 \
        if (id_ != (IGNORE) && bx_test(&q, &tg_, &t_, &n_) != 0 && t_ <= (TMAX) && (t_ < best_t || (t_ == best_t && id_ < best_id))) { \
            best_t = t_; best_id = id_; bnx = n_.x; bny = n_.y; bnz = n_.z;                                   \
            best_k = K; best_st = IS_STATIC;                                                                   \
        }                                                                                                      \
    } while (0)

template <bool STATS, bool FILT>
__global__ __launch_bounds__(kRcThreads) void k_bx_trace(uint32_t n_casts, const float* __restrict__ origin, const float* __restrict__ dir,
                                                        BoxArgs ba, const float* __restrict__ max_t,
                                                        const uint32_t* __restrict__ ignore_body, const RcHeader* __restrict__ hdr,
                                                        uint32_t bits, const uint32_t* __restrict__ start, const float4* __restrict__ rec,
                                                        uint32_t n_bodies, int ground, float ground_y, const float4* __restrict__ st_rec,
                                                        uint32_t n_static, uint32_t* __restrict__ body_out, float* __restrict__ t_out,
                                                        float* __restrict__ normal_out, unsigned long long* __restrict__ stats,
                                                        QueryFilters qf) {
    const uint32_t r = blockIdx.x * kRcThreads + threadIdx.x;
    if (r >= n_casts) return;
    const uint32_t qm = FILT ? (uint32_t)qf.query_mask[r] : 0xFFFFu;
    uint32_t cells = 0, cands = 0;
    const v3 o = ld3(origin, r), d = ld3(dir, r), he = ld3(ba.half_extent, r);
    const float tmax = max_t ? max_t[r] : __builtin_inff();
    const uint32_t ign = ignore_body && ignore_body[r] < n_bodies ? ignore_body[r] : 0xFFFFFFFFu;
    const float len = rc_length(d);
    quat rot; rot.i = 0.0f; rot.j = 0.0f; rot.k = 0.0f; rot.w = 1.0f;
    if (ba.rot) { rot.i = ba.rot[4 * (size_t)r]; rot.j = ba.rot[4 * (size_t)r + 1]; rot.k = ba.rot[4 * (size_t)r + 2]; rot.w = ba.rot[4 * (size_t)r + 3]; }
    float best_t = __builtin_inff(), bnx = 0.0f, bny = 0.0f, bnz = 0.0f;
    uint32_t best_id = kRayMiss;
    v3 point = v3_make(0.0f, 0.0f, 0.0f);
    const float sum = ((o.x + o.y) + (o.z + d.x)) + (d.y + d.z);
    if (len > 0.0f && len <= 3.0e38f && isfinite(sum) && tmax >= 0.0f && bx_valid(he, ba.rot != nullptr, rot)) {
        const float ux = d.x / len, uy = d.y / len, uz = d.z / len;
        const bx_query q = bx_query_make(o, v3_make(ux, uy, uz), ba.rot != nullptr, rot, he);
        uint32_t best_st = 0u;
        uint32_t best_k = 0;
        // the ground: the solid half-space y <= ground_y, reached by the box's lowest point
        const float gy = ground_y + bx_ground_reach(&q);
        if (ground && (!FILT || (qf.ground & qm) != 0u)) {
            float tg = -1.0f;
            if (o.y <= gy) { tg = 0.0f; bnx = -ux; bny = -uy; bnz = -uz; }
            else if (uy < 0.0f) { tg = (gy - o.y) / uy; bnx = 0.0f; bny = 1.0f; bnz = 0.0f; }
            if (tg >= 0.0f && tg <= tmax) { best_t = tg; best_id = kRayGround; }
            else { bnx = 0.0f; bny = 0.0f; bnz = 0.0f; }
        }
        // One candidate loop, so that the exact test is in the kernel once: first the static colliders, every one tested (before the
        // bodies' walk, so that a static hit shortens it), then cell after cell of the centre line's walk through the grid (rc_walk's
        // DDA: the grid was grown by |he|, so the walk meets every target the box can touch).
        const RcGrid g = rc_grid(hdr);
        const float iux = 1.0f / ux, iuy = 1.0f / uy, iuz = 1.0f / uz;  // +-inf on a zero component
        // (what is uniform or a flag lives in scalar registers, which this kernel runs out of: the walk's flags are integers in
        // vector registers, and a direction's sign is asked of its step each time)
        const int sx = ux > 0.0f ? 1 : (ux < 0.0f ? -1 : 0), sy = uy > 0.0f ? 1 : (uy < 0.0f ? -1 : 0), sz = uz > 0.0f ? 1 : (uz < 0.0f ? -1 : 0);
        const float inf = __builtin_inff();
        uint32_t in_statics = 1u;
        const float4* cur = st_rec;
        uint32_t b0 = 0, b1 = n_static;
        int ix = 0, iy = 0, iz = 0;
        float tx = inf, ty = inf, tz = inf, t1 = 0.0f, tlim = tmax;
        // a walk never takes more steps than the grid has cells along the three axes (also bounds a NaN walk)
        int steps = g.nx + g.ny + g.nz + 3;
        for (;;) {
            for (uint32_t k = b0; k < b1; ++k) {
                if (FILT) {
                    const uint32_t cat = in_statics ? qf.st[k].x : qf.body[__float_as_uint(cur[3 * (size_t)k + 2].w)].x;
                    if ((cat & qm) == 0u) continue;
                }
                BX_CANDIDATE(cur, k, in_statics, tlim, in_statics ? 0xFFFFFFFFu : ign);
            }
            if (in_statics) {
                in_statics = 0u;
                cur = rec;
                // clip to the grid box and to [0, min(max_t, best)] (bodies win ties with the ground: best_t itself stays in)
                const float hx = g.lox + (float)g.nx * g.cell, hy = g.loy + (float)g.ny * g.cell, hz = g.loz + (float)g.nz * g.cell;
                float t0 = 0.0f;
                t1 = fminf(tmax, best_t);
                bool hit_box = g.valid;
                if (ux == 0.0f) hit_box = hit_box && o.x >= g.lox && o.x <= hx;
                else { const float a = (g.lox - o.x) * iux, b = (hx - o.x) * iux; t0 = fmaxf(t0, fminf(a, b)); t1 = fminf(t1, fmaxf(a, b)); }
                if (uy == 0.0f) hit_box = hit_box && o.y >= g.loy && o.y <= hy;
                else { const float a = (g.loy - o.y) * iuy, b = (hy - o.y) * iuy; t0 = fmaxf(t0, fminf(a, b)); t1 = fminf(t1, fmaxf(a, b)); }
                if (uz == 0.0f) hit_box = hit_box && o.z >= g.loz && o.z <= hz;
                else { const float a = (g.loz - o.z) * iuz, b = (hz - o.z) * iuz; t0 = fmaxf(t0, fminf(a, b)); t1 = fminf(t1, fmaxf(a, b)); }
                if (!(hit_box && t0 <= t1)) break;
                tlim = fminf(tmax, best_t);
                ix = rc_coord(o.x + t0 * ux, g.lox, g.inv, g.nx);
                iy = rc_coord(o.y + t0 * uy, g.loy, g.inv, g.ny);
                iz = rc_coord(o.z + t0 * uz, g.loz, g.inv, g.nz);
                tx = sx ? rc_plane_t(ix, sx > 0, g.lox, g.cell, o.x, iux) : inf;
                ty = sy ? rc_plane_t(iy, sy > 0, g.loy, g.cell, o.y, iuy) : inf;
                tz = sz ? rc_plane_t(iz, sz > 0, g.loz, g.cell, o.z, iuz) : inf;
            } else {
                const float texit = fminf(tx, fminf(ty, tz));  // of the cell just tested
                if (best_t <= texit || texit > t1) break;
                if (--steps <= 0) break;
                const bool stepx = tx <= ty && tx <= tz, stepy = !stepx && ty <= tz, stepz = !stepx && !stepy;
                ix += stepx ? sx : 0; iy += stepy ? sy : 0; iz += stepz ? sz : 0;
                if (ix < 0 || ix >= g.nx || iy < 0 || iy >= g.ny || iz < 0 || iz >= g.nz) break;
                tx = stepx ? rc_plane_t(ix, sx > 0, g.lox, g.cell, o.x, iux) : tx;
                ty = stepy ? rc_plane_t(iy, sy > 0, g.loy, g.cell, o.y, iuy) : ty;
                tz = stepz ? rc_plane_t(iz, sz > 0, g.loz, g.cell, o.z, iuz) : tz;
            }
            const uint32_t bk = rc_bucket(ix, iy, iz, bits);
            b0 = start[bk]; b1 = start[bk + 1];
            if (STATS) { cells += 1; cands += b1 - b0; }
        }
        // the contact, once per query
        if (best_id == kRayGround && best_t > 0.0f) {
            point = bx_ground_point(&q, best_t, ground_y);
        } else if (best_id != kRayMiss && best_t > 0.0f) {
            uint32_t id;
            const bx_target tg = bx_record(best_st ? st_rec : rec, best_k, id);
            v3 n = v3_make(bnx, bny, bnz);
            bx_contact(&q, &tg, best_t, &n, &point);
            bnx = n.x; bny = n.y; bnz = n.z;
        }
    }
    body_out[r] = best_id;
    t_out[r] = best_t;
    if (normal_out) st3(normal_out, r, v3_make(bnx, bny, bnz));
    if (ba.point_out) st3(ba.point_out, r, point);
    if (STATS) { atomicAdd(&stats[0], (unsigned long long)cells); atomicAdd(&stats[1], (unsigned long long)cands); }
}

// the largest bx_grow over the call's valid half extents into the header's grow slot: non-negative floats order as their bits,
// so one atomicMax per workgroup (k_sc_grow's scheme)
__global__ __launch_bounds__(kRcThreads) void k_bx_grow(uint32_t n, const float* __restrict__ half_extent, RcHeader* __restrict__ hdr) {
    float m = 0.0f;
    quat none; none.i = 0.0f; none.j = 0.0f; none.k = 0.0f; none.w = 1.0f;
    for (uint32_t i = blockIdx.x * kRcThreads + threadIdx.x; i < n; i += gridDim.x * kRcThreads) {
        const v3 he = ld3(half_extent, i);
        if (bx_valid(he, 0, none)) m = fmaxf(m, bx_grow(he));
    }
    const auto op_fmax = [](float a, float b) { return fmaxf(a, b); };
    __shared__ float red[kRcThreads / 64];
    block_put(m, red, op_fmax);
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(&hdr->grow, __float_as_uint(block_get<kRcThreads>(red, op_fmax)));
}

#undef BX_CANDIDATE

}  // namespace

void launch_box_grow(phys_world* w, const float* half_extent, uint64_t n) {
    hipLaunchKernelGGL(k_bx_grow, dim3(std::min<unsigned>(rc_blocks(n), kBxMaxGrowBlocks)), dim3(kRcThreads), 0, w->stream, (uint32_t)n,
                       half_extent, reinterpret_cast<RcHeader*>(w->rc_header.p));
}

int32_t launch_boxcast(phys_world* w, const CastBatch& b) {
    hipStream_t s = w->stream;
    const BoxArgs ba{b.rot, b.half_extent, b.point_out};
    QueryGrid g;
    PHYS_TRY(query_grid(w, nullptr, nullptr, b.n, &g, b.half_extent));
    const bool stats = debug_switches().raycast_stats;
    if (stats) {
        PHYS_HIP_TRY(w->rc_stats.resize(2));
        PHYS_HIP_TRY(hipMemsetAsync(w->rc_stats.p, 0, 16, s));
    }
    const QueryFilters qf = query_filters(w, b.query_mask);
    dispatch_bool(stats, [&](auto st) {
        dispatch_bool(b.query_mask != nullptr, [&](auto filt) {
            hipLaunchKernelGGL((k_bx_trace<decltype(st)::value, decltype(filt)::value>), dim3(rc_blocks(b.n)), dim3(kRcThreads), 0, s,
                               (uint32_t)b.n, b.origin, b.dir, ba, b.max_t, b.ignore_body, g.hdr, g.bits, g.start, g.rec, g.n_bodies,
                               g.ground, g.ground_y, g.st_rec, g.n_static, b.body_out, b.t_out, b.normal_out, w->rc_stats.p, qf);
        });
    });
    PHYS_HIP_TRY(hipGetLastError());
    if (stats) {
        unsigned long long h[2] = {0, 0};
        PHYS_HIP_TRY(hipMemcpyAsync(h, w->rc_stats.p, 16, hipMemcpyDeviceToHost, s));
        PHYS_HIP_TRY(hipStreamSynchronize(s));
        fprintf(stderr, "PHYS_BOXCAST_STATS rays=%llu cells=%llu candidates=%llu\n", (unsigned long long)b.n, h[0], h[1]);
    }
    return PHYS_OK;
}

}  // namespace phys
