// depen.hip — depenetration (phys_penetration / phys_depenetrate and their _device twins): how deep a capsule
// sits in the deepest target within a gap of it, and the loop that pushes it out of what it overlaps.
//
// A read-only query like the casts and the overlaps: the query grid is built ONCE per call from the current poses
// (launch_query_grid, not grown, as for phys_overlap), then k_depen gives every lane one capsule. A round is one probe: the lane
// walks the cells its capsule's AABB covers where it stands now (grown by the gap, padded like the bodies' cells; every owned body
// directly, ascending, when the cells outnumber the bodies: k_ov_query's candidate walk without its dedup, which a maximum with
// an id tie-break does not need), then every static, then the ground, and keeps the deepest (include/spec/depenetrate.h:
// dp_target, dp_ground, dp_better over collide.h's capsule functions). dp_step then pushes it or ends the loop. The lane keeps
// its state in registers through all rounds; the slots go straight to global memory, iteration-major (slot k of query i at
// k * n + i), so nothing in private memory is indexed at run time. PROBE = true is the single probe behind phys_penetration: no
// move, slot 0 is the answer.
// The lane's query is loaded by capsule_query and its slots are written by query_slot (rc_grid.hpp), as in slide.hip and
// character.hip; the host side is the one query path of DESIGN.md section 16, this family's launch_query at the end.
#include "../../include/spec/depenetrate.h"
#include "rc_grid.hpp"

namespace phys {

namespace {

static_assert(DP_MAX_ITERS == PHYS_DEPEN_MAX_ITERS && DP_MAX_ITERS == kDepenMaxIters, "depenetration limit mismatch");
static_assert(DP_STUCK == PHYS_DEPEN_STUCK && DP_INVALID == PHYS_DEPEN_INVALID, "status flags mismatch");
static_assert(DP_MISS == PHYS_RAY_MISS && DP_GROUND == PHYS_RAY_GROUND, "target ids mismatch");

// where a call's answers go. PROBE: the slot arrays are the call's body_out, normal_out and depth_out (one slot per query),
// pos and status unused
struct DepenOut {
    float* pos;
    uint32_t* status;
    uint32_t* hit_body;
    float* hit_normal;
    float* hit_depth;
};

// what a probe reads of the world: the grid of launch_query_grid, the bodies' own arrays (the direct path), the statics, the ground
struct DepenWorld {
    const RcHeader* hdr;
    uint32_t bits;
    const uint32_t* start;
    const float4* rec;
    uint32_t n_bodies;
    const float *pos, *rot, *he;
    const uint32_t* shape;
    int ground;
    float ground_y;
    const float4* st_rec;
    uint32_t n_static;
};

__device__ __forceinline__ geom_t depen_geom(v3 c, float4 q4, v3 h, uint32_t type) {
    quat q; q.i = q4.x; q.j = q4.y; q.k = q4.z; q.w = q4.w;
    return geom_make(c, q, h, type);
}

// the deepest target within gap of the capsule (p, a, rad, hq): one probe
template <bool FILT>
__device__ __forceinline__ dp_best depen_probe(const DepenWorld& w, const QueryFilters& qf, uint32_t qm, uint32_t ign, v3 p, v3 a,
                                               float rad, float hq, float gap) {
    dp_best best = dp_none();
    const geom_t Q = dp_capsule(p, a, rad, hq);
    // the capsule's AABB grown by the gap: what a target must touch to come within gap of it
    const float ex = (fabsf(a.x) * hq + rad) + gap, ey = (fabsf(a.y) * hq + rad) + gap, ez = (fabsf(a.z) * hq + rad) + gap;
    aabb_t qa;
    qa.lo = v3_make(p.x - ex, p.y - ey, p.z - ez);
    qa.hi = v3_make(p.x + ex, p.y + ey, p.z + ez);
    const RcGrid g = rc_grid(w.hdr);
    if (g.valid && w.n_bodies) {
        aabb_t qp;  // padded like the bodies' cells
        qp.lo = v3_make(qa.lo.x - g.pad, qa.lo.y - g.pad, qa.lo.z - g.pad);
        qp.hi = v3_make(qa.hi.x + g.pad, qa.hi.y + g.pad, qa.hi.z + g.pad);
        const int x0 = rc_coord(qp.lo.x, g.lox, g.inv, g.nx), x1 = rc_coord(qp.hi.x, g.lox, g.inv, g.nx);
        const int y0 = rc_coord(qp.lo.y, g.loy, g.inv, g.ny), y1 = rc_coord(qp.hi.y, g.loy, g.inv, g.ny);
        const int z0 = rc_coord(qp.lo.z, g.loz, g.inv, g.nz), z1 = rc_coord(qp.hi.z, g.loz, g.inv, g.nz);
        const unsigned long long cells = (unsigned long long)(x1 - x0 + 1) * (unsigned long long)(y1 - y0 + 1) *
                                         (unsigned long long)(z1 - z0 + 1);
        if (cells > w.n_bodies) {
            // more cells than bodies: every owned body directly, in ascending order
            for (uint32_t i = 0; i < w.n_bodies; ++i) {
                aabb_t b;
                if (i == ign || (FILT && (qf.body[i].x & qm) == 0u) || !rc_aabb(w.pos, w.rot, w.he, w.shape, i, &b) || !aabb_overlap(b, qp)) continue;
                const geom_t T = depen_geom(ld3(w.pos, i), reinterpret_cast<const float4*>(w.rot)[i], ld3(w.he, i), w.shape[i]);
                dp_target(&Q, &T, i, gap, &best);
            }
        } else {
            for (int z = z0; z <= z1; ++z)
                for (int y = y0; y <= y1; ++y)
                    for (int x = x0; x <= x1; ++x) {
                        const uint32_t bk = rc_bucket(x, y, z, w.bits);
                        const uint32_t b0 = w.start[bk], b1 = w.start[bk + 1];
                        for (uint32_t k = b0; k < b1; ++k) {
                            const float4 r0 = w.rec[3 * (size_t)k], r1 = w.rec[3 * (size_t)k + 1], r2 = w.rec[3 * (size_t)k + 2];
                            const uint32_t id = __float_as_uint(r2.w);
                            const v3 bc = v3_make(r0.x, r0.y, r0.z), bh = v3_make(r2.x, r2.y, r2.z);
                            aabb_t b;
                            // (a record of another cell hashed to this bucket, or this body's second record: tested again, the same answer)
                            if (id == ign || (FILT && (qf.body[id].x & qm) == 0u) || !rc_aabb_of(bc, r1, bh, __float_as_uint(r0.w), &b) ||
                                !aabb_overlap(b, qp))
                                continue;
                            const geom_t T = depen_geom(bc, r1, bh, __float_as_uint(r0.w));
                            dp_target(&Q, &T, id, gap, &best);
                        }
                    }
        }
    }
    // static colliders, ascending (ids PHYS_STATIC_ID_BIT | k above every body id), rejected by their boxes against the grown box
    // as k_ov_query does it (unpadded: a static within an ulp or two of the gap's edge may go either way, physics_hip.h)
    for (uint32_t k = 0; k < w.n_static; ++k) {
        if (FILT && (qf.st[k].x & qm) == 0u) continue;
        const float4 r0 = w.st_rec[3 * (size_t)k], r1 = w.st_rec[3 * (size_t)k + 1], r2 = w.st_rec[3 * (size_t)k + 2];
        const v3 bc = v3_make(r0.x, r0.y, r0.z), bh = v3_make(r2.x, r2.y, r2.z);
        aabb_t b;
        if (!rc_aabb_of(bc, r1, bh, __float_as_uint(r0.w), &b) || !aabb_overlap(b, qa)) continue;
        const geom_t T = depen_geom(bc, r1, bh, __float_as_uint(r0.w));
        dp_target(&Q, &T, __float_as_uint(r2.w), gap, &best);
    }
    if (w.ground && (!FILT || (qf.ground & qm) != 0u)) dp_ground(&Q, w.ground_y, gap, &best);
    return best;
}

// FILT: a query_mask was given: a target whose category misses the query's mask is skipped before its exact test (qf is read
// by these instances alone). PROBE: phys_penetration (gap = the call's max_gap, max_iters unused); otherwise phys_depenetrate
// (gap = the call's skin)
template <bool FILT, bool PROBE>
__global__ __launch_bounds__(kRcThreads) void k_depen(uint32_t n, const float* __restrict__ pos, const float* __restrict__ rot,
                                                     const float* __restrict__ radius, const float* __restrict__ half_length, float gap,
                                                     uint32_t max_iters, const uint32_t* __restrict__ ignore_body, QueryFilters qf,
                                                     DepenWorld w, DepenOut out) {
    const uint32_t i = blockIdx.x * kRcThreads + threadIdx.x;
    if (i >= n) return;
    const CapsuleQuery c = capsule_query<FILT, false>(i, qf, pos, nullptr, rot, radius, half_length, ignore_body, w.n_bodies);
    const uint32_t qm = c.qm, ign = c.ign;
    const v3 p0 = c.p;
    const float rad = c.rad, hq = c.hq;
    const quat q = c.q;
    const bool valid = dp_valid(p0, rot != nullptr, q, rad, hq);
    // the capsule's core axis: the y axis of rot, used as given (the capsule cast's rule)
    const v3 a = rot ? dp_axis(q) : v3_make(0.0f, 1.0f, 0.0f);
    if (PROBE) {
        // an invalid query is a miss
        const dp_best best = valid ? depen_probe<FILT>(w, qf, qm, ign, p0, a, rad, hq, gap) : dp_none();
        query_slot(out.hit_body, out.hit_normal, out.hit_depth, i, best.id, best.n, best.depth);
        return;
    }
    dp_state s;
    dp_begin(&s, p0);
    uint32_t k = 0;  // slots written
    if (!valid) {
        s.status = DP_INVALID;
    } else {
        for (;; ++k) {
            const dp_best best = depen_probe<FILT>(w, qf, qm, ign, s.p, a, rad, hq, gap);
            if (!dp_step(&s, k, max_iters, gap, &best)) break;
            query_slot(out.hit_body, out.hit_normal, out.hit_depth, (size_t)k * n + i, best.id, best.n, best.depth);
        }
    }
    query_slots_empty(out.hit_body, out.hit_normal, out.hit_depth, 0u, k, max_iters, n, i, 0.0f);
    st3(out.pos, i, s.p);
    out.status[i] = s.status;
}

}  // namespace

int32_t launch_query(phys_world* w, const DepenBatch& b) {
    QueryGrid g;
    PHYS_TRY(query_grid(w, nullptr, nullptr, 0, &g));
    const QueryFilters qf = query_filters(w, b.query_mask);
    const DepenWorld dw{g.hdr, g.bits, g.start, g.rec, g.n_bodies, w->pos.p, w->rot.p, w->half_extent.p, w->shape.p,
                        g.ground, g.ground_y, g.st_rec, g.n_static};
    const DepenOut out{b.pos_out, b.status_out, b.hit_body_out, b.hit_normal_out, b.hit_depth_out};
    dispatch_bool(b.query_mask != nullptr, [&](auto filt) {
        dispatch_bool(b.probe, [&](auto probe) {
            hipLaunchKernelGGL((k_depen<decltype(filt)::value, decltype(probe)::value>), dim3(rc_blocks(b.n)), dim3(kRcThreads), 0, w->stream,
                               (uint32_t)b.n, b.pos, b.rot, b.radius, b.half_length, b.gap, b.max_iters, b.ignore_body, qf, dw, out);
        });
    });
    PHYS_HIP_TRY(hipGetLastError());
    return PHYS_OK;
}

}  // namespace phys
