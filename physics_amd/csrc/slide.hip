// slide.hip — move-and-slide (phys_move_and_slide / phys_move_and_slide_device): a capsule character
// moves along its motion, stops a skin short of what it meets, slides along the contact plane with what is left, and repeats.
//
// A read-only query like the casts (raycast.hip): the query grid is built ONCE per call from the current poses
// (launch_query_grid, grown by the call's largest valid radius + half-length exactly as for a capsule cast: the length of the
// motion does not enter into it), then k_slide gives every lane one character. The lane keeps its state in registers and runs
// the whole loop itself: the capsule cast's own walk (rc_walk, cast_walk.hpp: ground, statics, clip, DDA, cc_contact - the
// one copy k_rc_trace calls too), then the rule of include/spec/slide.h for what the hit does to position and motion. Nothing
// but these two is arithmetic here. The hit slots go straight to global memory, iteration-major (slot k of query i at
// k * n + i: the lanes of a wave write side by side), so nothing in private memory is indexed at run time.
// Lanes of a wave leave the loop at different rounds and wait for the longest: the price of one launch.
// The lane's query is loaded by capsule_query and its slots are written by query_slot (rc_grid.hpp), as in character.hip and
// depen.hip; the host side is the one query path of DESIGN.md section 16, this family's launch_query at the end.
#include "../../include/spec/slide.h"
#include "cast_walk.hpp"

namespace phys {

namespace {

static_assert(SL_MAX_SLIDES == PHYS_SLIDE_MAX_SLIDES && SL_MAX_SLIDES == kSlideMaxSlides, "slide limit mismatch");
static_assert(SL_BLOCKED == PHYS_SLIDE_BLOCKED && SL_EXHAUSTED == PHYS_SLIDE_EXHAUSTED && SL_INVALID == PHYS_SLIDE_INVALID,
              "status flags mismatch");

// where a call's answers go: per query, and the hit slots (each may be null but pos_out and status_out)
struct SlideOut {
    float* pos;
    float* remaining;
    uint32_t* status;
    uint32_t* hit_body;
    float* hit_normal;
    float* hit_point;
};

// FILT: a query_mask was given: a target whose category misses the query's mask is skipped before its exact test (qf is
// read by this instance alone)
template <bool FILT>
__global__ __launch_bounds__(kRcThreads) void k_slide(uint32_t n, const float* __restrict__ pos, const float* __restrict__ motion,
                                                     const float* __restrict__ rot, const float* __restrict__ radius,
                                                     const float* __restrict__ half_length, float skin, uint32_t max_slides,
                                                     const uint32_t* __restrict__ ignore_body, QueryFilters qf,
                                                     const RcHeader* __restrict__ hdr, uint32_t bits, const uint32_t* __restrict__ start,
                                                     const float4* __restrict__ rec, uint32_t n_bodies, int ground, float ground_y,
                                                     const float4* __restrict__ st_rec, uint32_t n_static, SlideOut out) {
    const uint32_t i = blockIdx.x * kRcThreads + threadIdx.x;
    if (i >= n) return;
    const CapsuleQuery c = capsule_query<FILT, true>(i, qf, pos, motion, rot, radius, half_length, ignore_body, n_bodies);
    const uint32_t qm = c.qm, ign = c.ign;
    const v3 p0 = c.p, m0 = c.m;
    const float rad = c.rad, hq = c.hq;
    const quat q = c.q;
    sl_state s;
    sl_begin(&s, p0, m0);
    uint32_t k = 0;  // slots written
    if (!sl_valid(p0, m0, rot != nullptr, q, rad, hq)) {
        s.status = SL_INVALID;
    } else {
        // the capsule's core axis: the y axis of rot, used as given (the capsule cast's rule)
        float ax = 0.0f, ay = 1.0f, az = 0.0f;
        if (rot) rc_capsule_axis(make_float4(q.i, q.j, q.k, q.w), ax, ay, az);
        const bool cap_ok = hq <= 3.4e38f;  // the capsule cast's bound on a half-length (sl_valid: finite and >= 0)
        bool ran_out = true;
        for (; k < max_slides; ++k) {
            const float L = sl_length(s.m);
            if (!(L > 0.0f)) { ran_out = false; break; }
            RayHit best;
            v3 point;
            uint32_t cells = 0, cands = 0;
            rc_walk<false, true, FILT, true>(hdr, bits, start, rec, ground, ground_y, st_rec, n_static, qf, qm, s.p, s.m, L,
                                             sl_max_t(L, skin), ign, rad, hq, ax, ay, az, cap_ok, best, point, cells, cands);
            if (best.id == kRayMiss) { sl_miss(&s); ran_out = false; break; }
            const v3 nrm = v3_make(best.nx, best.ny, best.nz);
            query_slot(out.hit_body, out.hit_normal, out.hit_point, (size_t)k * n + i, best.id, nrm, point);
            if (!sl_hit(&s, L, skin, best.t, nrm)) { ++k; ran_out = false; break; }
        }
        if (ran_out) sl_ran_out(&s);
    }
    query_slots_empty(out.hit_body, out.hit_normal, out.hit_point, 0u, k, max_slides, n, i, v3_make(0.0f, 0.0f, 0.0f));
    st3(out.pos, i, s.p);
    if (out.remaining) st3(out.remaining, i, s.m);
    out.status[i] = s.status;
}

}  // namespace

int32_t launch_query(phys_world* w, const SlideBatch& b) {
    QueryGrid g;
    PHYS_TRY(query_grid(w, b.radius, b.half_length, b.n, &g));
    const QueryFilters qf = query_filters(w, b.query_mask);
    const SlideOut out{b.pos_out, b.remaining_out, b.status_out, b.hit_body_out, b.hit_normal_out, b.hit_point_out};
    dispatch_bool(b.query_mask != nullptr, [&](auto filt) {
        hipLaunchKernelGGL((k_slide<decltype(filt)::value>), dim3(rc_blocks(b.n)), dim3(kRcThreads), 0, w->stream, (uint32_t)b.n, b.pos,
                           b.motion, b.rot, b.radius, b.half_length, b.skin, b.max_slides, b.ignore_body, qf, g.hdr, g.bits, g.start, g.rec,
                           g.n_bodies, g.ground, g.ground_y, g.st_rec, g.n_static, out);
    });
    PHYS_HIP_TRY(hipGetLastError());
    return PHYS_OK;
}

}  // namespace phys
