// character.hip — character walking (phys_character_move / phys_character_move_device): a capsule
// character moves and slides, does not climb what is too steep, steps up, snaps down to the floor and learns what it stands on.
//
// A read-only query like move-and-slide (slide.hip): the query grid is built ONCE per call from the current poses
// (launch_query_grid, grown by the call's largest valid radius + half-length: no motion, step or snap length enters into it),
// then k_character gives every lane one character. The lane keeps the state machine of include/spec/character.h in registers
// and drives it: ch_next names the next cast, the capsule cast's own walk (rc_walk, cast_walk.hpp) makes it at the ONE call
// site below, ch_answer consumes the answer. Nothing but these is arithmetic here. Hit slots and the floor's normal and point
// go straight to global memory as they become known, iteration-major (slot k of query i at k * n + i), so nothing in private
// memory is indexed at run time. Lanes of a wave make different numbers of casts and wait for the longest.
// The slots are written by query_slot and query_slots_empty (rc_grid.hpp), as in slide.hip and depen.hip; the host side is the
// one query path of DESIGN.md section 16, this family's launch_query at the end. The lane's query is loaded here and not by
// capsule_query: with it the kernel compiled to another schedule that was 1.4 and 1.7 % slower on C2 and C3.
#include "../../include/spec/character.h"
#include "cast_walk.hpp"

namespace phys {

namespace {

static_assert(SL_MAX_SLIDES == kSlideMaxSlides, "slide limit mismatch");
static_assert(CH_BLOCKED == PHYS_CHAR_BLOCKED && CH_EXHAUSTED == PHYS_CHAR_EXHAUSTED && CH_INVALID == PHYS_CHAR_INVALID &&
                  CH_GROUNDED == PHYS_CHAR_GROUNDED && CH_STEPPED == PHYS_CHAR_STEPPED && CH_SNAPPED == PHYS_CHAR_SNAPPED &&
                  CH_ON_STEEP == PHYS_CHAR_ON_STEEP && CH_HIT_WALL == PHYS_CHAR_HIT_WALL && CH_HIT_CEILING == PHYS_CHAR_HIT_CEILING,
              "status flags mismatch");
static_assert(CH_MISS == kRayMiss, "miss id mismatch");

// where a call's answers go: per query, the floor, and the hit slots (each may be null but pos_out and status_out)
struct CharacterOut {
    float* pos;
    float* remaining;
    uint32_t* status;
    uint32_t* floor_body;
    float* floor_normal;
    float* floor_point;
    uint32_t* hit_body;
    float* hit_normal;
    float* hit_point;
};

// FILT: a query_mask was given: a target whose category misses the query's mask is skipped before its exact test (qf is
// read by this instance alone)
template <bool FILT>
__global__ __launch_bounds__(kRcThreads) void k_character(uint32_t n, const float* __restrict__ pos, const float* __restrict__ motion,
                                                         const float* __restrict__ rot, const float* __restrict__ radius,
                                                         const float* __restrict__ half_length,
                                                         const uint32_t* __restrict__ grounded_in, float skin, uint32_t max_slides,
                                                         float step_height, float snap_distance, float min_floor_ny,
                                                         const uint32_t* __restrict__ ignore_body, QueryFilters qf,
                                                         const RcHeader* __restrict__ hdr, uint32_t bits,
                                                         const uint32_t* __restrict__ start, const float4* __restrict__ rec,
                                                         uint32_t n_bodies, int ground, float ground_y,
                                                         const float4* __restrict__ st_rec, uint32_t n_static, CharacterOut out) {
    const uint32_t i = blockIdx.x * kRcThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t qm = FILT ? (uint32_t)qf.query_mask[i] : 0xFFFFu;
    const v3 p0 = ld3(pos, i), m0 = ld3(motion, i);
    const float rad = radius[i], hq = half_length[i];
    const uint32_t ign = ignore_body && ignore_body[i] < n_bodies ? ignore_body[i] : 0xFFFFFFFFu;
    quat q; q.i = 0.0f; q.j = 0.0f; q.k = 0.0f; q.w = 1.0f;
    if (rot) { q.i = rot[4 * (size_t)i]; q.j = rot[4 * (size_t)i + 1]; q.k = rot[4 * (size_t)i + 2]; q.w = rot[4 * (size_t)i + 3]; }
    const v3 zero = v3_make(0.0f, 0.0f, 0.0f);
    ch_state s;
    ch_begin(&s, p0, m0, grounded_in ? grounded_in[i] : 0u, skin, max_slides, step_height, snap_distance, min_floor_ny);
    if (!ch_valid(p0, m0, rot != nullptr, q, rad, hq)) {
        s.status = CH_INVALID;
    } else {
        // the capsule's core axis: the y axis of rot, used as given (the capsule cast's rule)
        float ax = 0.0f, ay = 1.0f, az = 0.0f;
        if (rot) rc_capsule_axis(make_float4(q.i, q.j, q.k, q.w), ax, ay, az);
        const bool cap_ok = hq <= 3.4e38f;  // the capsule cast's bound on a half-length (ch_valid: finite and >= 0)
        ch_request req;
        while (ch_next(&s, &req)) {
            RayHit best;
            v3 point;
            uint32_t cells = 0, cands = 0;
            rc_walk<false, true, FILT, true>(hdr, bits, start, rec, ground, ground_y, st_rec, n_static, qf, qm, req.origin, req.dir, req.len,
                                             req.max_t, ign, rad, hq, ax, ay, az, cap_ok, best, point, cells, cands);
            const v3 nrm = v3_make(best.nx, best.ny, best.nz);
            if (req.slot >= 0 && best.id != kRayMiss)
                query_slot(out.hit_body, out.hit_normal, out.hit_point, (size_t)(uint32_t)req.slot * n + i, best.id, nrm, point);
            ch_answer(&s, best.id, best.t, nrm, point);
            if (req.slot == CH_SLOT_FLOOR && ch_floor_found(&s)) query_slot(out.floor_body, out.floor_normal, out.floor_point, i, best.id, nrm, point);
        }
    }
    // the kernel writes every slot: the ones neither slide used are empty
    const uint32_t k_move = s.status & SL_HITS_MASK, k_lift = (s.status >> CH_HITS_SHIFT) & SL_HITS_MASK;
    query_slots_empty(out.hit_body, out.hit_normal, out.hit_point, 0u, k_move, max_slides, n, i, zero);
    query_slots_empty(out.hit_body, out.hit_normal, out.hit_point, max_slides, k_lift, max_slides, n, i, zero);
    if (!ch_floor_found(&s)) query_slot(out.floor_body, out.floor_normal, out.floor_point, i, kRayMiss, zero, zero);
    st3(out.pos, i, s.sl.p);
    if (out.remaining) st3(out.remaining, i, s.sl.m);
    out.status[i] = s.status;
}

}  // namespace

int32_t launch_query(phys_world* w, const CharacterBatch& b) {
    QueryGrid g;
    PHYS_TRY(query_grid(w, b.radius, b.half_length, b.n, &g));
    const QueryFilters qf = query_filters(w, b.query_mask);
    const CharacterOut out{b.pos_out,          b.remaining_out,    b.status_out,  b.floor_body_out, b.floor_normal_out,
                           b.floor_point_out, b.hit_body_out,     b.hit_normal_out, b.hit_point_out};
    dispatch_bool(b.query_mask != nullptr, [&](auto filt) {
        hipLaunchKernelGGL((k_character<decltype(filt)::value>), dim3(rc_blocks(b.n)), dim3(kRcThreads), 0, w->stream, (uint32_t)b.n, b.pos,
                           b.motion, b.rot, b.radius, b.half_length, b.grounded_in, b.skin, b.max_slides, b.step_height, b.snap_distance,
                           b.min_floor_ny, b.ignore_body, qf, g.hdr, g.bits, g.start, g.rec, g.n_bodies, g.ground, g.ground_y, g.st_rec,
                           g.n_static, out);
    });
    PHYS_HIP_TRY(hipGetLastError());
    return PHYS_OK;
}

}  // namespace phys
